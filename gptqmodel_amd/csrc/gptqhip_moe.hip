// Fused quantised mixture-of-experts decode ops (include/gptqhip.h: gptqhip_moe_gate_up / gptqhip_moe_down / gptqhip_moe_supported).
//
// A sparse-MoE block picks top_k of E experts per token; each expert is a SiLU MLP of three GPTQ linears.  The experts' tiled words and meta
// constants are STACKED at a constant stride (expert e = base + e * gptqhip_tiled_words / gptqhip_meta_words), the routing (ids int32
// [T, top_k], weights float32 [T, top_k]) stays on the DEVICE, and two launches whose grids depend only on (T, top_k, shapes) serve a few
// tokens (T <= 16): no host read of the router output, so the step can be captured in a graph.
//
//   moe_gate_up_kernel   grid (2I / 16 column tiles, T * top_k slots); slot s = t * top_k + j reads x[t] and expert ids[s].  The fused gate|up
//                        projection's columns are interleaved in blocks of 8 (utils.model.fuse_gate_up_interleaved), so a 16-column tile holds both
//                        halves of 8 MLP neurons and the epilogue writes act[s, 8 tile .. 8 tile + 8) directly, with the SiLU * up rounding chain
//                        (gptqhip_moe_common.h: moe_silu_up).
//   moe_down_kernel      grid (H / 16 column tiles, T tokens); the block's waves are dealt to the token's top_k slots (wps waves per slot, each taking
//                        every wps-th 128-row chunk of its slot's expert), park their fp32 partial sums in LDS, and wave 0 combines them: ONE fp32
//                        weighted sum in slot order, ONE rounding (the combine contract, gptqhip_moe_common.h: moe_combine_slots).
//
// Both kernels contract on the matrix pipe like the decode kernel at one row, with per-weight rounding kept (dequant_word4: the reference's
// W = round(scale * (code - zero)), bit-faithful as in decode form 4).  A wave's work item is one (16-column tile, 128-row chunk) block:
//   * ONE non-temporal 16 B-per-lane load = the block's 1 KiB of codes, one 4 B-per-lane load of the group constants (group_size = 128 * 2^n:
//     one constant per chunk and column), and ONE 16 B-per-lane load of the chunk's 128 activations: lane (rq, c) takes the 8 values of K-step
//     (c & 3), rows 8 rq .. 8 rq + 7 (the masked K-steps of gptqhip_moe_common.h).
//   * up to four chunks' loads are issued before the first is consumed (16 + 16 + 4 VGPRs per chunk in flight).
// LDS: 16 x 16 floats of reduction rows (1 KiB); VGPRs stay under 128, so the 1024-thread down blocks launch and 2048 threads fit a CU.
//
// Expert ids outside [0, E) dereference nothing: the slot contributes zero (gate_up writes zeros for it) and the device status word is set to 1.
#include "gptqhip_moe_common.h"

namespace gptqhip {

struct MoeParams {
    const uint16_t* x;       // gate_up: [T, H]; down: act [T * top_k, I]
    const uint32_t* qw;      // stacked tiled words
    const uint32_t* meta;    // stacked constants
    const int32_t* ids;      // [T * top_k]
    const float* weights;    // [T * top_k] (down)
    uint16_t* out;           // gate_up: act [T * top_k, I]; down: [T, H]
    int32_t* status;
    size_t w_stride, m_stride;   // words between two experts
    int top_k, E, K, N;          // N: columns of the stacked projection (2I / H)
    int chunks, cpg, G;          // 128-row chunks of K, chunks per group, groups
    int wps;                     // down: waves per slot
};

// fp32 partial dot products of columns 16 tile .. 16 tile + 15 over chunks ck0, ck0 + step, ..: lanes 0 .. 15 return the column sums, the rest 0.
template <int ACT, int SCL>
__device__ __forceinline__ float wave_partial(const uint32_t* __restrict__ wt, const uint32_t* __restrict__ mt, const uint16_t* __restrict__ xrow,
                                              int ck0, int step, int chunks, int cpg, int lane) {
    const DequantConsts kc = make_dequant_consts<4>();
    const int c16 = lane & 15, rq = lane >> 4;
    uint32_t mask[4];
    moe_kstep_masks(c16, mask);
    const uint16_t* xl = xrow + 32 * (c16 & 3) + 8 * rq;
    f4_t acc = {0.f, 0.f, 0.f, 0.f};
    for (int base = ck0; base < chunks; base += step * kMoeAhead) {
        u4_t w[kMoeAhead], a[kMoeAhead];
        uint32_t m[kMoeAhead];
#pragma unroll
        for (int u = 0; u < kMoeAhead; ++u) {
            const int ck = base + u * step < chunks ? base + u * step : base;   // past the end: a harmless repeat of an in-range chunk
            w[u] = __builtin_nontemporal_load(reinterpret_cast<const u4_t*>(wt + (size_t)ck * 256 + lane * 4));
            a[u] = *reinterpret_cast<const u4_t*>(xl + (size_t)ck * kChunkK);
            m[u] = mt[(ck / cpg) * 16 + c16];
        }
#pragma unroll
        for (int u = 0; u < kMoeAhead; ++u) {
            if (base + u * step < chunks) {   // wave-uniform
                const ColConst cc = expand_meta<4, SCL>(m[u]);
#pragma unroll
                for (int j = 0; j < 4; ++j) acc = mfma16<ACT>(moe_masked_a(a[u], mask[j]), dequant_word4<ACT, SCL>(w[u][j], cc, kc), acc);
            }
        }
    }
    return moe_lane_sum(acc, rq);
}

template <int ACT, int SCL>
__global__ __launch_bounds__(64 * kMoeGateUpWaves) void moe_gate_up_kernel(MoeParams p) {
    __shared__ float red[kMoeGateUpWaves][16];
    const int tile = blockIdx.x, slot = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, W = blockDim.x >> 6;
    const int inter = p.N >> 1;
    const int e = p.ids[slot];
    uint16_t* out8 = p.out + (size_t)slot * inter + tile * 8;
    if (moe_gate_up_invalid(e, p.E, out8, p.status)) return;
    const uint32_t* wt = p.qw + (size_t)e * p.w_stride + (size_t)tile * p.chunks * 256;
    const uint32_t* mt = p.meta + (size_t)e * p.m_stride + (size_t)tile * p.G * 16;
    const uint16_t* xrow = p.x + (size_t)(slot / p.top_k) * p.K;
    const float part = wave_partial<ACT, SCL>(wt, mt, xrow, wave, W, p.chunks, p.cpg, lane);
    if (lane < 16) red[wave][lane] = part;
    __syncthreads();
    if (wave != 0) return;
    float v = 0.f;
    for (int w = 0; w < W; ++w) v += red[w][lane & 15];
    const uint16_t a = moe_silu_up<ACT>(v);   // lanes 0 .. 7 hold gate columns, lanes 8 .. 15 the matching up columns
    if (lane < 8) out8[lane] = a;
}

template <int ACT, int SCL>
__global__ __launch_bounds__(64 * kMoeDownWaves) void moe_down_kernel(MoeParams p) {
    __shared__ float red[kMoeDownWaves][16];
    const int tile = blockIdx.x, t = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = wave / p.wps, sub = wave - j * p.wps;   // this wave's slot and its share of the slot's chunks
    const int slot = t * p.top_k + j;
    const int e = p.ids[slot];
    float part = 0.f;
    if (e >= 0 && e < p.E) {   // wave-uniform
        const uint32_t* wt = p.qw + (size_t)e * p.w_stride + (size_t)tile * p.chunks * 256;
        const uint32_t* mt = p.meta + (size_t)e * p.m_stride + (size_t)tile * p.G * 16;
        part = wave_partial<ACT, SCL>(wt, mt, p.x + (size_t)slot * p.K, sub, p.wps, p.chunks, p.cpg, lane);
    } else if (lane == 0) {
        *p.status = 1;
    }
    if (lane < 16) red[wave][lane] = part;
    __syncthreads();
    moe_combine_slots<ACT>(red, wave, lane, p.ids + t * p.top_k, p.weights + t * p.top_k, p.top_k, p.E, p.wps, p.out + (size_t)t * p.N + tile * 16,
                           [](float d, int) { return d; });
}

static int moe_validate(const char* fn, const void* const* ptrs16, int n16, const void* const* ptrs4, int n4, int T, int top_k, int E, int H, int I,
                        int K, int group_size, int bits, int act_dtype, int scale_dtype) {
    int rc = moe_check_ptrs(fn, ptrs16, n16, "activations, weights, constants and outputs", ptrs4, n4, "ids, weights and status");
    if (!rc) rc = moe_check_few_tokens(fn, T, top_k, E);
    if (!rc) rc = moe_check_int4_shape(fn, H, I, K, group_size, bits);
    if (!rc) rc = moe_check_dtypes(fn, act_dtype, scale_dtype);
    return rc;
}

static MoeParams moe_params(const void* x, const uint32_t* qw, const uint32_t* meta, const int32_t* ids, const float* weights, void* out,
                            int32_t* status, int top_k, int E, int K, int N, int group_size) {
    MoeParams p;
    p.x = reinterpret_cast<const uint16_t*>(x);
    p.qw = qw;
    p.meta = meta;
    p.ids = ids;
    p.weights = weights;
    p.out = reinterpret_cast<uint16_t*>(out);
    p.status = status;
    p.w_stride = gptqhip_tiled_words(K, N, 4);
    p.m_stride = gptqhip_meta_words(K, N, group_size);
    p.top_k = top_k;
    p.E = E;
    p.K = K;
    p.N = N;
    p.chunks = K / kChunkK;
    p.cpg = group_size / kChunkK;
    p.G = K / group_size;
    p.wps = 1;
    return p;
}

}  // namespace gptqhip

using namespace gptqhip;

extern "C" {

int gptqhip_moe_supported(int H, int I, int group_size, int bits, int has_perm, int T, int top_k) {
    if (has_perm) return 0;
    // group_size <= 0: one group for the whole K of each projection (group_size = -1 checkpoints)
    return moe_int4_shape_ok(H, I, H, group_size <= 0 ? H : group_size, bits) && moe_int4_shape_ok(H, I, I, group_size <= 0 ? I : group_size, bits) &&
                   moe_few_tokens_ok(T, top_k)
               ? 1
               : 0;
}

int gptqhip_moe_gate_up(const void* x, const uint32_t* qweight_t, const uint32_t* meta, const int32_t* ids, void* act, int32_t* status,
                        int T, int top_k, int E, int H, int I, int group_size, int bits, int act_dtype, int scale_dtype,
                        gptqhip_stream_t stream) {
    const void* p16[] = {x, qweight_t, meta, act};
    const void* p4[] = {ids, status};
    int rc = moe_validate("gptqhip_moe_gate_up", p16, 4, p4, 2, T, top_k, E, H, I, H, group_size, bits, act_dtype, scale_dtype);
    if (rc) return rc;
    const MoeParams p = moe_params(x, qweight_t, meta, ids, nullptr, act, status, top_k, E, H, 2 * I, group_size);
    const int waves = p.chunks < kMoeGateUpWaves ? p.chunks : kMoeGateUpWaves;
    const dim3 grid(2 * I / kTileN, T * top_k), block(64 * waves);
    moe_dispatch(act_dtype, scale_dtype, [&](auto a, auto s) {
        hipLaunchKernelGGL((moe_gate_up_kernel<decltype(a)::value, decltype(s)::value>), grid, block, 0, reinterpret_cast<hipStream_t>(stream), p);
    });
    return check_hip(hipGetLastError(), "moe_gate_up_kernel launch");
}

int gptqhip_moe_down(const void* act, const uint32_t* qweight_t, const uint32_t* meta, const int32_t* ids, const float* weights, void* out,
                     int32_t* status, int T, int top_k, int E, int H, int I, int group_size, int bits, int act_dtype, int scale_dtype,
                     gptqhip_stream_t stream) {
    const void* p16[] = {act, qweight_t, meta, out};
    const void* p4[] = {ids, weights, status};
    int rc = moe_validate("gptqhip_moe_down", p16, 4, p4, 3, T, top_k, E, H, I, I, group_size, bits, act_dtype, scale_dtype);
    if (rc) return rc;
    MoeParams p = moe_params(act, qweight_t, meta, ids, weights, out, status, top_k, E, I, H, group_size);
    const int per_slot = kMoeDownWaves / top_k;
    p.wps = p.chunks < per_slot ? p.chunks : per_slot;
    const dim3 grid(H / kTileN, T), block(64 * p.wps * top_k);
    moe_dispatch(act_dtype, scale_dtype, [&](auto a, auto s) {
        hipLaunchKernelGGL((moe_down_kernel<decltype(a)::value, decltype(s)::value>), grid, block, 0, reinterpret_cast<hipStream_t>(stream), p);
    });
    return check_hip(hipGetLastError(), "moe_down_kernel launch");
}

}  // extern "C"
