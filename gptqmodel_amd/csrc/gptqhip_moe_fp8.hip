// Fused FP8 (float8_e4m3fn) mixture-of-experts decode ops (include/gptqhip.h: gptqhip_moe_fp8_gate_up / gptqhip_moe_fp8_down /
// gptqhip_moe_fp8_supported): the device-routed few-token path of gptqhip_moe.hip on the weight format and arithmetic of gptqhip_fp8.hip.
//
// The experts' weights are in the FP8 kernel layout (gptqhip_fp8_repack: 2 KiB per (16-column tile, 128-row chunk) block, the chunks of a tile
// contiguous) and STACKED at a constant stride; the routing (ids int32 [T, top_k], weights float32 [T, top_k]) stays on the DEVICE, and two
// launches whose grids depend only on (T, top_k, shapes) serve T <= 16 tokens: no host read of the router output, capturable in a graph.
//
//   moe_fp8_gate_up_kernel  grid (2I / 16 column tiles, T * top_k slots), min(8, chunks) waves; slot s = t * top_k + j reads x[t] and expert ids[s].
//                           The fused gate|up weight interleaves gate and up rows in blocks of 8, so a 16-column tile holds both halves of 8 MLP
//                           neurons.  Fixed-order LDS reduction over the waves, then the SiLU * up rounding chain (gptqhip_moe_common.h: moe_silu_up).
//   moe_fp8_down_kernel     grid (H / 16 column tiles, T tokens); the block's waves are dealt to the token's top_k slots (wps = min(16 / top_k,
//                           chunks) waves per slot), park their fp32 partial sums in LDS, and wave 0 combines them: ONE fp32 weighted sum in slot
//                           order, ONE rounding (the combine contract, gptqhip_moe_common.h: moe_combine_slots).
//
// A wave's work item is one 2 KiB block: two non-temporal 16 B-per-lane loads, the codes converted EXACTLY to fp16 / bf16 (fp8x8_to_frag, the packed
// convert), and ONE 16 B-per-lane load of the chunk's 128 activations with the masked K-steps of gptqhip_moe_common.h.  Up to four chunks' loads
// are in flight (32 + 16 + 1 VGPRs per chunk).  Wave w of W takes the CONTIGUOUS chunk range [w * chunks / W, (w + 1) * chunks / W): a function
// of the shape alone, and one that keeps a wave inside as few K blocks as possible.
//
// SCALES (reciprocals, formed once by gptqhip_fp8_repack).  gate|up carries one scale row per fused column: [E, 2I] or [E, 2I, H / bc]; down is
// [E] | [E, H] | [E, H / br, I / bc].  With K-block scales the fp32 accumulator is multiplied by the reciprocal scale and flushed at every bc
// boundary of a wave's share; otherwise the scale multiplies the reduced sum once in the epilogue.
//
// Expert ids outside [0, E) dereference nothing: the slot contributes zero (gate_up writes zeros for it) and the device status word is set to 1.
// NaN codes (0x7f, 0xff) are undefined, as in gptqhip_fp8.hip.  LDS: 16 x 16 floats; no floating-point atomics: two runs give the same bits.
#include "gptqhip_fp8_frag.h"
#include "gptqhip_moe_common.h"

namespace gptqhip {

struct MoeFp8Params {
    const uint16_t* x;       // gate_up: [T, H]; down: act [T * top_k, I]
    const uint8_t* wt;       // stacked kernel-layout weights
    const float* rs;         // stacked reciprocal scales
    const int32_t* ids;      // [T * top_k]
    const float* weights;    // [T * top_k] (down)
    uint16_t* out;           // gate_up: act [T * top_k, I]; down: [T, H]
    int32_t* status;
    size_t w_stride;         // bytes between two experts' weights
    size_t s_stride;         // floats between two experts' scales
    int top_k, E, K, N;      // N: columns of the stacked projection (2I / H)
    int chunks;              // 128-row chunks of K
    int mode;                // GPTQHIP_FP8_SCALE_* (gate_up: row or block)
    int br, kbn, cpb;        // block scales: weight rows per scale row, scales per weight row (K / bc), chunks per scale (bc / 128)
    int wps;                 // down: waves per slot
};

// fp32 partial dot products of one 16-column tile over chunks [c0, c1), c0 < c1: lanes 0 .. 15 return the column sums, the rest 0.
// wt: the tile's first block + 16 * lane; rs (BLOCK): this lane's column's scale row.
template <int ACT, bool BLOCK>
__device__ __forceinline__ float fp8_wave_partial(const uint8_t* __restrict__ wt, const float* __restrict__ rs, const uint16_t* __restrict__ xrow,
                                                  int c0, int c1, int cpb, int lane) {
    const int c16 = lane & 15, rq = lane >> 4;
    uint32_t mask[4];
    moe_kstep_masks(c16, mask);
    const uint16_t* xl = xrow + 32 * (c16 & 3) + 8 * rq;
    const f4_t zero = {0.f, 0.f, 0.f, 0.f};
    f4_t acc = zero, tot = zero;
    for (int base = c0; base < c1; base += kMoeAhead) {
        u4_t w[kMoeAhead][2], a[kMoeAhead];
        float r[kMoeAhead];
#pragma unroll
        for (int u = 0; u < kMoeAhead; ++u) {
            const int ck = base + u < c1 ? base + u : c1 - 1;   // past the end: a harmless repeat of the wave's last chunk
            w[u][0] = __builtin_nontemporal_load(reinterpret_cast<const u4_t*>(wt + (size_t)ck * kFp8BlockBytes));
            w[u][1] = __builtin_nontemporal_load(reinterpret_cast<const u4_t*>(wt + (size_t)ck * kFp8BlockBytes + 1024));
            a[u] = *reinterpret_cast<const u4_t*>(xl + (size_t)ck * kChunkK);
            r[u] = BLOCK ? rs[ck / cpb] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < kMoeAhead; ++u) {
            const int ck = base + u;
            if (ck < c1) {   // wave-uniform
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const u4_t& wh = w[u][j >> 1];   // K-step j = 2 h + jj: half h, bytes 8 jj .. 8 jj + 7 of the lane's 16
                    const u4_t b = (j & 1) ? fp8x8_to_frag<ACT, kCvtPacked>(wh.z, wh.w) : fp8x8_to_frag<ACT, kCvtPacked>(wh.x, wh.y);
                    acc = mfma16<ACT>(moe_masked_a(a[u], mask[j]), b, acc);
                }
                if (BLOCK && ((ck + 1) % cpb == 0 || ck + 1 == c1)) {   // the K block (or the wave's share of it) ends here
                    tot += acc * r[u];
                    acc = zero;
                }
            }
        }
    }
    return moe_lane_sum(BLOCK ? tot : acc, rq);
}

template <int ACT, bool BLOCK>
__global__ __launch_bounds__(64 * kMoeGateUpWaves) void moe_fp8_gate_up_kernel(MoeFp8Params p) {
    __shared__ float red[kMoeGateUpWaves][16];
    const int tile = blockIdx.x, slot = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, W = blockDim.x >> 6;
    const int inter = p.N >> 1;
    const int e = p.ids[slot];
    uint16_t* out8 = p.out + (size_t)slot * inter + tile * 8;
    if (moe_gate_up_invalid(e, p.E, out8, p.status)) return;
    const int n = tile * kTileN + (lane & 15);
    const uint8_t* wt = p.wt + (size_t)e * p.w_stride + (size_t)tile * p.chunks * kFp8BlockBytes + lane * 16;
    const float* rs = p.rs + (size_t)e * p.s_stride + (size_t)n * p.kbn;   // row scales: kbn = 1, one scale per column
    const uint16_t* xrow = p.x + (size_t)(slot / p.top_k) * p.K;
    const int c0 = wave * p.chunks / W, c1 = (wave + 1) * p.chunks / W;    // W <= chunks: every wave owns at least one chunk
    const float part = fp8_wave_partial<ACT, BLOCK>(wt, rs, xrow, c0, c1, p.cpb, lane);
    if (lane < 16) red[wave][lane] = part;
    __syncthreads();
    if (wave != 0) return;
    float v = 0.f;
    for (int w = 0; w < W; ++w) v += red[w][lane & 15];   // wave order, always
    if (!BLOCK) v *= rs[0];
    const uint16_t a = moe_silu_up<ACT>(v);   // lanes 0 .. 7 hold gate columns, lanes 8 .. 15 the matching up columns
    if (lane < 8) out8[lane] = a;
}

// float offset of (expert's) scale for column n of the down projection, tensor / row layouts
__device__ __forceinline__ size_t down_scale_index(const MoeFp8Params& p, int e, int n) {
    return (size_t)e * p.s_stride + (p.mode == GPTQHIP_FP8_SCALE_ROW ? n : 0);
}

template <int ACT, bool BLOCK>
__global__ __launch_bounds__(64 * kMoeDownWaves) void moe_fp8_down_kernel(MoeFp8Params p) {
    __shared__ float red[kMoeDownWaves][16];
    const int tile = blockIdx.x, t = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = wave / p.wps, sub = wave - j * p.wps;   // this wave's slot and its share of the slot's chunks
    const int slot = t * p.top_k + j;
    const int e = p.ids[slot];
    const int n = tile * kTileN + (lane & 15);
    float part = 0.f;
    if (e >= 0 && e < p.E) {   // wave-uniform
        const uint8_t* wt = p.wt + (size_t)e * p.w_stride + (size_t)tile * p.chunks * kFp8BlockBytes + lane * 16;
        const float* rs = BLOCK ? p.rs + (size_t)e * p.s_stride + (size_t)(n / p.br) * p.kbn : p.rs;
        const int c0 = sub * p.chunks / p.wps, c1 = (sub + 1) * p.chunks / p.wps;   // wps <= chunks
        part = fp8_wave_partial<ACT, BLOCK>(wt, rs, p.x + (size_t)slot * p.K, c0, c1, p.cpb, lane);
    } else if (lane == 0) {
        *p.status = 1;
    }
    if (lane < 16) red[wave][lane] = part;
    __syncthreads();
    // block scales are already in the partial sums; tensor / row scales multiply each slot's reduced dot product
    moe_combine_slots<ACT>(red, wave, lane, p.ids + t * p.top_k, p.weights + t * p.top_k, p.top_k, p.E, p.wps, p.out + (size_t)t * p.N + tile * kTileN,
                           [&](float d, int ej) { return BLOCK ? d : d * p.rs[down_scale_index(p, ej, n)]; });
}

// K, N, mode, br, bc: the projection the call runs
static int moe_fp8_validate(const char* fn, const void* const* ptrs16, int n16, const void* const* ptrs4, int n4, int T, int top_k, int E, int H, int I,
                            int K, int N, int mode, int br, int bc, int act_dtype) {
    int rc = moe_check_ptrs(fn, ptrs16, n16, "activations, weights and outputs", ptrs4, n4, "reciprocal scales, ids, routing weights and status");
    if (!rc) rc = moe_check_few_tokens(fn, T, top_k, E);
    if (rc) return rc;
    return moe_check_fp8_shape(fn, H, I, K, N, mode, br, bc, act_dtype);
}

static MoeFp8Params moe_fp8_params(const void* x, const uint8_t* wt, const float* rs, const int32_t* ids, const float* weights, void* out,
                                   int32_t* status, int top_k, int E, int K, int N, int mode, int br, int bc) {
    MoeFp8Params p;
    p.x = reinterpret_cast<const uint16_t*>(x);
    p.wt = wt;
    p.rs = rs;
    p.ids = ids;
    p.weights = weights;
    p.out = reinterpret_cast<uint16_t*>(out);
    p.status = status;
    p.top_k = top_k;
    p.E = E;
    p.K = K;
    p.N = N;
    p.chunks = K / kChunkK;
    p.mode = mode;
    const bool block = mode == GPTQHIP_FP8_SCALE_BLOCK;
    p.br = block ? br : 1;
    p.kbn = block ? K / bc : 1;
    p.cpb = block ? bc / kChunkK : p.chunks;
    p.w_stride = (size_t)K * N;
    p.s_stride = mode == GPTQHIP_FP8_SCALE_TENSOR ? 1 : mode == GPTQHIP_FP8_SCALE_ROW ? (size_t)N : (size_t)(N / br) * p.kbn;
    p.wps = 1;
    return p;
}

}  // namespace gptqhip

using namespace gptqhip;

extern "C" {

int gptqhip_moe_fp8_supported(int H, int I, int gate_up_block_cols, int down_scale_mode, int down_block_rows, int down_block_cols, int T, int top_k,
                              int act_dtype) {
    return moe_fp8_layouts_ok(H, I, gate_up_block_cols, down_scale_mode, down_block_rows, down_block_cols, act_dtype) && moe_few_tokens_ok(T, top_k) ? 1 : 0;
}

int gptqhip_moe_fp8_gate_up(const void* x, const uint8_t* weight_t, const float* rscale, const int32_t* ids, void* act, int32_t* status, int T,
                            int top_k, int E, int H, int I, int block_cols, int act_dtype, gptqhip_stream_t stream) {
    const void* p16[] = {x, weight_t, act};
    const void* p4[] = {rscale, ids, status};
    const int mode = block_cols == 0 ? GPTQHIP_FP8_SCALE_ROW : GPTQHIP_FP8_SCALE_BLOCK;
    int rc = moe_fp8_validate("gptqhip_moe_fp8_gate_up", p16, 3, p4, 3, T, top_k, E, H, I, H, 2 * I, mode, 1, block_cols, act_dtype);
    if (rc) return rc;
    const MoeFp8Params p = moe_fp8_params(x, weight_t, rscale, ids, nullptr, act, status, top_k, E, H, 2 * I, mode, 1, block_cols);
    const int waves = p.chunks < kMoeGateUpWaves ? p.chunks : kMoeGateUpWaves;
    const dim3 grid(2 * I / kTileN, T * top_k), block(64 * waves);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const bool blk = mode == GPTQHIP_FP8_SCALE_BLOCK;
    if (act_dtype == GPTQHIP_FP16) {
        if (blk) hipLaunchKernelGGL((moe_fp8_gate_up_kernel<kFP16, true>), grid, block, 0, s, p);
        else hipLaunchKernelGGL((moe_fp8_gate_up_kernel<kFP16, false>), grid, block, 0, s, p);
    } else {
        if (blk) hipLaunchKernelGGL((moe_fp8_gate_up_kernel<kBF16, true>), grid, block, 0, s, p);
        else hipLaunchKernelGGL((moe_fp8_gate_up_kernel<kBF16, false>), grid, block, 0, s, p);
    }
    return check_hip(hipGetLastError(), "moe_fp8_gate_up_kernel launch");
}

int gptqhip_moe_fp8_down(const void* act, const uint8_t* weight_t, const float* rscale, const int32_t* ids, const float* weights, void* out,
                         int32_t* status, int T, int top_k, int E, int H, int I, int scale_mode, int block_rows, int block_cols, int act_dtype,
                         gptqhip_stream_t stream) {
    const void* p16[] = {act, weight_t, out};
    const void* p4[] = {rscale, ids, weights, status};
    int rc = moe_fp8_validate("gptqhip_moe_fp8_down", p16, 3, p4, 4, T, top_k, E, H, I, I, H, scale_mode, block_rows, block_cols, act_dtype);
    if (rc) return rc;
    MoeFp8Params p = moe_fp8_params(act, weight_t, rscale, ids, weights, out, status, top_k, E, I, H, scale_mode, block_rows, block_cols);
    const int per_slot = kMoeDownWaves / top_k;
    p.wps = p.chunks < per_slot ? p.chunks : per_slot;
    const dim3 grid(H / kTileN, T), block(64 * p.wps * top_k);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const bool blk = scale_mode == GPTQHIP_FP8_SCALE_BLOCK;
    if (act_dtype == GPTQHIP_FP16) {
        if (blk) hipLaunchKernelGGL((moe_fp8_down_kernel<kFP16, true>), grid, block, 0, s, p);
        else hipLaunchKernelGGL((moe_fp8_down_kernel<kFP16, false>), grid, block, 0, s, p);
    } else {
        if (blk) hipLaunchKernelGGL((moe_fp8_down_kernel<kBF16, true>), grid, block, 0, s, p);
        else hipLaunchKernelGGL((moe_fp8_down_kernel<kBF16, false>), grid, block, 0, s, p);
    }
    return check_hip(hipGetLastError(), "moe_fp8_down_kernel launch");
}

}  // extern "C"
