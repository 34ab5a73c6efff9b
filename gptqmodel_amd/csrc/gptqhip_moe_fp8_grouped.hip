// Expert-grouped fused FP8 (float8_e4m3fn) MoE stages (include/gptqhip.h: gptqhip_moe_fp8_gate_up_grouped / gptqhip_moe_fp8_down_grouped /
// gptqhip_moe_fp8_grouped_supported): the matrix stage of the expert-grouped pipeline of gptqhip_moe_grouped.hip on the weight format, stacked
// scale layout and arithmetic of gptqhip_moe_fp8.hip, for ANY number of tokens.  The two format-agnostic launches around it are the int4 path's:
//
//   gptqhip_moe_align -> gptqhip_moe_fp8_gate_up_grouped -> gptqhip_moe_fp8_down_grouped -> gptqhip_moe_combine
//
// gptqhip_moe_fp8.hip serves T <= 16 with one block per (tile, slot), so an expert is streamed once per slot that routes to it; here every 16-row
// UNIT of one expert (moe_align's sorted_slots / unit_expert) streams the expert's tile once with all 16 MFMA rows carrying real tokens.
//
//   moe_fp8_grouped_kernel  grid (N / 16 column tiles, max_units); unit u >= num_units exits.  Row m of the unit is slot sorted_slots[16 u + m];
//                           lane (rq, m) loads A[m][32 j + 8 rq ..] of K-step j straight from that slot's activation row (GATE_UP: x[s / top_k];
//                           DOWN: act[s]; a padded row reads the unit's row 0 and stores nothing).  B: expert unit_expert[u]'s 2 KiB (tile, chunk)
//                           block as two non-temporal 16 B-per-lane loads, fp8x8_to_frag per K-step -- the fragment order fp8_decode_kernel
//                           (gptqhip_fp8.hip) feeds to the matrix pipe with four natural-order A fragments per chunk.  Wave w of
//                           W = min(kFp8GroupedGateUpWaves | kFp8GroupedDownWaves, chunks) takes the CONTIGUOUS chunk range
//                           [w * chunks / W, (w + 1) * chunks / W) with kFp8GroupedAhead chunks' loads in flight: W and the deal are functions of
//                           the shape alone, rows of a unit never mix, so a token's bits do not depend on its batch.
//                           The waves park their 16 x 16 fp32 accumulators in LDS and threads 0 .. 255 add them in wave order.
//                             GATE_UP: the SiLU * up rounding chain (gptqhip_moe_common.h: moe_silu_up), scattered to act[slot, 8 tile .. 8 tile + 8)
//                             DOWN:    the unrounded, already-scaled fp32 dot products, scattered to part[slot, 16 tile .. 16 tile + 16);
//                                      moe_combine_kernel's w * part is then (d * rscale) * w, the product order of moe_fp8_down_kernel.
//
// SCALES (reciprocals, 4-byte loads, the stacked layout of gptqhip_moe_fp8.hip).  A lane's scale depends on its column only.  K-block scales: the
// fp32 accumulator is multiplied by rs[e][(n / br) * kbn + ck / cpb] (gate|up: br = 1) and flushed at every bc boundary and at the end of the
// wave's share; tensor / row scales multiply the wave-order-reduced sum once in the epilogue.
//
// Nothing is dereferenced through an id or slot moe_align would never produce.  No floating-point atomics: two runs give the same bits.  The K
// summation order differs from gptqhip_moe_fp8.hip: same contract, not the same bits.  Registers / LDS / scratch per kernel: DESIGN.md 4.6.1.
#include "gptqhip_fp8_frag.h"
#include "gptqhip_moe_common.h"

namespace gptqhip {

constexpr int kFp8GroupedGateUpWaves = 8;
constexpr int kFp8GroupedDownWaves = 16;
constexpr int kFp8GroupedAhead = 2;        // chunks whose loads a wave issues before consuming the first (8 + 16 + 1 VGPRs per chunk)

struct Fp8GroupedParams {
    const uint16_t* x;            // GATE_UP: [T, H]; DOWN: act [S, I]
    const uint8_t* wt;            // stacked kernel-layout weights
    const float* rs;              // stacked reciprocal scales
    const int32_t* sorted_slots;
    const int32_t* unit_expert;
    const int32_t* num_units;
    void* out;                    // GATE_UP: act [S, I] 16-bit; DOWN: part [S, H] fp32
    size_t w_stride;              // bytes between two experts' weights
    size_t s_stride;              // floats between two experts' scales
    int S, row_div, E, K, N;      // row_div: slots per activation row (top_k for GATE_UP, 1 for DOWN)
    int chunks, max_units;
    int mode;                     // GPTQHIP_FP8_SCALE_* (GATE_UP: row or block)
    int br, kbn, cpb;             // block scales: weight rows per scale row, scales per weight row (K / bc), chunks per scale (bc / 128)
};

template <int ACT, bool BLOCK, bool GATE_UP, int MAXW>
__global__ __launch_bounds__(64 * MAXW) void moe_fp8_grouped_kernel(Fp8GroupedParams p) {
    __shared__ float red[MAXW][kUnitRows][16];
    __shared__ int slots[kUnitRows];
    const int tile = blockIdx.x, unit = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, W = blockDim.x >> 6;
    int nu = *p.num_units;
    nu = nu < p.max_units ? nu : p.max_units;
    if (unit >= nu) return;                                   // block-uniform
    const int e = p.unit_expert[unit];
    const int slot0 = p.sorted_slots[unit * kUnitRows];
    if (e < 0 || e >= p.E || slot0 < 0 || slot0 >= p.S) return;   // never produced by moe_align; nothing is dereferenced through it
    const int c16 = lane & 15, rq = lane >> 4;
    int slot = p.sorted_slots[unit * kUnitRows + c16];
    if (slot < 0 || slot >= p.S) slot = -1;
    if (threadIdx.x < kUnitRows) slots[threadIdx.x] = slot;
    const uint8_t* wt = p.wt + (size_t)e * p.w_stride + (size_t)tile * p.chunks * kFp8BlockBytes + lane * 16;
    const float* rse = p.rs + (size_t)e * p.s_stride;
    const float* rs = BLOCK ? rse + (size_t)((tile * kTileN + c16) / p.br) * p.kbn : rse;   // this lane's column's scale row
    // lane (rq, m): A[m][32 j + 8 rq .. + 7] of K-step j
    const uint16_t* xl = p.x + (size_t)((slot < 0 ? slot0 : slot) / p.row_div) * p.K + 8 * rq;
    const int c0 = wave * p.chunks / W, c1 = (wave + 1) * p.chunks / W;   // W <= chunks: every wave owns at least one chunk
    const f4_t zero = {0.f, 0.f, 0.f, 0.f};
    f4_t acc = zero, tot = zero;
    for (int base = c0; base < c1; base += kFp8GroupedAhead) {
        u4_t w[kFp8GroupedAhead][2], a[kFp8GroupedAhead][4];
        float r[kFp8GroupedAhead];
#pragma unroll
        for (int u = 0; u < kFp8GroupedAhead; ++u) {
            const int ck = base + u < c1 ? base + u : c1 - 1;   // past the end: a harmless repeat of the wave's last chunk
            w[u][0] = __builtin_nontemporal_load(reinterpret_cast<const u4_t*>(wt + (size_t)ck * kFp8BlockBytes));
            w[u][1] = __builtin_nontemporal_load(reinterpret_cast<const u4_t*>(wt + (size_t)ck * kFp8BlockBytes + 1024));
#pragma unroll
            for (int j = 0; j < 4; ++j) a[u][j] = *reinterpret_cast<const u4_t*>(xl + (size_t)ck * kChunkK + 32 * j);
            r[u] = BLOCK ? rs[ck / p.cpb] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < kFp8GroupedAhead; ++u) {
            const int ck = base + u;
            if (ck < c1) {   // wave-uniform
                acc = mfma16<ACT>(a[u][0], fp8x8_to_frag<ACT, kCvtPacked>(w[u][0].x, w[u][0].y), acc);
                acc = mfma16<ACT>(a[u][1], fp8x8_to_frag<ACT, kCvtPacked>(w[u][0].z, w[u][0].w), acc);
                acc = mfma16<ACT>(a[u][2], fp8x8_to_frag<ACT, kCvtPacked>(w[u][1].x, w[u][1].y), acc);
                acc = mfma16<ACT>(a[u][3], fp8x8_to_frag<ACT, kCvtPacked>(w[u][1].z, w[u][1].w), acc);
                if (BLOCK && ((ck + 1) % p.cpb == 0 || ck + 1 == c1)) {   // the K block (or the wave's share of it) ends here
                    tot += acc * r[u];
                    acc = zero;
                }
            }
        }
    }
    // accumulator register i of lane (rq, n) = row 4 rq + i, column n
#pragma unroll
    for (int i = 0; i < 4; ++i) red[wave][4 * rq + i][c16] = BLOCK ? tot[i] : acc[i];
    __syncthreads();
    for (int t = threadIdx.x; t < kUnitRows * 16; t += blockDim.x) {   // (t and t + 8 sit in one wave in the same trip: the shuffle below is safe)
        const int mrow = t >> 4, n = t & 15;
        float v = 0.f;
        for (int ww = 0; ww < W; ++ww) v += red[ww][mrow][n];   // wave order, always
        if (!BLOCK) v *= rse[p.mode == GPTQHIP_FP8_SCALE_ROW ? tile * kTileN + n : 0];
        const int s = slots[mrow];
        if constexpr (GATE_UP) {
            const uint16_t r = moe_silu_up<ACT>(v);   // columns 0 .. 7 are gate columns, 8 .. 15 the matching up columns
            if (n < 8 && s >= 0) reinterpret_cast<uint16_t*>(p.out)[(size_t)s * (p.N >> 1) + tile * 8 + n] = r;
        } else {
            if (s >= 0) reinterpret_cast<float*>(p.out)[(size_t)s * p.N + tile * 16 + n] = v;
        }
    }
}

// K, N, mode, br, bc: the projection the call runs
static int fp8_grouped_validate(const char* fn, const void* const* ptrs16, int n16, const void* const* ptrs4, int n4, int T, int top_k, int E, int H,
                                int I, int K, int N, int mode, int br, int bc, int act_dtype) {
    int rc = moe_check_ptrs(fn, ptrs16, n16, "activations, weights, partial sums and outputs", ptrs4, n4, "reciprocal scales and sort buffers");
    if (!rc) rc = grouped_check_routing(fn, T, top_k, E);
    if (!rc) rc = moe_check_fp8_shape(fn, H, I, K, N, mode, br, bc, act_dtype);
    return rc;
}

static Fp8GroupedParams fp8_grouped_params(const void* x, const uint8_t* wt, const float* rs, const int32_t* sorted_slots, const int32_t* unit_expert,
                                           const int32_t* num_units, void* out, int S, int row_div, int E, int K, int N, int mode, int br, int bc) {
    Fp8GroupedParams p;
    p.x = reinterpret_cast<const uint16_t*>(x);
    p.wt = wt;
    p.rs = rs;
    p.sorted_slots = sorted_slots;
    p.unit_expert = unit_expert;
    p.num_units = num_units;
    p.out = out;
    p.S = S;
    p.row_div = row_div;
    p.E = E;
    p.K = K;
    p.N = N;
    p.chunks = K / kChunkK;
    p.max_units = grouped_units(S, E);
    p.mode = mode;
    const bool block = mode == GPTQHIP_FP8_SCALE_BLOCK;
    p.br = block ? br : 1;
    p.kbn = block ? K / bc : 1;
    p.cpb = block ? bc / kChunkK : p.chunks;
    p.w_stride = (size_t)K * N;
    p.s_stride = mode == GPTQHIP_FP8_SCALE_TENSOR ? 1 : mode == GPTQHIP_FP8_SCALE_ROW ? (size_t)N : (size_t)(N / br) * p.kbn;
    return p;
}

template <bool GATE_UP, int MAXW>
static void fp8_grouped_launch(int act_dtype, const Fp8GroupedParams& p, dim3 grid, dim3 block, hipStream_t s) {
    const bool blk = p.mode == GPTQHIP_FP8_SCALE_BLOCK;
    if (act_dtype == GPTQHIP_FP16) {
        if (blk) hipLaunchKernelGGL((moe_fp8_grouped_kernel<kFP16, true, GATE_UP, MAXW>), grid, block, 0, s, p);
        else hipLaunchKernelGGL((moe_fp8_grouped_kernel<kFP16, false, GATE_UP, MAXW>), grid, block, 0, s, p);
    } else {
        if (blk) hipLaunchKernelGGL((moe_fp8_grouped_kernel<kBF16, true, GATE_UP, MAXW>), grid, block, 0, s, p);
        else hipLaunchKernelGGL((moe_fp8_grouped_kernel<kBF16, false, GATE_UP, MAXW>), grid, block, 0, s, p);
    }
}

}  // namespace gptqhip

using namespace gptqhip;

extern "C" {

int gptqhip_moe_fp8_grouped_supported(int H, int I, int gate_up_block_cols, int down_scale_mode, int down_block_rows, int down_block_cols, int T,
                                      int top_k, int E, int act_dtype) {
    return moe_fp8_layouts_ok(H, I, gate_up_block_cols, down_scale_mode, down_block_rows, down_block_cols, act_dtype) && grouped_routing_ok(T, top_k, E)
               ? 1
               : 0;
}

int gptqhip_moe_fp8_gate_up_grouped(const void* x, const uint8_t* weight_t, const float* rscale, const int32_t* sorted_slots,
                                    const int32_t* unit_expert, const int32_t* num_units, void* act, int T, int top_k, int E, int H, int I,
                                    int block_cols, int act_dtype, gptqhip_stream_t stream) {
    const void* p16[] = {x, weight_t, act};
    const void* p4[] = {rscale, sorted_slots, unit_expert, num_units};
    const int mode = block_cols == 0 ? GPTQHIP_FP8_SCALE_ROW : GPTQHIP_FP8_SCALE_BLOCK;
    int rc = fp8_grouped_validate("gptqhip_moe_fp8_gate_up_grouped", p16, 3, p4, 4, T, top_k, E, H, I, H, 2 * I, mode, 1, block_cols, act_dtype);
    if (rc) return rc;
    const Fp8GroupedParams p =
        fp8_grouped_params(x, weight_t, rscale, sorted_slots, unit_expert, num_units, act, T * top_k, top_k, E, H, 2 * I, mode, 1, block_cols);
    const int waves = p.chunks < kFp8GroupedGateUpWaves ? p.chunks : kFp8GroupedGateUpWaves;
    fp8_grouped_launch<true, kFp8GroupedGateUpWaves>(act_dtype, p, dim3(2 * I / kTileN, p.max_units), dim3(64 * waves),
                                                     reinterpret_cast<hipStream_t>(stream));
    return check_hip(hipGetLastError(), "moe_fp8_grouped_kernel (gate_up) launch");
}

int gptqhip_moe_fp8_down_grouped(const void* act, const uint8_t* weight_t, const float* rscale, const int32_t* sorted_slots,
                                 const int32_t* unit_expert, const int32_t* num_units, float* part, int T, int top_k, int E, int H, int I,
                                 int scale_mode, int block_rows, int block_cols, int act_dtype, gptqhip_stream_t stream) {
    const void* p16[] = {act, weight_t, part};
    const void* p4[] = {rscale, sorted_slots, unit_expert, num_units};
    int rc = fp8_grouped_validate("gptqhip_moe_fp8_down_grouped", p16, 3, p4, 4, T, top_k, E, H, I, I, H, scale_mode, block_rows, block_cols,
                                  act_dtype);
    if (rc) return rc;
    const Fp8GroupedParams p = fp8_grouped_params(act, weight_t, rscale, sorted_slots, unit_expert, num_units, part, T * top_k, 1, E, I, H, scale_mode,
                                                  block_rows, block_cols);
    const int waves = p.chunks < kFp8GroupedDownWaves ? p.chunks : kFp8GroupedDownWaves;
    fp8_grouped_launch<false, kFp8GroupedDownWaves>(act_dtype, p, dim3(H / kTileN, p.max_units), dim3(64 * waves),
                                                    reinterpret_cast<hipStream_t>(stream));
    return check_hip(hipGetLastError(), "moe_fp8_grouped_kernel (down) launch");
}

}  // extern "C"
