// Expert-grouped fused MoE ops (include/gptqhip.h: gptqhip_moe_align / gptqhip_moe_gate_up_grouped / gptqhip_moe_down_grouped /
// gptqhip_moe_combine): the device-routed experts path for ANY number of tokens.  gptqhip_moe.hip serves T <= 16 with one block per (tile, slot),
// so every slot streams its expert's weights on its own; here the S = T * top_k slots are sorted by expert on the device and every 16-row UNIT of
// one expert runs through the matrix pipe with all 16 MFMA rows carrying real tokens.  All grids depend only on (T, top_k, E, shapes).
//
//   moe_align_kernel     ONE block of 16 waves: a stable counting sort of the slots by expert id.  Wave w owns the contiguous slot range
//                        [w * per, (w + 1) * per); pass 1 counts cnt[w][e] (integer LDS atomics: the counts do not depend on their order), thread e
//                        then turns column e into exclusive prefixes over the waves and a block scan of ceil(total_e / 16) gives expert e its first
//                        unit; pass 2 walks each wave's slots in ascending order 64 at a time, a lane's rank among the lanes of its step with the
//                        same expert coming from ballots over the id's bits.  Every position is a pure function of the ids: no ordering by atomics.
//                        Every word of sorted_slots / unit_expert / num_units is written exactly once (slots, padding, tail).
//   moe_grouped_kernel   grid (N / 16 column tiles, max_units); unit u >= num_units exits.  Row m of the unit is slot sorted_slots[16 u + m]; lane
//                        (rq, m) loads A[m][32 j + 8 rq ..] of K-step j from that slot's activation row (a padded row reads the unit's row 0 and
//                        stores nothing), the B fragments are dequant_word4 of the tiled words of expert unit_expert[u].  The block's waves split
//                        the 128-row chunks (wave w takes w, w + W, ..), park their 16 x 16 fp32 accumulators in LDS and threads 0 .. 255 add them
//                        in wave order.  Rows of a unit never mix, and W depends on the shape alone: a token's bits do not depend on its batch.
//                          GATE_UP: the SiLU * up rounding chain (gptqhip_moe_common.h: moe_silu_up), scattered to act[slot, 8 tile .. 8 tile + 8)
//                          DOWN:    the unrounded fp32 dot products, scattered to part[slot, 16 tile .. 16 tile + 16)
//   moe_combine_kernel   out[t, n] = act( sum_j weights[t, j] * part[t * top_k + j, n] ), fp32, slot order, ONE rounding, ids outside [0, E) skipped:
//                        the combine contract of gptqhip_moe_common.h on 4-wide vectors.  No floating-point atomics anywhere.
//
// Registers / LDS / scratch per kernel: DESIGN.md 4.4.
#include "gptqhip_moe_common.h"

namespace gptqhip {

// (kUnitRows, grouped_units, the routing limits and their checks: gptqhip_moe_common.h, shared with gptqhip_moe_fp8_grouped.hip)
constexpr int kAlignWaves = 16;            // waves of the align block
constexpr int kGroupedGateUpWaves = 8;
constexpr int kGroupedDownWaves = 16;
constexpr int kGroupedAhead = 2;           // chunks whose loads a wave issues before consuming the first

struct AlignParams {
    const int32_t* ids;
    int32_t* sorted_slots;
    int32_t* unit_expert;
    int32_t* num_units;
    int32_t* status;
    int S, E, max_units;
};

__global__ __launch_bounds__(64 * kAlignWaves) void moe_align_kernel(AlignParams p) {
    extern __shared__ int cnt[];                 // [kAlignWaves][E]
    __shared__ int wsum[kAlignWaves];
    __shared__ int start_row[kGroupedMaxExperts];   // first sorted row of expert e
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int S = p.S, E = p.E;
    for (int i = tid; i < kAlignWaves * E; i += blockDim.x) cnt[i] = 0;
    __syncthreads();
    // pass 1: per-wave, per-expert counts
    const int per = ((S + kAlignWaves * 64 - 1) / (kAlignWaves * 64)) * 64;   // slots per wave, a multiple of 64
    const int s0 = wave * per, s1 = s0 + per < S ? s0 + per : S;
    bool bad = false;
    for (int s = s0 + lane; s < s1; s += 64) {
        const int e = p.ids[s];
        if (e >= 0 && e < E) atomicAdd(&cnt[wave * E + e], 1);
        else bad = true;
    }
    if (bad) *p.status = 1;
    __syncthreads();
    // thread e: exclusive prefixes over the waves, units of expert e, block scan of the units
    int total = 0, units = 0;
    if (tid < E) {
        for (int w = 0; w < kAlignWaves; ++w) {
            const int c = cnt[w * E + tid];
            cnt[w * E + tid] = total;
            total += c;
        }
        units = (total + kUnitRows - 1) / kUnitRows;
    }
    int incl = units;
    for (int d = 1; d < 64; d <<= 1) {
        const int n = __shfl_up(incl, d);
        if (lane >= d) incl += n;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    int first = incl - units, all = 0;
    for (int w = 0; w < kAlignWaves; ++w) {
        if (w < wave) first += wsum[w];
        all += wsum[w];
    }
    if (tid < E) {
        start_row[tid] = first * kUnitRows;
        for (int u = 0; u < units; ++u) p.unit_expert[first + u] = tid;
        for (int r = first * kUnitRows + total; r < (first + units) * kUnitRows; ++r) p.sorted_slots[r] = -1;   // padding of the last unit
    }
    if (tid == 0) *p.num_units = all;
    for (int u = all + tid; u < p.max_units; u += blockDim.x) p.unit_expert[u] = -1;                            // tail
    for (int r = all * kUnitRows + tid; r < p.max_units * kUnitRows; r += blockDim.x) p.sorted_slots[r] = -1;
    __syncthreads();
    // pass 2: scatter, 64 slots of the wave's range per step in ascending order
    volatile int* off = cnt + wave * E;
    for (int base = s0; base < s1; base += 64) {     // wave-uniform trip count
        const int s = base + lane;
        const int e = s < s1 ? p.ids[s] : -1;
        const bool ok = e >= 0 && e < E;
        uint64_t same = __ballot(ok);
        for (int b = 0; b < 9; ++b) {                // E <= 512: nine id bits
            const uint64_t m = __ballot(ok && ((e >> b) & 1));
            same &= ((e >> b) & 1) ? m : ~m;
        }
        const int rank = __popcll(same & ((1ull << lane) - 1));
        int o = 0;
        if (ok) o = off[e];
        if (ok) p.sorted_slots[start_row[e] + o + rank] = s;
        if (ok && rank == 0) off[e] = o + __popcll(same);
    }
}

struct GroupedParams {
    const uint16_t* x;            // GATE_UP: [T, H]; DOWN: act [S, I]
    const uint32_t* qw;
    const uint32_t* meta;
    const int32_t* sorted_slots;
    const int32_t* unit_expert;
    const int32_t* num_units;
    void* out;                    // GATE_UP: act [S, I] 16-bit; DOWN: part [S, H] fp32
    size_t w_stride, m_stride;
    int S, row_div, E, K, N;      // row_div: slots per activation row (top_k for GATE_UP, 1 for DOWN)
    int chunks, cpg, G, max_units;
};

template <int ACT, int SCL, bool GATE_UP, int MAXW>
__global__ __launch_bounds__(64 * MAXW) void moe_grouped_kernel(GroupedParams p) {
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
    const uint32_t* wt = p.qw + (size_t)e * p.w_stride + (size_t)tile * p.chunks * 256;
    const uint32_t* mt = p.meta + (size_t)e * p.m_stride + (size_t)tile * p.G * 16;
    // lane (rq, m): A[m][32 j + 8 rq .. + 7] of K-step j
    const uint16_t* xl = p.x + (size_t)((slot < 0 ? slot0 : slot) / p.row_div) * p.K + 8 * rq;
    const DequantConsts kc = make_dequant_consts<4>();
    f4_t acc = {0.f, 0.f, 0.f, 0.f};
    for (int base = wave; base < p.chunks; base += W * kGroupedAhead) {
        u4_t w[kGroupedAhead], a[kGroupedAhead][4];
        uint32_t m[kGroupedAhead];
#pragma unroll
        for (int u = 0; u < kGroupedAhead; ++u) {
            const int ck = base + u * W < p.chunks ? base + u * W : base;   // past the end: a harmless repeat of an in-range chunk
            w[u] = __builtin_nontemporal_load(reinterpret_cast<const u4_t*>(wt + (size_t)ck * 256 + lane * 4));
            m[u] = mt[(ck / p.cpg) * 16 + c16];
#pragma unroll
            for (int j = 0; j < 4; ++j) a[u][j] = *reinterpret_cast<const u4_t*>(xl + (size_t)ck * kChunkK + 32 * j);
        }
#pragma unroll
        for (int u = 0; u < kGroupedAhead; ++u) {
            if (base + u * W < p.chunks) {   // wave-uniform
                const ColConst cc = expand_meta<4, SCL>(m[u]);
#pragma unroll
                for (int j = 0; j < 4; ++j) acc = mfma16<ACT>(a[u][j], dequant_word4<ACT, SCL>(w[u][j], cc, kc), acc);
            }
        }
    }
    // accumulator register i of lane (rq, n) = row 4 rq + i, column n
#pragma unroll
    for (int i = 0; i < 4; ++i) red[wave][4 * rq + i][c16] = acc[i];
    __syncthreads();
    for (int t = threadIdx.x; t < kUnitRows * 16; t += blockDim.x) {   // (t and t + 8 sit in one wave in the same trip: the shuffle below is safe)
        const int mrow = t >> 4, n = t & 15;
        float v = 0.f;
        for (int ww = 0; ww < W; ++ww) v += red[ww][mrow][n];
        const int s = slots[mrow];
        if constexpr (GATE_UP) {
            const uint16_t r = moe_silu_up<ACT>(v);   // columns 0 .. 7 are gate columns, 8 .. 15 the matching up columns
            if (n < 8 && s >= 0) reinterpret_cast<uint16_t*>(p.out)[(size_t)s * (p.N >> 1) + tile * 8 + n] = r;
        } else {
            if (s >= 0) reinterpret_cast<float*>(p.out)[(size_t)s * p.N + tile * 16 + n] = v;
        }
    }
}

struct CombineParams {
    const float* part;
    const int32_t* ids;
    const float* weights;
    uint16_t* out;
    int32_t* status;
    int top_k, E, H;
};

template <int ACT>
__global__ __launch_bounds__(256) void moe_combine_kernel(CombineParams p) {
    const int t = blockIdx.x;
    const int col = (blockIdx.y * 256 + threadIdx.x) * 4;
    if (col >= p.H) return;
    f4_t y = {0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < p.top_k; ++j) {   // slot order; an out-of-range expert contributes nothing, whatever its routing weight
        const int s = t * p.top_k + j;
        const int e = p.ids[s];
        if (e < 0 || e >= p.E) {
            if (col == 0) *p.status = 1;
            continue;
        }
        const float wj = p.weights[s];
        const f4_t d = *reinterpret_cast<const f4_t*>(p.part + (size_t)s * p.H + col);
        y[0] += wj * d[0];
        y[1] += wj * d[1];
        y[2] += wj * d[2];
        y[3] += wj * d[3];
    }
    u2_t o;
    if constexpr (ACT == kFP16) {
        o.x = pack_f16(y[0], y[1]);
        o.y = pack_f16(y[2], y[3]);
    } else {
        o.x = pack_bf16(y[0], y[1]);
        o.y = pack_bf16(y[2], y[3]);
    }
    *reinterpret_cast<u2_t*>(p.out + (size_t)t * p.H + col) = o;
}

template <bool GATE_UP, int MAXW>
static void grouped_launch(int act_dtype, int scale_dtype, const GroupedParams& p, dim3 grid, dim3 block, hipStream_t stream) {
    moe_dispatch(act_dtype, scale_dtype, [&](auto a, auto s) {
        hipLaunchKernelGGL((moe_grouped_kernel<decltype(a)::value, decltype(s)::value, GATE_UP, MAXW>), grid, block, 0, stream, p);
    });
}

static GroupedParams grouped_params(const void* x, const uint32_t* qw, const uint32_t* meta, const int32_t* sorted_slots, const int32_t* unit_expert,
                                    const int32_t* num_units, void* out, int S, int row_div, int E, int K, int N, int group_size) {
    GroupedParams p;
    p.x = reinterpret_cast<const uint16_t*>(x);
    p.qw = qw;
    p.meta = meta;
    p.sorted_slots = sorted_slots;
    p.unit_expert = unit_expert;
    p.num_units = num_units;
    p.out = out;
    p.w_stride = gptqhip_tiled_words(K, N, 4);
    p.m_stride = gptqhip_meta_words(K, N, group_size);
    p.S = S;
    p.row_div = row_div;
    p.E = E;
    p.K = K;
    p.N = N;
    p.chunks = K / kChunkK;
    p.cpg = group_size / kChunkK;
    p.G = K / group_size;
    p.max_units = grouped_units(S, E);
    return p;
}

}  // namespace gptqhip

using namespace gptqhip;

extern "C" {

int gptqhip_moe_grouped_supported(int H, int I, int group_size, int bits, int has_perm, int T, int top_k, int E) {
    if (has_perm) return 0;
    // group_size <= 0: one group for the whole K of each projection (group_size = -1 checkpoints)
    return moe_int4_shape_ok(H, I, H, group_size <= 0 ? H : group_size, bits) && moe_int4_shape_ok(H, I, I, group_size <= 0 ? I : group_size, bits) &&
                   grouped_routing_ok(T, top_k, E)
               ? 1
               : 0;
}

int gptqhip_moe_grouped_units(int S, int E) {
    if (S < 1 || E < 1) return 0;
    return grouped_units(S, E);
}

int gptqhip_moe_align(const int32_t* ids, int32_t* sorted_slots, int32_t* unit_expert, int32_t* num_units, int32_t* status, int T, int top_k, int E,
                      gptqhip_stream_t stream) {
    const void* p4[] = {ids, sorted_slots, unit_expert, num_units, status};
    int rc = grouped_check_ptrs("gptqhip_moe_align", nullptr, 0, p4, 5);
    if (!rc) rc = grouped_check_routing("gptqhip_moe_align", T, top_k, E);
    if (rc) return rc;
    AlignParams p;
    p.ids = ids;
    p.sorted_slots = sorted_slots;
    p.unit_expert = unit_expert;
    p.num_units = num_units;
    p.status = status;
    p.S = T * top_k;
    p.E = E;
    p.max_units = grouped_units(p.S, E);
    hipLaunchKernelGGL(moe_align_kernel, dim3(1), dim3(64 * kAlignWaves), sizeof(int) * kAlignWaves * E, reinterpret_cast<hipStream_t>(stream), p);
    return check_hip(hipGetLastError(), "moe_align_kernel launch");
}

int gptqhip_moe_gate_up_grouped(const void* x, const uint32_t* qweight_t, const uint32_t* meta, const int32_t* sorted_slots,
                                const int32_t* unit_expert, const int32_t* num_units, void* act, int T, int top_k, int E, int H, int I,
                                int group_size, int bits, int act_dtype, int scale_dtype, gptqhip_stream_t stream) {
    const char* fn = "gptqhip_moe_gate_up_grouped";
    const void* p16[] = {x, qweight_t, meta, act};
    const void* p4[] = {sorted_slots, unit_expert, num_units};
    int rc = grouped_check_ptrs(fn, p16, 4, p4, 3);
    if (!rc) rc = grouped_check_routing(fn, T, top_k, E);
    if (!rc) rc = moe_check_int4_shape(fn, H, I, H, group_size, bits);
    if (!rc) rc = moe_check_dtypes(fn, act_dtype, scale_dtype);
    if (rc) return rc;
    const GroupedParams p = grouped_params(x, qweight_t, meta, sorted_slots, unit_expert, num_units, act, T * top_k, top_k, E, H, 2 * I, group_size);
    const int waves = p.chunks < kGroupedGateUpWaves ? p.chunks : kGroupedGateUpWaves;
    grouped_launch<true, kGroupedGateUpWaves>(act_dtype, scale_dtype, p, dim3(2 * I / kTileN, p.max_units), dim3(64 * waves),
                                              reinterpret_cast<hipStream_t>(stream));
    return check_hip(hipGetLastError(), "moe_grouped_kernel (gate_up) launch");
}

int gptqhip_moe_down_grouped(const void* act, const uint32_t* qweight_t, const uint32_t* meta, const int32_t* sorted_slots,
                             const int32_t* unit_expert, const int32_t* num_units, float* part, int T, int top_k, int E, int H, int I,
                             int group_size, int bits, int act_dtype, int scale_dtype, gptqhip_stream_t stream) {
    const char* fn = "gptqhip_moe_down_grouped";
    const void* p16[] = {act, qweight_t, meta, part};
    const void* p4[] = {sorted_slots, unit_expert, num_units};
    int rc = grouped_check_ptrs(fn, p16, 4, p4, 3);
    if (!rc) rc = grouped_check_routing(fn, T, top_k, E);
    if (!rc) rc = moe_check_int4_shape(fn, H, I, I, group_size, bits);
    if (!rc) rc = moe_check_dtypes(fn, act_dtype, scale_dtype);
    if (rc) return rc;
    const GroupedParams p = grouped_params(act, qweight_t, meta, sorted_slots, unit_expert, num_units, part, T * top_k, 1, E, I, H, group_size);
    const int waves = p.chunks < kGroupedDownWaves ? p.chunks : kGroupedDownWaves;
    grouped_launch<false, kGroupedDownWaves>(act_dtype, scale_dtype, p, dim3(H / kTileN, p.max_units), dim3(64 * waves),
                                             reinterpret_cast<hipStream_t>(stream));
    return check_hip(hipGetLastError(), "moe_grouped_kernel (down) launch");
}

int gptqhip_moe_combine(const float* part, const int32_t* ids, const float* weights, void* out, int32_t* status, int T, int top_k, int E, int H,
                        int act_dtype, gptqhip_stream_t stream) {
    const char* fn = "gptqhip_moe_combine";
    const void* p16[] = {part, out};
    const void* p4[] = {ids, weights, status};
    int rc = grouped_check_ptrs(fn, p16, 2, p4, 3);
    if (!rc) rc = grouped_check_routing(fn, T, top_k, E);
    if (rc) return rc;
    if (H <= 0 || H % 128 != 0) {
        set_error("%s: H=%d must be a positive multiple of 128", fn, H);
        return GPTQHIP_EINVAL;
    }
    if (act_dtype != GPTQHIP_FP16 && act_dtype != GPTQHIP_BF16) {
        set_error("%s: unsupported output dtype %d", fn, act_dtype);
        return GPTQHIP_EINVAL;
    }
    CombineParams p;
    p.part = part;
    p.ids = ids;
    p.weights = weights;
    p.out = reinterpret_cast<uint16_t*>(out);
    p.status = status;
    p.top_k = top_k;
    p.E = E;
    p.H = H;
    const dim3 grid(T, (H / 4 + 255) / 256);
    if (act_dtype == GPTQHIP_FP16) hipLaunchKernelGGL(moe_combine_kernel<kFP16>, grid, dim3(256), 0, reinterpret_cast<hipStream_t>(stream), p);
    else hipLaunchKernelGGL(moe_combine_kernel<kBF16>, grid, dim3(256), 0, reinterpret_cast<hipStream_t>(stream), p);
    return check_hip(hipGetLastError(), "moe_combine_kernel launch");
}

}  // extern "C"
