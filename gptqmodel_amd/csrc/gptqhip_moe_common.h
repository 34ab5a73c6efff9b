// What the device-routed MoE translation units share (gptqhip_moe.hip, gptqhip_moe_fp8.hip, gptqhip_moe_grouped.hip, gptqhip_moe_fp8_grouped.hip):
// the constants of the few-token kernels, the limits and unit size of the expert-grouped path, the masked-K-step fragments, and the two NUMERICS
// CONTRACTS of the experts path, each stated and written ONCE here:
//
//   SiLU * up   (moe_silu_up)         y = act(v) for the gate and the up column, s = act(silu(y_gate)) with the accurate expf, a = act(s * y_up):
//                                     the rounding chain of GPTQHIP_OUT_SILU_MUL_PAIRED = HF's act_fn(gate) * up in the activation dtype.
//   combine     (moe_combine_slots)   out[t, n] = act( sum_{j = 0 .. top_k - 1} weights[t, j] * scale_j * ( sum_{s = 0 .. wps - 1} partial[j, s][n] ) ):
//                                     fp32 dot products, ONE fp32 weighted sum in slot order, ONE rounding; an expert id outside [0, E) contributes
//                                     nothing whatever its routing weight and sets the device status word (the convention of gptqhip_embedding).  No
//                                     floating-point atomics: two runs give the same bits.  Deliberately NOT the chain of the HF experts loop (which
//                                     rounds every expert's output and every product and accumulates in the activation dtype through index_add_); it
//                                     is the choice the tensor-parallel path made.  moe_combine_kernel (grouped path) restates it on 4-wide vectors.
//
// NOT shared, on purpose: the inner loops.  The int4 few-token loop deals chunks to waves strided (w, w + W, ..), the FP8 loop deals contiguous
// ranges and flushes at K-block boundaries, the grouped loops (int4 strided, FP8 contiguous) carry 16 real rows: each fixes a summation order and
// with it the output bits.
//
// Host side: the argument checks every entry point runs, in the order they are listed here; the entry point's name leads every message.
#pragma once
#include <type_traits>

#include "../../include/gptqhip.h"
#include "gptqhip_device.h"
#include "gptqhip_host.h"

namespace gptqhip {

constexpr int kMoeMaxRows = 16;      // few-token ops: tokens per call, and slots per token
constexpr int kMoeGateUpWaves = 8;   // most waves of a gate_up block (in-block split-K)
constexpr int kMoeDownWaves = 16;    // most waves of a down block
constexpr int kMoeAhead = 4;         // chunks whose loads a wave issues before consuming the first

// expert-grouped path (gptqhip_moe_grouped.hip: align, int4 stages, combine; gptqhip_moe_fp8_grouped.hip: FP8 stages)
constexpr int kGroupedMaxExperts = 512;    // cnt[16][E] ints of LDS: 32 KiB at E = 512
constexpr int kGroupedMaxSlots = 65536;    // max_units <= 4576 blocks in grid.y
constexpr int kGroupedMaxTopK = 16;
constexpr int kUnitRows = 16;

__host__ __device__ inline int grouped_units(int S, int E) {
    const int ne = S < E ? S : E;
    const int u = (S + 15 * ne) / 16;
    return u < S ? u : S;
}

// ---- device ----------------------------------------------------------------------------------------------------------------------------------
// Masked K-steps: lane (rq, c) loads the 8 activations of K-step c & 3 (rows 8 rq .. 8 rq + 7 of it), so MFMA row m carries K-step m & 3.  K-step j
// runs with the A rows of the other K-steps masked to zero; accumulator row m ends up with K-step m & 3's share and rows 0 .. 3 add up to the chunk's
// dot product: one activation load per chunk instead of four broadcast ones.
__device__ __forceinline__ void moe_kstep_masks(int c16, uint32_t (&mask)[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) mask[j] = (c16 & 3) == j ? 0xffffffffu : 0u;
}

__device__ __forceinline__ u4_t moe_masked_a(const u4_t& a, uint32_t m) {
    u4_t r;
    r.x = a.x & m;
    r.y = a.y & m;
    r.z = a.z & m;
    r.w = a.w & m;
    return r;
}

// accumulator register i of lanes 0 .. 15 = row i = K-step i's share: lanes 0 .. 15 return the column sums, the rest 0
__device__ __forceinline__ float moe_lane_sum(const f4_t& s, int rq) { return rq == 0 ? (s[0] + s[1]) + (s[2] + s[3]) : 0.f; }

// gate_up, expert id outside [0, E) (block-uniform): nothing is dereferenced through it, the slot's 8 outputs of this tile are zero, status is set.
// True: the block is done.
__device__ __forceinline__ bool moe_gate_up_invalid(int e, int E, uint16_t* out8, int32_t* status) {
    if (e >= 0 && e < E) return false;
    if (threadIdx.x < 8) out8[threadIdx.x] = 0;
    if (threadIdx.x == 0) *status = 1;
    return true;
}

// The SiLU * up chain on a fused gate|up tile whose columns 0 .. 7 are gate columns and 8 .. 15 the matching up columns: every lane passes its
// column's fp32 sum, the lane of gate column n (whose lane + 8 holds up column n, in the same wave) gets the 16-bit result; the rest get garbage.
template <int ACT>
__device__ __forceinline__ uint16_t moe_silu_up(float v) {
    const float y = round_through<ACT>(v);
    const float up = __shfl_down(y, 8);
    const float a = round_through<ACT>(y / (1.0f + expf(-y))) * up;   // expf, not __expf: HF evaluates SiLU with the accurate exp
    return f32_to_16<ACT>(a);
}

// The combine of a few-token down block (contract above): wave 0, lanes 0 .. 15 = columns out16[0 .. 15]; red[j * wps + s] holds slot j's s-th
// partial row.  ids / weights: the token's top_k entries.  scale(d, e): the per-slot factor of the reduced dot product (identity; FP8 tensor / row
// reciprocal scale of expert e).
template <int ACT, class Scale>
__device__ __forceinline__ void moe_combine_slots(const float (*red)[16], int wave, int lane, const int32_t* ids, const float* weights, int top_k,
                                                  int E, int wps, uint16_t* out16, Scale scale) {
    if (wave != 0 || lane >= 16) return;
    float y = 0.f;
    for (int jj = 0; jj < top_k; ++jj) {   // slot order; an out-of-range expert contributes nothing, whatever its routing weight
        const int ej = ids[jj];
        if (ej < 0 || ej >= E) continue;
        float d = 0.f;
        for (int s = 0; s < wps; ++s) d += red[jj * wps + s][lane];
        y += weights[jj] * scale(d, ej);
    }
    out16[lane] = f32_to_16<ACT>(y);
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------------
// null, then the 16-byte list, then the 4-byte list; what16 / what4 name the lists in the message
inline int moe_check_ptrs(const char* fn, const void* const* ptrs16, int n16, const char* what16, const void* const* ptrs4, int n4, const char* what4) {
    for (int i = 0; i < n16 + n4; ++i) {
        if ((i < n16 ? ptrs16[i] : ptrs4[i - n16]) == nullptr) {
            set_error("%s: null tensor pointer", fn);
            return GPTQHIP_EINVAL;
        }
    }
    for (int i = 0; i < n16; ++i) {
        if (reinterpret_cast<uintptr_t>(ptrs16[i]) % 16 != 0) {
            set_error("%s: %s must be 16-byte aligned", fn, what16);
            return GPTQHIP_EINVAL;
        }
    }
    for (int i = 0; i < n4; ++i) {
        if (reinterpret_cast<uintptr_t>(ptrs4[i]) % 4 != 0) {
            set_error("%s: %s must be 4-byte aligned", fn, what4);
            return GPTQHIP_EINVAL;
        }
    }
    return GPTQHIP_OK;
}

inline bool moe_few_tokens_ok(int T, int top_k) { return T >= 1 && T <= kMoeMaxRows && top_k >= 1 && top_k <= kMoeMaxRows; }

inline int moe_check_few_tokens(const char* fn, int T, int top_k, int E) {
    if (!moe_few_tokens_ok(T, top_k)) {
        set_error("%s: T=%d and top_k=%d must be 1..%d", fn, T, top_k, kMoeMaxRows);
        return GPTQHIP_EINVAL;
    }
    if (E < 1) {
        set_error("%s: E=%d experts", fn, E);
        return GPTQHIP_EINVAL;
    }
    return GPTQHIP_OK;
}

inline bool moe_group_ok(int K, int group_size) {   // 128 * 2^n dividing K (one group for the whole K included)
    if (group_size < 128 || K % group_size != 0) return false;
    const int q = group_size / 128;
    return group_size % 128 == 0 && (q & (q - 1)) == 0;
}

// one int4 projection with K input rows of experts H x I
inline bool moe_int4_shape_ok(int H, int I, int K, int group_size, int bits) {
    return bits == 4 && H > 0 && I > 0 && H % 128 == 0 && I % 128 == 0 && moe_group_ok(K, group_size);
}

inline int moe_check_int4_shape(const char* fn, int H, int I, int K, int group_size, int bits) {
    if (!moe_int4_shape_ok(H, I, K, group_size, bits)) {
        set_error("%s: unsupported shape H=%d I=%d group_size=%d bits=%d (4 bits, H and I multiples of 128, group_size = 128 * 2^n dividing K=%d)",
                  fn, H, I, group_size, bits, K);
        return GPTQHIP_EINVAL;
    }
    return GPTQHIP_OK;
}

inline int moe_check_dtypes(const char* fn, int act_dtype, int scale_dtype) {
    if ((act_dtype != GPTQHIP_FP16 && act_dtype != GPTQHIP_BF16) || (scale_dtype != GPTQHIP_FP16 && scale_dtype != GPTQHIP_BF16) ||
        (act_dtype == GPTQHIP_BF16 && scale_dtype == GPTQHIP_FP16)) {
        set_error("%s: unsupported dtypes act=%d scales=%d (fp16 x fp16, bf16 x bf16, fp16 activations x bf16 scales)", fn, act_dtype, scale_dtype);
        return GPTQHIP_EINVAL;
    }
    return GPTQHIP_OK;
}

// launch(act, scl): called with the two dtype tags of a pair moe_check_dtypes passed, as std::integral_constant (decltype(act)::value is the ACT
// template argument of the kernel to launch)
template <class Launch>
inline void moe_dispatch(int act_dtype, int scale_dtype, Launch&& launch) {
    using fp16 = std::integral_constant<int, kFP16>;
    using bf16 = std::integral_constant<int, kBF16>;
    if (act_dtype == GPTQHIP_FP16 && scale_dtype == GPTQHIP_FP16) launch(fp16{}, fp16{});
    else if (act_dtype == GPTQHIP_BF16) launch(bf16{}, bf16{});
    else launch(fp16{}, bf16{});
}

// ---- expert-grouped path: routing limits and pointer lists ------------------------------------------------------------------------------------
inline bool grouped_routing_ok(int T, int top_k, int E) {
    return T >= 1 && top_k >= 1 && top_k <= kGroupedMaxTopK && E >= 1 && E <= kGroupedMaxExperts && (long long)T * top_k <= kGroupedMaxSlots;
}

inline int grouped_check_ptrs(const char* fn, const void* const* ptrs16, int n16, const void* const* ptrs4, int n4) {
    return moe_check_ptrs(fn, ptrs16, n16, "activations, weights, constants, partial sums and outputs", ptrs4, n4,
                          "ids, weights, sort buffers and status");
}

inline int grouped_check_routing(const char* fn, int T, int top_k, int E) {
    if (!grouped_routing_ok(T, top_k, E)) {
        set_error("%s: T=%d top_k=%d E=%d outside T >= 1, 1 <= top_k <= %d, 1 <= E <= %d, T * top_k <= %d", fn, T, top_k, E, kGroupedMaxTopK,
                  kGroupedMaxExperts, kGroupedMaxSlots);
        return GPTQHIP_EINVAL;
    }
    return GPTQHIP_OK;
}

// ---- FP8 experts: shapes and scale layouts (few-token and grouped ops) ------------------------------------------------------------------------
// the scale layout of one stacked projection [N, K]: nullptr when served
inline const char* moe_fp8_scale_error(int K, int N, int mode, int br, int bc) {
    if (mode == GPTQHIP_FP8_SCALE_TENSOR || mode == GPTQHIP_FP8_SCALE_ROW) return nullptr;
    if (mode != GPTQHIP_FP8_SCALE_BLOCK) return "scale layout must be tensor (0), row (1) or block (2)";
    if (bc <= 0 || bc % kChunkK != 0 || K % bc != 0) return "block columns must be a multiple of 128 dividing in_features";
    if (br <= 0 || N % br != 0) return "block rows must divide out_features";
    return nullptr;
}

// experts H x I with these scale layouts and activations, whatever the number of tokens
inline bool moe_fp8_layouts_ok(int H, int I, int gate_up_block_cols, int down_scale_mode, int down_block_rows, int down_block_cols, int act_dtype) {
    if (act_dtype != GPTQHIP_FP16 && act_dtype != GPTQHIP_BF16) return false;
    if (!(H > 0 && I > 0 && H % 128 == 0 && I % 128 == 0)) return false;
    if (gate_up_block_cols != 0 && moe_fp8_scale_error(H, 2 * I, GPTQHIP_FP8_SCALE_BLOCK, 1, gate_up_block_cols) != nullptr) return false;
    return moe_fp8_scale_error(I, H, down_scale_mode, down_block_rows, down_block_cols) == nullptr;
}

// K, N, mode, br, bc: the projection the call runs
inline int moe_check_fp8_shape(const char* fn, int H, int I, int K, int N, int mode, int br, int bc, int act_dtype) {
    if (H <= 0 || I <= 0 || H % 128 != 0 || I % 128 != 0) {
        set_error("%s: unsupported shape H=%d I=%d (H and I positive multiples of 128)", fn, H, I);
        return GPTQHIP_EINVAL;
    }
    if (const char* why = moe_fp8_scale_error(K, N, mode, br, bc)) {
        set_error("%s: %s (in_features=%d out_features=%d scale layout %d block %d x %d)", fn, why, K, N, mode, br, bc);
        return GPTQHIP_EINVAL;
    }
    if (act_dtype != GPTQHIP_FP16 && act_dtype != GPTQHIP_BF16) {
        set_error("%s: unsupported activation dtype tag %d (fp16 = 0, bf16 = 1)", fn, act_dtype);
        return GPTQHIP_EINVAL;
    }
    return GPTQHIP_OK;
}

}  // namespace gptqhip
