// FP8 (float8_e4m3fn) codes -> MFMA B fragments: shared by gptqhip_fp8.hip and gptqhip_moe_fp8.hip.  The conversion routes are described in
// gptqhip_fp8.hip (CONVERSION ROUTES).
#pragma once
#include "gptqhip_device.h"

namespace gptqhip {

constexpr int kFp8BlockBytes = 2048;   // one (tile, chunk) block of the FP8 kernel layout
constexpr int kCvtPacked = 0, kCvtF32 = 1, kCvtBits = 2;

// lane (rq, c)'s 8 consecutive codes of one K-step -> MFMA B fragment (8 x 16-bit, natural k order)
template <int ACT, int CVT>
__device__ __forceinline__ u4_t fp8x8_to_frag(uint32_t lo, uint32_t hi) {
    u4_t r;
    if constexpr (CVT == kCvtPacked && ACT == kFP16) {
        r.x = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(lo, 1.0f, false));
        r.y = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(lo, 1.0f, true));
        r.z = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(hi, 1.0f, false));
        r.w = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(hi, 1.0f, true));
    } else if constexpr (CVT == kCvtPacked) {
        r.x = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, 1.0f, false));
        r.y = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, 1.0f, true));
        r.z = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, 1.0f, false));
        r.w = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, 1.0f, true));
    } else if constexpr (CVT == kCvtF32) {
        auto pair = [](uint32_t w, bool upper) {
            const auto f = upper ? __builtin_amdgcn_cvt_pk_f32_fp8(w, true) : __builtin_amdgcn_cvt_pk_f32_fp8(w, false);
            return ACT == kFP16 ? pack_f16(f[0], f[1]) : pack_bf16(f[0], f[1]);   // exact: 4 significant bits
        };
        r.x = pair(lo, false);
        r.y = pair(lo, true);
        r.z = pair(hi, false);
        r.w = pair(hi, true);
    } else {
        static_assert(ACT == kFP16, "the bit-placement route exists for fp16 only");
        // bytes (b0, b1) -> the upper bytes of the two halves, then sign stays and exponent | mantissa move down by one: value * 2^-8
        auto pair = [](uint32_t w, uint32_t sel) {
            const uint32_t t = __builtin_amdgcn_perm(w, w, sel);
            return ((t >> 1) & 0x3f803f80u) | (t & 0x80008000u);
        };
        r.x = pair(lo, 0x010c000cu);
        r.y = pair(lo, 0x030c020cu);
        r.z = pair(hi, 0x010c000cu);
        r.w = pair(hi, 0x030c020cu);
    }
    return r;
}

}  // namespace gptqhip
