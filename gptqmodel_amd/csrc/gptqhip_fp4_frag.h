// NVFP4 (e2m1 codes, one float8_e4m3fn scale per 16 input features) -> MFMA B fragments with the block scale applied.  The conversion routes are
// described in gptqhip_fp4.hip (CONVERSION ROUTES); kept apart from the kernels so that a later stacked-expert form can share them.
#pragma once
#include "gptqhip_device.h"

namespace gptqhip {

constexpr int kFp4BlockBytes = 1024;       // codes of one (tile, chunk) block of the FP4 kernel layout
constexpr int kFp4ScaleBlockBytes = 128;   // its block scales
constexpr int kFp4CvtPacked = 0, kFp4CvtF32 = 1;

typedef float f2_t __attribute__((ext_vector_type(2)));

// The four block scales of a lane (one e4m3 byte per K-step, gptqhip_fp4.hip KERNEL LAYOUT), converted once per chunk: exactly.
template <int ACT, int CVT>
struct Fp4Scales {
    h2_t h01, h23;   // packed route, fp16: (s0, s1), (s2, s3)
    float f[4];      // fp32 routes
};

template <int ACT, int CVT>
__device__ __forceinline__ Fp4Scales<ACT, CVT> fp4_scales(uint32_t sw) {
    Fp4Scales<ACT, CVT> s;
    if constexpr (CVT == kFp4CvtPacked && ACT == kFP16) {
        s.h01 = __builtin_bit_cast(h2_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(sw, 1.0f, false));   // e4m3 -> fp16 is exact, subnormals included
        s.h23 = __builtin_bit_cast(h2_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(sw, 1.0f, true));
    } else {
        s.f[0] = __builtin_amdgcn_cvt_f32_fp8((int)sw, 0);
        s.f[1] = __builtin_amdgcn_cvt_f32_fp8((int)sw, 1);
        s.f[2] = __builtin_amdgcn_cvt_f32_fp8((int)sw, 2);
        s.f[3] = __builtin_amdgcn_cvt_f32_fp8((int)sw, 3);
    }
    return s;
}

// two codes (byte SEL of w: the low nibble is the even feature) times the scale, in fp32: exact (<= 6 significant bits)
template <int SEL>
__device__ __forceinline__ f2_t fp4_pair_f32(uint32_t w, float scale) {
    return __builtin_bit_cast(f2_t, __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, 1.0f, SEL)) * scale;
}

// lane (rq, c)'s 8 consecutive codes of K-step J (one dword, nibble e = row 8 rq + e) -> MFMA B fragment (8 x 16-bit, natural k order)
template <int ACT, int CVT, int J>
__device__ __forceinline__ u4_t fp4x8_to_frag(uint32_t w, const Fp4Scales<ACT, CVT>& s) {
    u4_t r;
    if constexpr (CVT == kFp4CvtPacked && ACT == kFP16) {
        const h2_t pair = J < 2 ? s.h01 : s.h23;
        const _Float16 sj = (J & 1) ? pair.y : pair.x;
        const h2_t sc = {sj, sj};
        r.x = as_u32(__builtin_bit_cast(h2_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, 1.0f, 0)) * sc);   // exact products: one v_pk_mul_f16 per two weights
        r.y = as_u32(__builtin_bit_cast(h2_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, 1.0f, 1)) * sc);
        r.z = as_u32(__builtin_bit_cast(h2_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, 1.0f, 2)) * sc);
        r.w = as_u32(__builtin_bit_cast(h2_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, 1.0f, 3)) * sc);
    } else if constexpr (CVT == kFp4CvtPacked) {
        // bf16: the hardware converts to bf16, but gfx950 has no packed bf16 multiply: widen (a shift / a mask), multiply in fp32, narrow
        auto pair = [](uint32_t b, float scale) { return pack_bf16(bf16lo_to_f32(b) * scale, bf16hi_to_f32(b) * scale); };
        const float sj = s.f[J];
        r.x = pair(__builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, 1.0f, 0)), sj);
        r.y = pair(__builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, 1.0f, 1)), sj);
        r.z = pair(__builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, 1.0f, 2)), sj);
        r.w = pair(__builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, 1.0f, 3)), sj);
    } else {
        auto narrow = [](f2_t v) { return ACT == kFP16 ? pack_f16(v.x, v.y) : pack_bf16(v.x, v.y); };   // exact: <= 6 significant bits
        const float sj = s.f[J];
        r.x = narrow(fp4_pair_f32<0>(w, sj));
        r.y = narrow(fp4_pair_f32<1>(w, sj));
        r.z = narrow(fp4_pair_f32<2>(w, sj));
        r.w = narrow(fp4_pair_f32<3>(w, sj));
    }
    return r;
}

}  // namespace gptqhip
