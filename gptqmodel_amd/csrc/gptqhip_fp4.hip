// NVFP4 weight-only linear, W4A16 (include/gptqhip.h: gptqhip_fp4_supported / gptqhip_fp4_tiled_bytes / gptqhip_fp4_scale_bytes / gptqhip_fp4_repack /
// gptqhip_fp4_gemm / gptqhip_fp4_dequant).  Serves the checkpoints the reference rebuilds as TorchFP4Linear (gptqmodel/nn_modules/qlinear/fp4.py:19,
// models/base.py:2099-2142), whose forward needs torchao's NVFP4Tensor and hardware that advertises native NVFP4: on ROCm it has none.
//
// SEMANTICS.  W[n, k] = code[n, k] * weight_scale[n, k / 16] * weight_scale_2:
//   code          e2m1, two per byte, `s e1 e0 m` = +-{0, 0.5, 1, 1.5, 2, 3, 4, 6} (gptqmodel_ext/floatx_cpu.cpp:153-156); feature 2 b is the LOW nibble of
//                 byte b, 2 b + 1 the high nibble (floatx_cpu.cpp:1998-2003)
//   weight_scale  float8_e4m3fn [N, K / 16], plain row-major (torchao's swizzled layout is declined)
//   weight_scale_2  ONE fp32 scalar behind a device pointer (ModelOpt's global scale, base.py:2113-2115); a null pointer means 1.0
// Every product code * weight_scale is EXACT in fp16 and in bf16 (16 codes x 254 finite e4m3 bytes: magnitudes 2^-10 .. 2688, at most 6
// significant bits; tests/test_fp4_cpu.py), so block-scaled weights enter the f16 / bf16 matrix pipe exactly and NO per-block accumulator flush is
// needed.  Sums are fp32; weight_scale_2 and the bias touch the fp32 accumulator once, in the epilogue; then ONE rounding:
//     y[m, n] = round_act( s2 * sum_k x[m, k] * (code[n, k] * s_blk[n, k / 16]) + bias[n] ).
// This is deliberately NOT the reference's chain (quantization/dtype.py:303-340: table value cast to the activation dtype, the effective scale
// fp32(weight_scale) * scale_2 cast to it, the product rounded, then the matmul's and the bias add's roundings): it is the choice decode form 5
// and gptqhip_fp8_gemm made, held to the same bar (tests/test_gpu_fp4.py).
//
// NaN SCALE BYTES (0x7f, 0xff): UNDEFINED.  Every other scale byte is defined: +-0, subnormals, negative values.  The sign of a zero output is not
// part of the contract.
//
// SUPPORTED SET (gptqhip_fp4_supported, the one host predicate; everything else is GPTQHIP_EINVAL before any device access):
//   block_size 16; activations fp16 | bf16; K % 128 == 0, N % 16 == 0; 0 <= M <= 65535 * 64.
//
// KERNEL LAYOUT (gptqhip_fp4_repack, once in post_init), tile = n / 16, chunk = k / 128, lane = (rq << 4) | c:
//   codes   byte[((tile * chunks + chunk) * 64 + lane) * 16 + 4 j + (e >> 1)], nibble e & 1 (low first), holds column n = 16 tile + c, row
//           k = 128 chunk + 32 j + 8 rq + e: dword j of the lane's 16 bytes is its B fragment of K-step j of mfma_f32_16x16x32, nibble e = row e, in
//           natural k order -- the checkpoint's own byte order, so the relayout moves whole dwords.  All eight rows lie in ONE 16-wide scale block,
//           2 j + (rq >> 1) of the chunk's eight.  A (tile, chunk) block is 1 KiB contiguous = ONE 16 B-per-lane wave load.
//   scales  byte[((tile * chunks + chunk) * 32 + 16 (rq >> 1) + c) * 4 + j] = weight_scale[16 tile + c, 8 chunk + 2 j + (rq >> 1)]: a lane reads the
//           four scales of its four K-steps as ONE dword (lanes rq and rq ^ 1 read the same dword); 128 B per (tile, chunk) block.
//   The chunks of a tile follow each other in both arrays: a wave streams two linear address ranges, one weight load and one scale load per chunk.
//
// (a) fp4_decode_kernel, 1 <= M <= 16: grid = N / 16 column tiles (N / 64 on wide layers, below), min(8, chunks) waves per block; wave w takes the CONTIGUOUS chunk range
//     [w * chunks / W, (w + 1) * chunks / W) -- a rule of the shape alone -- with the loads of up to four chunks issued before the first is consumed
//     (weights non-temporal), all M rows in one MFMA tile (rows >= M are zero, never loaded).  Partial accumulators go through LDS and wave 0 adds
//     them in wave order: no floating-point atomics, so two runs give the same bits; MFMA rows never mix and the split does not depend on M, so a
//     row's bits do not depend on which other rows are in the batch.  One launch whose grid depends on (K, N) only: capturable in a graph.
//     At 4 bits a chunk is only 1 KiB against 4 KiB of activation fragments (64 of the lane's registers for four chunks, whatever M is), so the
//     registers, not the bytes, bound what a wave keeps in flight.  Layers of >= 1024 column tiles (two resident blocks per CU even so) therefore
//     give a block FOUR tiles that share the wave's activation fragments, with two chunks in flight: 8 KiB of weights per wave instead of 4, a
//     quarter of the activation traffic per weight (4096 x 28672, 16 rows: 31.7 -> 20.6 us).  The variant is a rule of (K, N) alone, and a
//     tile's partial sums are formed by the same wave over the same chunks in the same order in both, so the bits do not depend on it
//     (tests/test_gpu_fp4.py compares them).  Eight chunks in flight on narrow, deep layers (208 VGPRs, two waves per SIMD) measured no faster
//     (14336 x 4096, one row: 12.5 vs 11.9 us), sixteen waves per block there lost on 4096 x 4096 (6.5 vs 5.1 us): neither is built.
// (b) fp4_gemm_kernel, M >= 17: 4 waves per block, a block covers 64 rows x 128 columns (a wave: 4 row tiles x 2 column tiles), A fragments read
//     straight from global memory, B fragments converted in registers from the same layout; no workspace.  Correctness first.
// (c) fp4_dequant_kernel: [K, N] in fp16 | bf16 | fp32, each element round(fp32(code * s_blk) * s2), once.
// (d) fp4_repack_kernel / fp4_repack_scale_kernel: checkpoint layout -> kernel layout, one thread per 16 B of codes / per dword of scales.
//
// CONVERSION ROUTES (flags of gptqhip_fp4_gemm, both kernels; all give identical bits; measured in profiles/r15_fp4_linear.txt).  What the hardware
// converts do was established by tests/dev/fp4_cvt_probe.hip on an MI355X: v_cvt_scalef32_pk_{f16,bf16,f32}_fp4 takes the byte `byte_sel` of the
// source, low nibble first, and applies ONLY THE EXPONENT of its fp32 scale operand -- sign and mantissa are ignored (1.5 and 1.75 act as 1,
// 0.8125 as 0.5, -1 as 1, 0 as 2^-127).  An e4m3 block scale has three mantissa bits, so it cannot ride on that operand; every route converts the
// codes with scale 1.0 and applies the whole block scale with one packed multiply, which is exact:
//   packed   fp16: v_cvt_scalef32_pk_f16_fp4 + v_pk_mul_f16 by the scale (e4m3 -> fp16 by v_cvt_scalef32_pk_f16_fp8): 2 VALU per two weights (the
//            fp16 default).  bf16: v_cvt_scalef32_pk_bf16_fp4, widened to fp32 by a shift / a mask (gfx950 has no packed bf16 multiply),
//            v_pk_mul_f32, v_cvt_pk_bf16_f32: 5 VALU per two weights.
//   f32      v_cvt_scalef32_pk_f32_fp4 + v_pk_mul_f32 by the scale (v_cvt_f32_fp8) + v_cvt_pk_{f16,bf16}_f32: 3 VALU per two weights (the bf16 default)
// Splitting the scale into the hardware's exponent and a packed multiply by its mantissa costs the same multiply plus the split: not built.
#include "../../include/gptqhip.h"
#include "gptqhip_device.h"
#include "gptqhip_fp4_frag.h"
#include "gptqhip_host.h"

namespace gptqhip {

constexpr int kFp4DecodeRows = 16;     // rows of the decode kernel (one MFMA tile)
constexpr int kFp4DecodeWaves = 8;     // most waves of a decode block (in-block split of K)
constexpr int kFp4Ahead = 4;           // chunks whose loads a decode wave issues before consuming the first
constexpr int kFp4WideTiles = 1024;    // decode: from this many column tiles a block takes kFp4WideNT of them ...
constexpr int kFp4WideNT = 4;
constexpr int kFp4WideAhead = 2;       //   ... with this many chunks in flight (kFp4WideNT x kFp4WideAhead KiB of weights per wave)
constexpr int kFp4GemmWaves = 4;       // general kernel: waves per block
constexpr int kFp4GemmRT = 4;          //   16-row tiles per block (shared by its waves)
constexpr int kFp4GemmCT = 2;          //   16-column tiles per wave
constexpr int kFp4MaxRows = 65535 * 16 * kFp4GemmRT;   // gptqhip_fp8_gemm's limit
constexpr int kFp4Block = 16;          // input features per block scale

struct Fp4Params {
    const uint16_t* x;     // [M, K]
    const uint8_t* wt;     // codes, kernel layout
    const uint8_t* st;     // block scales, kernel layout
    const float* gs;       // global scale (one float) or nullptr = 1.0
    const uint16_t* bias;  // [N] or nullptr
    void* out;             // [M, N] (dequant: [K, N])
    int M, K, N, chunks;
};

template <int ACT>
__device__ __forceinline__ void fp4_store_round(void* out, size_t idx, float v) {
    reinterpret_cast<uint16_t*>(out)[idx] = f32_to_16<ACT>(v);
}

// the four MFMA K-steps of one chunk
template <int ACT, int CVT>
__device__ __forceinline__ f4_t fp4_chunk(const u4_t (&a)[4], u4_t w, uint32_t sw, f4_t acc) {
    const Fp4Scales<ACT, CVT> s = fp4_scales<ACT, CVT>(sw);
    acc = mfma16<ACT>(a[0], fp4x8_to_frag<ACT, CVT, 0>(w.x, s), acc);
    acc = mfma16<ACT>(a[1], fp4x8_to_frag<ACT, CVT, 1>(w.y, s), acc);
    acc = mfma16<ACT>(a[2], fp4x8_to_frag<ACT, CVT, 2>(w.z, s), acc);
    acc = mfma16<ACT>(a[3], fp4x8_to_frag<ACT, CVT, 3>(w.w, s), acc);
    return acc;
}

// NT column tiles per block (they share the wave's activation fragments), AHEAD chunks in flight: the bits do not depend on either -- a tile's
// partial sums are formed by the same wave over the same chunks in the same order in both variants.
template <int ACT, int CVT, int NT, int AHEAD>
__global__ __launch_bounds__(64 * kFp4DecodeWaves, 4) void fp4_decode_kernel(Fp4Params p) {
    __shared__ f4_t red[NT][kFp4DecodeWaves][64];
    const int tiles = p.N / kTileN, tile0 = blockIdx.x * NT;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, W = blockDim.x >> 6;
    const int c16 = lane & 15, rq = lane >> 4;
    const int c0 = wave * p.chunks / W, c1 = (wave + 1) * p.chunks / W;   // W <= chunks: every wave owns at least one chunk
    const uint8_t* wt[NT];
    const uint8_t* st[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int tile = tile0 + t < tiles ? tile0 + t : tiles - 1;       // a ragged last block repeats its last tile and stores it once
        wt[t] = p.wt + (size_t)tile * p.chunks * kFp4BlockBytes + lane * 16;
        st[t] = p.st + (size_t)tile * p.chunks * kFp4ScaleBlockBytes + (16 * (rq >> 1) + c16) * 4;
    }
    const bool live = c16 < p.M;                                          // MFMA row c16 carries activation row c16
    const uint16_t* xl = p.x + (size_t)(live ? c16 : 0) * p.K + 8 * rq;
    f4_t acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = f4_t{0.f, 0.f, 0.f, 0.f};
    for (int base = c0; base < c1; base += AHEAD) {
        u4_t w[AHEAD][NT], a[AHEAD][4];
        uint32_t sw[AHEAD][NT];
#pragma unroll
        for (int u = 0; u < AHEAD; ++u) {
            const int ck = base + u < c1 ? base + u : c1 - 1;   // past the end: a harmless repeat of the wave's last chunk
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                w[u][t] = __builtin_nontemporal_load(reinterpret_cast<const u4_t*>(wt[t] + (size_t)ck * kFp4BlockBytes));
                sw[u][t] = *reinterpret_cast<const uint32_t*>(st[t] + (size_t)ck * kFp4ScaleBlockBytes);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const u4_t z = {0u, 0u, 0u, 0u};
                a[u][j] = live ? *reinterpret_cast<const u4_t*>(xl + (size_t)ck * kChunkK + 32 * j) : z;
            }
        }
#pragma unroll
        for (int u = 0; u < AHEAD; ++u) {
            if (base + u < c1) {   // wave-uniform
#pragma unroll
                for (int t = 0; t < NT; ++t) acc[t] = fp4_chunk<ACT, CVT>(a[u], w[u][t], sw[u][t], acc[t]);
            }
        }
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) red[t][wave][lane] = acc[t];
    __syncthreads();
    if (wave != 0) return;
    const float s2 = p.gs ? p.gs[0] : 1.f;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        if (tile0 + t >= tiles) break;
        f4_t s = red[t][0][lane];
        for (int w = 1; w < W; ++w) s += red[t][w][lane];   // wave order, always
        const int n = (tile0 + t) * kTileN + c16;
        const float b = p.bias ? bits16_to_f32<ACT>(p.bias[n]) : 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int m = 4 * rq + i;   // accumulator register i of lane (rq, c) = row 4 rq + i, column c
            if (m < p.M) fp4_store_round<ACT>(p.out, (size_t)m * p.N + n, s[i] * s2 + b);
        }
    }
}

template <int ACT, int CVT>
__global__ __launch_bounds__(64 * kFp4GemmWaves) void fp4_gemm_kernel(Fp4Params p) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c16 = lane & 15, rq = lane >> 4;
    const int tiles = p.N / kTileN;
    const int tile0 = (blockIdx.x * kFp4GemmWaves + wave) * kFp4GemmCT;
    if (tile0 >= tiles) return;   // (no barrier in this kernel)
    const int nct = tiles - tile0 < kFp4GemmCT ? tiles - tile0 : kFp4GemmCT;
    const int m0 = blockIdx.y * (16 * kFp4GemmRT);
    const uint8_t* wt[kFp4GemmCT];
    const uint8_t* st[kFp4GemmCT];
    const uint16_t* xl[kFp4GemmRT];
    bool live[kFp4GemmRT];
#pragma unroll
    for (int ct = 0; ct < kFp4GemmCT; ++ct) {
        const int tile = tile0 + (ct < nct ? ct : nct - 1);   // a ragged last wave repeats its last tile and stores it once
        wt[ct] = p.wt + (size_t)tile * p.chunks * kFp4BlockBytes + lane * 16;
        st[ct] = p.st + (size_t)tile * p.chunks * kFp4ScaleBlockBytes + (16 * (rq >> 1) + c16) * 4;
    }
#pragma unroll
    for (int rt = 0; rt < kFp4GemmRT; ++rt) {
        const int m = m0 + 16 * rt + c16;
        live[rt] = m < p.M;
        xl[rt] = p.x + (size_t)(live[rt] ? m : 0) * p.K + 8 * rq;
    }
    const f4_t zero = {0.f, 0.f, 0.f, 0.f};
    f4_t acc[kFp4GemmRT][kFp4GemmCT];
#pragma unroll
    for (int rt = 0; rt < kFp4GemmRT; ++rt)
#pragma unroll
        for (int ct = 0; ct < kFp4GemmCT; ++ct) acc[rt][ct] = zero;
    for (int ck = 0; ck < p.chunks; ++ck) {
        u4_t b[kFp4GemmCT][4];
#pragma unroll
        for (int ct = 0; ct < kFp4GemmCT; ++ct) {
            const u4_t w = *reinterpret_cast<const u4_t*>(wt[ct] + (size_t)ck * kFp4BlockBytes);
            const Fp4Scales<ACT, CVT> s = fp4_scales<ACT, CVT>(*reinterpret_cast<const uint32_t*>(st[ct] + (size_t)ck * kFp4ScaleBlockBytes));
            b[ct][0] = fp4x8_to_frag<ACT, CVT, 0>(w.x, s);
            b[ct][1] = fp4x8_to_frag<ACT, CVT, 1>(w.y, s);
            b[ct][2] = fp4x8_to_frag<ACT, CVT, 2>(w.z, s);
            b[ct][3] = fp4x8_to_frag<ACT, CVT, 3>(w.w, s);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma unroll
            for (int rt = 0; rt < kFp4GemmRT; ++rt) {
                const u4_t z = {0u, 0u, 0u, 0u};
                const u4_t a = live[rt] ? *reinterpret_cast<const u4_t*>(xl[rt] + (size_t)ck * kChunkK + 32 * j) : z;
#pragma unroll
                for (int ct = 0; ct < kFp4GemmCT; ++ct) acc[rt][ct] = mfma16<ACT>(a, b[ct][j], acc[rt][ct]);
            }
        }
    }
    const float s2 = p.gs ? p.gs[0] : 1.f;
#pragma unroll
    for (int ct = 0; ct < kFp4GemmCT; ++ct) {
        if (ct >= nct) break;
        const int n = (tile0 + ct) * kTileN + c16;
        const float b = p.bias ? bits16_to_f32<ACT>(p.bias[n]) : 0.f;
#pragma unroll
        for (int rt = 0; rt < kFp4GemmRT; ++rt) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int m = m0 + 16 * rt + 4 * rq + i;
                if (m < p.M) fp4_store_round<ACT>(p.out, (size_t)m * p.N + n, acc[rt][ct][i] * s2 + b);
            }
        }
    }
}

// byte offset of the code pair (k, k ^ 1) of column n in the kernel layout; k & 1 picks the nibble
__device__ __forceinline__ size_t fp4_tiled_offset(int k, int n, int chunks) {
    const int kk = k & 127;
    const int lane = (((kk & 31) >> 3) << 4) | (n & 15);
    return (((size_t)(n >> 4) * chunks + (k >> 7)) * 64 + lane) * 16 + 4 * (kk >> 5) + ((kk & 7) >> 1);
}
// byte offset of the scale of (k, n)
__device__ __forceinline__ size_t fp4_scale_offset(int k, int n, int chunks) {
    const int blk = (k & 127) >> 4;   // the chunk's 16-wide block: 2 j + (rq >> 1)
    return (((size_t)(n >> 4) * chunks + (k >> 7)) * 32 + 16 * (blk & 1) + (n & 15)) * 4 + (blk >> 1);
}

template <int OUT>   // kFP16 | kBF16 | 2 = float32
__global__ __launch_bounds__(256) void fp4_dequant_kernel(Fp4Params p) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)p.K * p.N) return;
    const int k = (int)(idx / p.N), n = (int)(idx % p.N);
    const uint32_t nib = (p.wt[fp4_tiled_offset(k, n, p.chunks)] >> (4 * (k & 1))) & 0xfu;
    const float code = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(nib, 1.0f, 0)[0];
    const float sb = __builtin_amdgcn_cvt_f32_fp8((int)p.st[fp4_scale_offset(k, n, p.chunks)], 0);
    float v = (code * sb) * (p.gs ? p.gs[0] : 1.f);   // the first product is exact, the second is rounded to fp32
    // ... and held in a register of its own: hipcc would fold it into the fp16 conversion (v_fma_mixlo_f16), which rounds the exact product to
    // fp16, one ulp off round(fp32 product) wherever the fp32 product is an fp16 tie (gptqhip_fp8.hip: fp8_dequant_kernel)
    asm volatile("" : "+v"(v));
    if constexpr (OUT == 2) {
        reinterpret_cast<float*>(p.out)[idx] = v;
    } else {
        fp4_store_round<OUT>(p.out, idx, v);
    }
}

// checkpoint layout uint8 [N, K / 2] -> kernel layout; one thread per 16-byte unit (a lane's four K-step dwords of one chunk)
__global__ __launch_bounds__(256) void fp4_repack_kernel(const uint8_t* __restrict__ w, uint8_t* __restrict__ wt, int K, int N, int chunks) {
    const size_t unit = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (unit >= (size_t)K * N / 32) return;
    const int lane = (int)(unit & 63);
    const size_t blk = unit >> 6;
    const int chunk = (int)(blk % chunks), tile = (int)(blk / chunks);
    const uint8_t* src = w + (size_t)(tile * kTileN + (lane & 15)) * (K / 2) + chunk * (kChunkK / 2) + 4 * (lane >> 4);
    u4_t o;
    o.x = *reinterpret_cast<const uint32_t*>(src);
    o.y = *reinterpret_cast<const uint32_t*>(src + 16);
    o.z = *reinterpret_cast<const uint32_t*>(src + 32);
    o.w = *reinterpret_cast<const uint32_t*>(src + 48);
    *reinterpret_cast<u4_t*>(wt + unit * 16) = o;
}

// weight_scale uint8 [N, K / 16] -> kernel layout; one thread per dword (the four K-step scales of a lane pair)
__global__ __launch_bounds__(256) void fp4_repack_scale_kernel(const uint8_t* __restrict__ s, uint8_t* __restrict__ st, int K, int N, int chunks) {
    const size_t unit = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (unit >= (size_t)K * N / 64) return;
    const int c = (int)(unit & 15), hi = (int)((unit >> 4) & 1);
    const size_t blk = unit >> 5;
    const int chunk = (int)(blk % chunks), tile = (int)(blk / chunks);
    const uint8_t* src = s + (size_t)(tile * kTileN + c) * (K / kFp4Block) + chunk * 8 + hi;
    const uint32_t o = (uint32_t)src[0] | ((uint32_t)src[2] << 8) | ((uint32_t)src[4] << 16) | ((uint32_t)src[6] << 24);
    reinterpret_cast<uint32_t*>(st)[unit] = o;
}

static const char* fp4_shape_error(int M, int K, int N, int block_size) {
    if (block_size != kFp4Block) return "block size must be 16 (NVFP4; MXFP4's 32 is not supported)";
    if (M < 0 || M > kFp4MaxRows) return "M out of range";
    if (K <= 0 || K % kChunkK != 0) return "in_features (K) must be a positive multiple of 128";
    if (N <= 0 || N % kTileN != 0) return "out_features (N) must be a positive multiple of 16";
    return nullptr;
}

static Fp4Params fp4_params(const void* x, const uint8_t* wt, const uint8_t* st, const float* gs, const void* bias, void* out, int M, int K, int N) {
    Fp4Params p;
    p.x = reinterpret_cast<const uint16_t*>(x);
    p.wt = wt;
    p.st = st;
    p.gs = gs;
    p.bias = reinterpret_cast<const uint16_t*>(bias);
    p.out = out;
    p.M = M;
    p.K = K;
    p.N = N;
    p.chunks = K / kChunkK;
    return p;
}

// required pointers: non-null and 16-byte aligned; optional ones: aligned (global_scale: to a float)
static int fp4_check_ptrs(const char* fn, const void* const* req, int nreq, const void* opt, const float* gs) {
    for (int i = 0; i < nreq; ++i) {
        if (req[i] == nullptr) {
            set_error("%s: null tensor pointer", fn);
            return GPTQHIP_EINVAL;
        }
    }
    for (int i = 0; i <= nreq; ++i) {
        const void* q = i < nreq ? req[i] : opt;
        if (reinterpret_cast<uintptr_t>(q) % 16 != 0) {
            set_error("%s: tensors must be 16-byte aligned", fn);
            return GPTQHIP_EINVAL;
        }
    }
    if (reinterpret_cast<uintptr_t>(gs) % 4 != 0) {
        set_error("%s: global_scale must be aligned to a float", fn);
        return GPTQHIP_EINVAL;
    }
    return GPTQHIP_OK;
}

// The decode variant is a rule of (K, N) alone, like the grid: wide layers (>= kFp4WideTiles column tiles: two resident blocks for every CU even
// at four tiles per block) give each wave four column tiles per chunk (profiles/r15_fp4_linear.txt).
template <int ACT, int CVT>
static void fp4_launch_decode(const Fp4Params& p, hipStream_t stream) {
    const int waves = p.chunks < kFp4DecodeWaves ? p.chunks : kFp4DecodeWaves;
    const int tiles = p.N / kTileN;
    const dim3 block(64 * waves);
    if (tiles >= kFp4WideTiles) hipLaunchKernelGGL((fp4_decode_kernel<ACT, CVT, kFp4WideNT, kFp4WideAhead>), dim3(ceil_div(tiles, kFp4WideNT)), block, 0, stream, p);
    else hipLaunchKernelGGL((fp4_decode_kernel<ACT, CVT, 1, kFp4Ahead>), dim3(tiles), block, 0, stream, p);
}

template <int ACT, int CVT>
static void fp4_launch_gemm(const Fp4Params& p, hipStream_t stream) {
    const dim3 grid(ceil_div(p.N / kTileN, kFp4GemmWaves * kFp4GemmCT), ceil_div(p.M, 16 * kFp4GemmRT)), block(64 * kFp4GemmWaves);
    hipLaunchKernelGGL((fp4_gemm_kernel<ACT, CVT>), grid, block, 0, stream, p);
}

}  // namespace gptqhip

using namespace gptqhip;

extern "C" {

int gptqhip_fp4_supported(int M, int K, int N, int block_size, int act_dtype) {
    if (act_dtype != GPTQHIP_FP16 && act_dtype != GPTQHIP_BF16) return 0;
    return fp4_shape_error(M, K, N, block_size) == nullptr ? 1 : 0;
}

size_t gptqhip_fp4_tiled_bytes(int K, int N) {
    return fp4_shape_error(0, K, N, kFp4Block) == nullptr ? (size_t)K * N / 2 : 0;
}

size_t gptqhip_fp4_scale_bytes(int K, int N) {
    return fp4_shape_error(0, K, N, kFp4Block) == nullptr ? (size_t)K * N / kFp4Block : 0;
}

int gptqhip_fp4_repack(const uint8_t* weight, const uint8_t* weight_scale, uint8_t* weight_t, uint8_t* scale_t, int K, int N, int block_size,
                       gptqhip_stream_t stream) {
    const void* req[] = {weight, weight_scale, weight_t, scale_t};
    int rc = fp4_check_ptrs("gptqhip_fp4_repack", req, 4, nullptr, nullptr);
    if (rc) return rc;
    if (const char* why = fp4_shape_error(0, K, N, block_size)) {
        set_error("gptqhip_fp4_repack: %s (K=%d N=%d block size %d)", why, K, N, block_size);
        return GPTQHIP_EINVAL;
    }
    if (weight == weight_t || weight_scale == scale_t) {
        set_error("gptqhip_fp4_repack: the relayout is not in place");
        return GPTQHIP_EINVAL;
    }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const size_t units = (size_t)K * N / 32, sunits = (size_t)K * N / 64;
    hipLaunchKernelGGL(fp4_repack_kernel, dim3((unsigned)((units + 255) / 256)), dim3(256), 0, s, weight, weight_t, K, N, K / kChunkK);
    hipLaunchKernelGGL(fp4_repack_scale_kernel, dim3((unsigned)((sunits + 255) / 256)), dim3(256), 0, s, weight_scale, scale_t, K, N, K / kChunkK);
    return check_hip(hipGetLastError(), "fp4_repack_kernel launch");
}

int gptqhip_fp4_gemm(const void* x, const uint8_t* weight_t, const uint8_t* scale_t, const float* global_scale, const void* bias, void* out, int M,
                     int K, int N, int block_size, int act_dtype, int flags, gptqhip_stream_t stream) {
    if (M == 0) return GPTQHIP_OK;   // empty batch: an empty tensor
    const void* req[] = {x, weight_t, scale_t, out};
    int rc = fp4_check_ptrs("gptqhip_fp4_gemm", req, 4, bias, global_scale);
    if (rc) return rc;
    if (act_dtype != GPTQHIP_FP16 && act_dtype != GPTQHIP_BF16) {
        set_error("gptqhip_fp4_gemm: unsupported activation dtype tag %d (fp16 = 0, bf16 = 1)", act_dtype);
        return GPTQHIP_EINVAL;
    }
    if (const char* why = fp4_shape_error(M, K, N, block_size)) {
        set_error("gptqhip_fp4_gemm: %s (M=%d K=%d N=%d block size %d)", why, M, K, N, block_size);
        return GPTQHIP_EINVAL;
    }
    int cvt = flags & GPTQHIP_FP4_CVT_MASK;
    if ((flags & ~GPTQHIP_FP4_CVT_MASK) != 0 || cvt > GPTQHIP_FP4_CVT_F32) {
        set_error("gptqhip_fp4_gemm: unsupported flags 0x%x", flags);
        return GPTQHIP_EINVAL;
    }
    if (cvt == GPTQHIP_FP4_CVT_DEFAULT) cvt = act_dtype == GPTQHIP_FP16 ? GPTQHIP_FP4_CVT_PACKED : GPTQHIP_FP4_CVT_F32;
    const bool packed = cvt == GPTQHIP_FP4_CVT_PACKED;
    const Fp4Params p = fp4_params(x, weight_t, scale_t, global_scale, bias, out, M, K, N);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (M > kFp4DecodeRows) {
        if (act_dtype == GPTQHIP_FP16) {
            if (packed) fp4_launch_gemm<kFP16, kFp4CvtPacked>(p, s);
            else fp4_launch_gemm<kFP16, kFp4CvtF32>(p, s);
        } else {
            if (packed) fp4_launch_gemm<kBF16, kFp4CvtPacked>(p, s);
            else fp4_launch_gemm<kBF16, kFp4CvtF32>(p, s);
        }
        return check_hip(hipGetLastError(), "fp4_gemm_kernel launch");
    }
    if (act_dtype == GPTQHIP_FP16) {
        if (packed) fp4_launch_decode<kFP16, kFp4CvtPacked>(p, s);
        else fp4_launch_decode<kFP16, kFp4CvtF32>(p, s);
    } else {
        if (packed) fp4_launch_decode<kBF16, kFp4CvtPacked>(p, s);
        else fp4_launch_decode<kBF16, kFp4CvtF32>(p, s);
    }
    return check_hip(hipGetLastError(), "fp4_decode_kernel launch");
}

int gptqhip_fp4_dequant(const uint8_t* weight_t, const uint8_t* scale_t, const float* global_scale, void* out, int K, int N, int block_size,
                        int out_dtype, gptqhip_stream_t stream) {
    const void* req[] = {weight_t, scale_t, out};
    int rc = fp4_check_ptrs("gptqhip_fp4_dequant", req, 3, nullptr, global_scale);
    if (rc) return rc;
    if (out_dtype != GPTQHIP_FP16 && out_dtype != GPTQHIP_BF16 && out_dtype != GPTQHIP_FP32) {
        set_error("gptqhip_fp4_dequant: unsupported output dtype tag %d (fp16 = 0, bf16 = 1, fp32 = 2)", out_dtype);
        return GPTQHIP_EINVAL;
    }
    if (const char* why = fp4_shape_error(0, K, N, block_size)) {
        set_error("gptqhip_fp4_dequant: %s (K=%d N=%d block size %d)", why, K, N, block_size);
        return GPTQHIP_EINVAL;
    }
    const Fp4Params p = fp4_params(nullptr, weight_t, scale_t, global_scale, nullptr, out, 0, K, N);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)(((size_t)K * N + 255) / 256)), block(256);
    if (out_dtype == GPTQHIP_FP16) hipLaunchKernelGGL((fp4_dequant_kernel<kFP16>), grid, block, 0, s, p);
    else if (out_dtype == GPTQHIP_BF16) hipLaunchKernelGGL((fp4_dequant_kernel<kBF16>), grid, block, 0, s, p);
    else hipLaunchKernelGGL((fp4_dequant_kernel<2>), grid, block, 0, s, p);
    return check_hip(hipGetLastError(), "fp4_dequant_kernel launch");
}

}  // extern "C"
