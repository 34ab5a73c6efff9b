// FP8 (OCP float8_e4m3fn) weight-only linear, W8A16 (include/gptqhip.h: gptqhip_fp8_supported / gptqhip_fp8_tiled_bytes / gptqhip_fp8_repack /
// gptqhip_fp8_gemm / gptqhip_fp8_dequant).  Replaces TorchFP8Linear (gptqmodel/nn_modules/qlinear/fp8.py), whose ROCm forward dequantises the
// whole [out, in] weight into the activation dtype on every call and then runs a dense matmul.
//
// SEMANTICS.  W[n, k] = code[n, k] / scale_inv[...] (the reference's "inverse" scale semantics), scale_inv fp32 in one of three layouts:
//   tensor  scale_inv []            row  scale_inv [N]            block  scale_inv [N / br, K / bc]   (a column's scale row is n / br)
// e4m3 -> fp16 and e4m3 -> bf16 are EXACT, so the codes enter the matrix pipe unscaled and 1 / scale_inv multiplies the fp32 accumulator: once
// in the epilogue for tensor / row scales, once per bc-wide K block for block scales.  The reciprocal is formed ONCE, at post_init, by an IEEE
// fp32 division into a reciprocal-scale buffer (gptqhip_fp8_repack).  Then the bias is added in fp32 and the sum is rounded ONCE to the activation
// dtype:   y = round( sum_kb (1 / scale_inv[n / br, kb]) * (sum_{k in kb} x[k] * code[n, k]) + bias[n] ).
// This is deliberately NOT the reference's chain (every dequantised weight rounded to the activation dtype, then the matmul's rounding, then the
// bias add's): it is the choice decode form 5 and the MoE down stage made (exact products, fp32 sums, one rounding), and it is no further from
// float64 arithmetic than that chain (tests/test_gpu_fp8.py holds it to that bar).
//
// NaN CODES (0x7f, 0xff): UNDEFINED, never produced by the packer (it clamps to +-448 before the cast).  The hardware converts propagate them; the
// fp16 bit-placement route turns them into finite values.
//
// SUPPORTED SET (enforced by gptqhip_fp8_supported, the one host predicate; everything else is GPTQHIP_EINVAL before any device access):
//   format float8_e4m3fn; activations fp16 | bf16; K % 128 == 0, N % 16 == 0; 0 <= M <= 65535 * 64;
//   tensor and row scales; block scales with bc % 128 == 0, bc | K, br >= 1, br | N (br need not divide the 16-column tile).
//
// KERNEL LAYOUT (gptqhip_fp8_repack, once in post_init; the shape of gptqhip_repack_tiled's 8-bit layout):
//   byte[(((tile * chunks + chunk) * 2 + h) * 64 + lane) * 16 + 8 * jj + e],  tile = n / 16, chunk = k / 128, lane = (rq << 4) | c,
//   holds column n = 16 tile + c, row k = 128 chunk + 32 (2 h + jj) + 8 rq + e: the 8 bytes (jj, e = 0 .. 7) are lane (rq, c)'s B fragment of K-step
//   2 h + jj of mfma_f32_16x16x32, in natural k order.  A (tile, chunk) block is 2 KiB contiguous = two 16 B-per-lane wave loads, and the chunks
//   of a tile follow each other: every wave streams a linear address range.
//
// (a) fp8_decode_kernel, 1 <= M <= 16: grid = N / 16 column tiles, min(8, chunks) waves per block; wave w takes the CONTIGUOUS chunk range
//     [w * chunks / W, (w + 1) * chunks / W) -- a rule of the shape alone -- with the loads of up to four chunks issued before the first is
//     consumed, all M rows in one MFMA tile (rows >= M are zero, never loaded).  Partial accumulators go through LDS and wave 0 adds them in wave
//     order: no floating-point atomics, so two runs give the same bits; MFMA rows never mix and the split does not depend on M, so a row's bits
//     do not depend on which other rows are in the batch.  One launch whose grid depends on (K, N) only: capturable in a graph.
// (b) fp8_gemm_kernel, M >= 17: 4 waves per block, a block covers 64 rows x 128 columns (a wave: 4 row tiles x 2 column tiles), A fragments read
//     straight from global memory, B fragments converted in registers from the same layout; no workspace.  Correctness first.
// (c) fp8_dequant_kernel: [K, N] in fp16 | bf16 | fp32, each element round(code * (1 / scale_inv)) from the fp32 product, once.
//
// CONVERSION ROUTES (flags of gptqhip_fp8_gemm, decode kernel; measured in profiles/r09_fp8_linear.txt):
//   packed   v_cvt_scalef32_pk_{f16,bf16}_fp8 with scale 1.0: two weights per instruction (the default)
//   f32      v_cvt_pk_f32_fp8 + v_cvt_pk_{f16,bf16}_f32: two instructions per two weights
//   bits     fp16 only: ((b & 0x7f) << 7) | ((b & 0x80) << 8) = the exact value * 2^-8 (e4m3 subnormals land on fp16 subnormals, which the matrix
//            pipe takes at face value: tests/dev/mfma_denorm_probe.hip); the 2^8 multiplies the accumulator in the epilogue (exact)
#include "../../include/gptqhip.h"
#include "gptqhip_device.h"
#include "gptqhip_fp8_frag.h"
#include "gptqhip_host.h"

namespace gptqhip {

constexpr int kFp8DecodeRows = 16;     // rows of the decode kernel (one MFMA tile)
constexpr int kFp8DecodeWaves = 8;     // most waves of a decode block (in-block split of K)
constexpr int kFp8Ahead = 4;           // chunks whose loads a decode wave issues before consuming the first
constexpr int kFp8GemmWaves = 4;       // general kernel: waves per block
constexpr int kFp8GemmRT = 4;          //   16-row tiles per block (shared by its waves)
constexpr int kFp8GemmCT = 2;          //   16-column tiles per wave
constexpr int kFp8MaxRows = 65535 * 16 * kFp8GemmRT;

constexpr int kScaleTensor = GPTQHIP_FP8_SCALE_TENSOR, kScaleRow = GPTQHIP_FP8_SCALE_ROW, kScaleBlock = GPTQHIP_FP8_SCALE_BLOCK;

struct Fp8Params {
    const uint16_t* x;     // [M, K]
    const uint8_t* wt;     // kernel layout
    const float* rs;       // reciprocal scales: [1] | [N] | [N / br, kbn]
    const uint16_t* bias;  // [N] or nullptr
    void* out;             // [M, N] (dequant: [K, N])
    int M, K, N, chunks, mode;
    int br, bc;            // block scales: rows (of the [N, K] weight) and columns per scale
    int kbn, cpb;          //               scales per weight row (K / bc), 128-row chunks per scale (bc / 128)
};

template <int ACT>
__device__ __forceinline__ void store_round(void* out, size_t idx, float v) {
    reinterpret_cast<uint16_t*>(out)[idx] = f32_to_16<ACT>(v);
}

template <int ACT, int CVT, bool BLOCK>
__global__ __launch_bounds__(64 * kFp8DecodeWaves) void fp8_decode_kernel(Fp8Params p) {
    __shared__ f4_t red[kFp8DecodeWaves][64];
    const int tile = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, W = blockDim.x >> 6;
    const int c16 = lane & 15, rq = lane >> 4;
    const int c0 = wave * p.chunks / W, c1 = (wave + 1) * p.chunks / W;   // W <= chunks: every wave owns at least one chunk
    const uint8_t* wt = p.wt + (size_t)tile * p.chunks * kFp8BlockBytes + lane * 16;
    const bool live = c16 < p.M;                                          // MFMA row c16 carries activation row c16
    const uint16_t* xl = p.x + (size_t)(live ? c16 : 0) * p.K + 8 * rq;
    const float* rs = BLOCK ? p.rs + (size_t)((tile * kTileN + c16) / p.br) * p.kbn : p.rs;
    const f4_t zero = {0.f, 0.f, 0.f, 0.f};
    f4_t acc = zero, tot = zero;
    for (int base = c0; base < c1; base += kFp8Ahead) {
        u4_t w[kFp8Ahead][2], a[kFp8Ahead][4];
        float r[kFp8Ahead];
#pragma unroll
        for (int u = 0; u < kFp8Ahead; ++u) {
            const int ck = base + u < c1 ? base + u : c1 - 1;   // past the end: a harmless repeat of the wave's last chunk
            w[u][0] = __builtin_nontemporal_load(reinterpret_cast<const u4_t*>(wt + (size_t)ck * kFp8BlockBytes));
            w[u][1] = __builtin_nontemporal_load(reinterpret_cast<const u4_t*>(wt + (size_t)ck * kFp8BlockBytes + 1024));
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const u4_t z = {0u, 0u, 0u, 0u};
                a[u][j] = live ? *reinterpret_cast<const u4_t*>(xl + (size_t)ck * kChunkK + 32 * j) : z;
            }
            r[u] = BLOCK ? rs[ck / p.cpb] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < kFp8Ahead; ++u) {
            const int ck = base + u;
            if (ck < c1) {   // wave-uniform
                acc = mfma16<ACT>(a[u][0], fp8x8_to_frag<ACT, CVT>(w[u][0].x, w[u][0].y), acc);
                acc = mfma16<ACT>(a[u][1], fp8x8_to_frag<ACT, CVT>(w[u][0].z, w[u][0].w), acc);
                acc = mfma16<ACT>(a[u][2], fp8x8_to_frag<ACT, CVT>(w[u][1].x, w[u][1].y), acc);
                acc = mfma16<ACT>(a[u][3], fp8x8_to_frag<ACT, CVT>(w[u][1].z, w[u][1].w), acc);
                if (BLOCK && ((ck + 1) % p.cpb == 0 || ck + 1 == c1)) {   // the K block (or the wave's share of it) ends here
                    tot += acc * r[u];
                    acc = zero;
                }
            }
        }
    }
    red[wave][lane] = BLOCK ? tot : acc;
    __syncthreads();
    if (wave != 0) return;
    f4_t s = red[0][lane];
    for (int w = 1; w < W; ++w) s += red[w][lane];   // wave order, always
    const int n = tile * kTileN + c16;
    float scale = BLOCK ? 1.f : (p.mode == kScaleRow ? p.rs[n] : p.rs[0]);
    if (CVT == kCvtBits) scale *= 256.f;
    const float b = p.bias ? bits16_to_f32<ACT>(p.bias[n]) : 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m = 4 * rq + i;   // accumulator register i of lane (rq, c) = row 4 rq + i, column c
        if (m < p.M) store_round<ACT>(p.out, (size_t)m * p.N + n, s[i] * scale + b);
    }
}

template <int ACT, bool BLOCK>
__global__ __launch_bounds__(64 * kFp8GemmWaves) void fp8_gemm_kernel(Fp8Params p) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c16 = lane & 15, rq = lane >> 4;
    const int tiles = p.N / kTileN;
    const int tile0 = (blockIdx.x * kFp8GemmWaves + wave) * kFp8GemmCT;
    if (tile0 >= tiles) return;   // (no barrier in this kernel)
    const int nct = tiles - tile0 < kFp8GemmCT ? tiles - tile0 : kFp8GemmCT;
    const int m0 = blockIdx.y * (16 * kFp8GemmRT);
    const uint8_t* wt[kFp8GemmCT];
    const float* rs[kFp8GemmCT];
    const uint16_t* xl[kFp8GemmRT];
    bool live[kFp8GemmRT];
#pragma unroll
    for (int ct = 0; ct < kFp8GemmCT; ++ct) {
        const int tile = tile0 + (ct < nct ? ct : nct - 1);   // a ragged last wave repeats its last tile and stores it once
        wt[ct] = p.wt + (size_t)tile * p.chunks * kFp8BlockBytes + lane * 16;
        rs[ct] = BLOCK ? p.rs + (size_t)((tile * kTileN + c16) / p.br) * p.kbn : p.rs;
    }
#pragma unroll
    for (int rt = 0; rt < kFp8GemmRT; ++rt) {
        const int m = m0 + 16 * rt + c16;
        live[rt] = m < p.M;
        xl[rt] = p.x + (size_t)(live[rt] ? m : 0) * p.K + 8 * rq;
    }
    const f4_t zero = {0.f, 0.f, 0.f, 0.f};
    f4_t acc[kFp8GemmRT][kFp8GemmCT], tot[kFp8GemmRT][kFp8GemmCT];
#pragma unroll
    for (int rt = 0; rt < kFp8GemmRT; ++rt)
#pragma unroll
        for (int ct = 0; ct < kFp8GemmCT; ++ct) acc[rt][ct] = tot[rt][ct] = zero;
    for (int ck = 0; ck < p.chunks; ++ck) {
        u4_t w[kFp8GemmCT][2];
#pragma unroll
        for (int ct = 0; ct < kFp8GemmCT; ++ct) {
            w[ct][0] = *reinterpret_cast<const u4_t*>(wt[ct] + (size_t)ck * kFp8BlockBytes);
            w[ct][1] = *reinterpret_cast<const u4_t*>(wt[ct] + (size_t)ck * kFp8BlockBytes + 1024);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            u4_t b[kFp8GemmCT];
#pragma unroll
            for (int ct = 0; ct < kFp8GemmCT; ++ct) {
                b[ct] = (j & 1) ? fp8x8_to_frag<ACT, kCvtPacked>(w[ct][j >> 1].z, w[ct][j >> 1].w)
                                : fp8x8_to_frag<ACT, kCvtPacked>(w[ct][j >> 1].x, w[ct][j >> 1].y);
            }
#pragma unroll
            for (int rt = 0; rt < kFp8GemmRT; ++rt) {
                const u4_t z = {0u, 0u, 0u, 0u};
                const u4_t a = live[rt] ? *reinterpret_cast<const u4_t*>(xl[rt] + (size_t)ck * kChunkK + 32 * j) : z;
#pragma unroll
                for (int ct = 0; ct < kFp8GemmCT; ++ct) acc[rt][ct] = mfma16<ACT>(a, b[ct], acc[rt][ct]);
            }
        }
        if (BLOCK && (ck + 1) % p.cpb == 0) {   // bc | K: the last chunk closes the last K block
#pragma unroll
            for (int ct = 0; ct < kFp8GemmCT; ++ct) {
                const float r = rs[ct][ck / p.cpb];
#pragma unroll
                for (int rt = 0; rt < kFp8GemmRT; ++rt) {
                    tot[rt][ct] += acc[rt][ct] * r;
                    acc[rt][ct] = zero;
                }
            }
        }
    }
#pragma unroll
    for (int ct = 0; ct < kFp8GemmCT; ++ct) {
        if (ct >= nct) break;
        const int n = (tile0 + ct) * kTileN + c16;
        const float scale = BLOCK ? 1.f : (p.mode == kScaleRow ? p.rs[n] : p.rs[0]);
        const float b = p.bias ? bits16_to_f32<ACT>(p.bias[n]) : 0.f;
#pragma unroll
        for (int rt = 0; rt < kFp8GemmRT; ++rt) {
            const f4_t s = BLOCK ? tot[rt][ct] : acc[rt][ct];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int m = m0 + 16 * rt + 4 * rq + i;
                if (m < p.M) store_round<ACT>(p.out, (size_t)m * p.N + n, s[i] * scale + b);
            }
        }
    }
}

// byte offset of (k, n) in the kernel layout
__device__ __forceinline__ size_t fp8_tiled_offset(int k, int n, int chunks) {
    const int kk = k & 127;
    const int lane = (((kk & 31) >> 3) << 4) | (n & 15);
    return ((((size_t)(n >> 4) * chunks + (k >> 7)) * 2 + (kk >> 6)) * 64 + lane) * 16 + 8 * ((kk >> 5) & 1) + (kk & 7);
}

template <int OUT>   // kFP16 | kBF16 | 2 = float32
__global__ __launch_bounds__(256) void fp8_dequant_kernel(Fp8Params p) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)p.K * p.N) return;
    const int k = (int)(idx / p.N), n = (int)(idx % p.N);
    const float code = __builtin_amdgcn_cvt_f32_fp8((int)p.wt[fp8_tiled_offset(k, n, p.chunks)], 0);
    const float r = p.mode == kScaleTensor ? p.rs[0] : p.mode == kScaleRow ? p.rs[n] : p.rs[(size_t)(n / p.br) * p.kbn + k / p.bc];
    // The fp32 product is held in a register of its own.  Left to itself hipcc folds the multiply into the fp16 conversion (v_fma_mixlo_f16,
    // with a +0 addend for a plain product), which rounds the EXACT product to fp16: one ulp off round(fp32 product) wherever the fp32 product is
    // an fp16 tie, so the fp16 output was not the fp32 output rounded; the +0 addend also turned the -0 of code 0x80 into +0.
    float v = code * r;
    asm volatile("" : "+v"(v));
    if constexpr (OUT == 2) {
        reinterpret_cast<float*>(p.out)[idx] = v;
    } else {
        store_round<OUT>(p.out, idx, v);
    }
}

// checkpoint layout [N, K] (K contiguous) -> kernel layout; one thread per 16-byte unit
__global__ __launch_bounds__(256) void fp8_repack_kernel(const uint8_t* __restrict__ w, uint8_t* __restrict__ wt, int K, int N, int chunks) {
    const size_t unit = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (unit >= (size_t)K * N / 16) return;
    const int lane = (int)(unit & 63), h = (int)((unit >> 6) & 1);
    const size_t blk = unit >> 7;
    const int chunk = (int)(blk % chunks), tile = (int)(blk / chunks);
    const uint8_t* src = w + (size_t)(tile * kTileN + (lane & 15)) * K + chunk * kChunkK + 64 * h + 8 * (lane >> 4);
    const u2_t lo = *reinterpret_cast<const u2_t*>(src), hi = *reinterpret_cast<const u2_t*>(src + 32);
    u4_t o;
    o.x = lo.x;
    o.y = lo.y;
    o.z = hi.x;
    o.w = hi.y;
    *reinterpret_cast<u4_t*>(wt + unit * 16) = o;
}

// the reciprocal-scale buffer: IEEE fp32 division (hipcc's default is the correctly rounded divide), once
__global__ __launch_bounds__(256) void fp8_rscale_kernel(const float* __restrict__ scale_inv, float* __restrict__ rs, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) rs[i] = __fdiv_rn(1.0f, scale_inv[i]);
}

static const char* fp8_shape_error(int M, int K, int N, int mode, int br, int bc) {
    if (M < 0 || M > kFp8MaxRows) return "M out of range";
    if (K <= 0 || K % kChunkK != 0) return "in_features (K) must be a positive multiple of 128";
    if (N <= 0 || N % kTileN != 0) return "out_features (N) must be a positive multiple of 16";
    if (mode == kScaleTensor || mode == kScaleRow) return nullptr;
    if (mode != kScaleBlock) return "scale layout must be tensor (0), row (1) or block (2)";
    if (bc <= 0 || bc % kChunkK != 0 || K % bc != 0) return "block columns must be a multiple of 128 dividing in_features";
    if (br <= 0 || N % br != 0) return "block rows must divide out_features";
    return nullptr;
}

static size_t fp8_scale_count(int K, int N, int mode, int br, int bc) {
    return mode == kScaleTensor ? 1 : mode == kScaleRow ? (size_t)N : (size_t)(N / br) * (K / bc);
}

static Fp8Params fp8_params(const void* x, const uint8_t* wt, const float* rs, const void* bias, void* out, int M, int K, int N, int mode, int br,
                            int bc) {
    Fp8Params p;
    p.x = reinterpret_cast<const uint16_t*>(x);
    p.wt = wt;
    p.rs = rs;
    p.bias = reinterpret_cast<const uint16_t*>(bias);
    p.out = out;
    p.M = M;
    p.K = K;
    p.N = N;
    p.chunks = K / kChunkK;
    p.mode = mode;
    const bool block = mode == kScaleBlock;
    p.br = block ? br : 1;
    p.bc = block ? bc : K;
    p.kbn = block ? K / bc : 1;
    p.cpb = block ? bc / kChunkK : p.chunks;
    return p;
}

static int fp8_check_ptrs(const char* fn, const void* const* req, int nreq, const void* opt) {
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
    return GPTQHIP_OK;
}

template <int ACT, int CVT>
static void fp8_launch_decode(const Fp8Params& p, hipStream_t stream) {
    const int waves = p.chunks < kFp8DecodeWaves ? p.chunks : kFp8DecodeWaves;
    const dim3 grid(p.N / kTileN), block(64 * waves);
    if (p.mode == kScaleBlock) hipLaunchKernelGGL((fp8_decode_kernel<ACT, CVT, true>), grid, block, 0, stream, p);
    else hipLaunchKernelGGL((fp8_decode_kernel<ACT, CVT, false>), grid, block, 0, stream, p);
}

template <int ACT>
static void fp8_launch_gemm(const Fp8Params& p, hipStream_t stream) {
    const dim3 grid(ceil_div(p.N / kTileN, kFp8GemmWaves * kFp8GemmCT), ceil_div(p.M, 16 * kFp8GemmRT)), block(64 * kFp8GemmWaves);
    if (p.mode == kScaleBlock) hipLaunchKernelGGL((fp8_gemm_kernel<ACT, true>), grid, block, 0, stream, p);
    else hipLaunchKernelGGL((fp8_gemm_kernel<ACT, false>), grid, block, 0, stream, p);
}

}  // namespace gptqhip

using namespace gptqhip;

extern "C" {

int gptqhip_fp8_supported(int M, int K, int N, int scale_mode, int block_rows, int block_cols, int act_dtype, int fp8_format) {
    if (fp8_format != GPTQHIP_FP8_E4M3FN) return 0;
    if (act_dtype != GPTQHIP_FP16 && act_dtype != GPTQHIP_BF16) return 0;
    return fp8_shape_error(M, K, N, scale_mode, block_rows, block_cols) == nullptr ? 1 : 0;
}

size_t gptqhip_fp8_tiled_bytes(int K, int N) {
    return fp8_shape_error(0, K, N, kScaleTensor, 0, 0) == nullptr ? (size_t)K * N : 0;
}

int gptqhip_fp8_repack(const uint8_t* weight, const float* scale_inv, uint8_t* weight_t, float* rscale, int K, int N, int scale_mode,
                       int block_rows, int block_cols, gptqhip_stream_t stream) {
    const void* req[] = {weight, scale_inv, weight_t, rscale};
    int rc = fp8_check_ptrs("gptqhip_fp8_repack", req, 4, nullptr);
    if (rc) return rc;
    if (const char* why = fp8_shape_error(0, K, N, scale_mode, block_rows, block_cols)) {
        set_error("gptqhip_fp8_repack: %s (K=%d N=%d scale layout %d block %d x %d)", why, K, N, scale_mode, block_rows, block_cols);
        return GPTQHIP_EINVAL;
    }
    if (weight == weight_t || scale_inv == rscale) {
        set_error("gptqhip_fp8_repack: the relayout is not in place");
        return GPTQHIP_EINVAL;
    }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const size_t units = (size_t)K * N / 16, ns = fp8_scale_count(K, N, scale_mode, block_rows, block_cols);
    hipLaunchKernelGGL(fp8_repack_kernel, dim3((unsigned)((units + 255) / 256)), dim3(256), 0, s, weight, weight_t, K, N, K / kChunkK);
    hipLaunchKernelGGL(fp8_rscale_kernel, dim3((unsigned)((ns + 255) / 256)), dim3(256), 0, s, scale_inv, rscale, ns);
    return check_hip(hipGetLastError(), "fp8_repack_kernel launch");
}

int gptqhip_fp8_gemm(const void* x, const uint8_t* weight_t, const float* rscale, const void* bias, void* out, int M, int K, int N,
                     int scale_mode, int block_rows, int block_cols, int act_dtype, int flags, gptqhip_stream_t stream) {
    if (M == 0) return GPTQHIP_OK;   // empty batch: the reference returns an empty tensor
    const void* req[] = {x, weight_t, rscale, out};
    int rc = fp8_check_ptrs("gptqhip_fp8_gemm", req, 4, bias);
    if (rc) return rc;
    if (act_dtype != GPTQHIP_FP16 && act_dtype != GPTQHIP_BF16) {
        set_error("gptqhip_fp8_gemm: unsupported activation dtype tag %d (fp16 = 0, bf16 = 1)", act_dtype);
        return GPTQHIP_EINVAL;
    }
    if (const char* why = fp8_shape_error(M, K, N, scale_mode, block_rows, block_cols)) {
        set_error("gptqhip_fp8_gemm: %s (M=%d K=%d N=%d scale layout %d block %d x %d)", why, M, K, N, scale_mode, block_rows, block_cols);
        return GPTQHIP_EINVAL;
    }
    const int cvt = flags & GPTQHIP_FP8_CVT_MASK;
    if ((flags & ~GPTQHIP_FP8_CVT_MASK) != 0 || (cvt == GPTQHIP_FP8_CVT_BITS && act_dtype != GPTQHIP_FP16)) {
        set_error("gptqhip_fp8_gemm: unsupported flags 0x%x (the bit-placement conversion exists for fp16 activations only)", flags);
        return GPTQHIP_EINVAL;
    }
    const Fp8Params p = fp8_params(x, weight_t, rscale, bias, out, M, K, N, scale_mode, block_rows, block_cols);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (M > kFp8DecodeRows) {
        if (act_dtype == GPTQHIP_FP16) fp8_launch_gemm<kFP16>(p, s);
        else fp8_launch_gemm<kBF16>(p, s);
        return check_hip(hipGetLastError(), "fp8_gemm_kernel launch");
    }
    if (act_dtype == GPTQHIP_FP16) {
        if (cvt == GPTQHIP_FP8_CVT_F32) fp8_launch_decode<kFP16, kCvtF32>(p, s);
        else if (cvt == GPTQHIP_FP8_CVT_BITS) fp8_launch_decode<kFP16, kCvtBits>(p, s);
        else fp8_launch_decode<kFP16, kCvtPacked>(p, s);
    } else {
        if (cvt == GPTQHIP_FP8_CVT_F32) fp8_launch_decode<kBF16, kCvtF32>(p, s);
        else fp8_launch_decode<kBF16, kCvtPacked>(p, s);
    }
    return check_hip(hipGetLastError(), "fp8_decode_kernel launch");
}

int gptqhip_fp8_dequant(const uint8_t* weight_t, const float* rscale, void* out, int K, int N, int scale_mode, int block_rows, int block_cols,
                        int out_dtype, gptqhip_stream_t stream) {
    const void* req[] = {weight_t, rscale, out};
    int rc = fp8_check_ptrs("gptqhip_fp8_dequant", req, 3, nullptr);
    if (rc) return rc;
    if (out_dtype != GPTQHIP_FP16 && out_dtype != GPTQHIP_BF16 && out_dtype != GPTQHIP_FP32) {
        set_error("gptqhip_fp8_dequant: unsupported output dtype tag %d (fp16 = 0, bf16 = 1, fp32 = 2)", out_dtype);
        return GPTQHIP_EINVAL;
    }
    if (const char* why = fp8_shape_error(0, K, N, scale_mode, block_rows, block_cols)) {
        set_error("gptqhip_fp8_dequant: %s (K=%d N=%d scale layout %d block %d x %d)", why, K, N, scale_mode, block_rows, block_cols);
        return GPTQHIP_EINVAL;
    }
    const Fp8Params p = fp8_params(nullptr, weight_t, rscale, nullptr, out, 0, K, N, scale_mode, block_rows, block_cols);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)(((size_t)K * N + 255) / 256)), block(256);
    if (out_dtype == GPTQHIP_FP16) hipLaunchKernelGGL((fp8_dequant_kernel<kFP16>), grid, block, 0, s, p);
    else if (out_dtype == GPTQHIP_BF16) hipLaunchKernelGGL((fp8_dequant_kernel<kBF16>), grid, block, 0, s, p);
    else hipLaunchKernelGGL((fp8_dequant_kernel<2>), grid, block, 0, s, p);
    return check_hip(hipGetLastError(), "fp8_dequant_kernel launch");
}

}  // extern "C"
