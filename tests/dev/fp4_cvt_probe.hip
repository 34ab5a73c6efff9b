// What do gfx950's packed FP4 converts do?  v_cvt_scalef32_pk_{f16,bf16,f32}_fp4 on every code, with power-of-two and other scales: prints the
// nibble order inside a byte and whether the scale operand's mantissa takes part (gptqhip_fp4.hip, CONVERSION ROUTES, quotes the answer).
//   hipcc --offload-arch=gfx950 -O2 tests/dev/fp4_cvt_probe.hip -o fp4_cvt_probe && ./fp4_cvt_probe
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

typedef _Float16 h2_t __attribute__((ext_vector_type(2)));
typedef __bf16 b2_t __attribute__((ext_vector_type(2)));
typedef float f2_t __attribute__((ext_vector_type(2)));

__global__ void probe(uint32_t word, const float* scales, int ns, float* out) {
    const int s = threadIdx.x;
    if (s >= ns) return;
    const float sc = scales[s];
    float* o = out + s * 24;
    h2_t h[4] = {__builtin_amdgcn_cvt_scalef32_pk_f16_fp4(word, sc, 0), __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(word, sc, 1),
                 __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(word, sc, 2), __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(word, sc, 3)};
    b2_t b[4] = {__builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(word, sc, 0), __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(word, sc, 1),
                 __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(word, sc, 2), __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(word, sc, 3)};
    f2_t f[4] = {__builtin_amdgcn_cvt_scalef32_pk_f32_fp4(word, sc, 0), __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(word, sc, 1),
                 __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(word, sc, 2), __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(word, sc, 3)};
    for (int i = 0; i < 4; ++i) {
        o[2 * i] = (float)h[i].x;
        o[2 * i + 1] = (float)h[i].y;
        o[8 + 2 * i] = (float)b[i].x;
        o[8 + 2 * i + 1] = (float)b[i].y;
        o[16 + 2 * i] = f[i].x;
        o[16 + 2 * i + 1] = f[i].y;
    }
}

#define CHECK(e)                                                            \
    do {                                                                    \
        hipError_t r_ = (e);                                                \
        if (r_ != hipSuccess) {                                             \
            printf("%s: %s\n", #e, hipGetErrorString(r_));                  \
            return 1;                                                       \
        }                                                                   \
    } while (0)

int main() {
    const float scales[] = {1.0f, 2.0f, 0.5f, 1.5f, 1.75f, 0.8125f, 448.0f, 0.001953125f, -1.0f, 0.0f};
    const int ns = sizeof(scales) / sizeof(scales[0]);
    float *ds, *dout, out[ns * 24];
    CHECK(hipMalloc(&ds, sizeof(scales)));
    CHECK(hipMalloc(&dout, sizeof(out)));
    CHECK(hipMemcpy(ds, scales, sizeof(scales), hipMemcpyHostToDevice));
    const uint32_t words[2] = {0x76543210u, 0xfedcba98u};
    const char* names[3] = {"f16 ", "bf16", "f32 "};
    for (int w = 0; w < 2; ++w) {
        hipLaunchKernelGGL(probe, dim3(1), dim3(64), 0, 0, words[w], ds, ns, dout);
        CHECK(hipDeviceSynchronize());
        CHECK(hipMemcpy(out, dout, sizeof(out), hipMemcpyDeviceToHost));
        for (int s = 0; s < ns; ++s)
            for (int t = 0; t < 3; ++t) {
                printf("word %08x scale %-12g %s:", words[w], scales[s], names[t]);
                for (int i = 0; i < 8; ++i) printf(" %g", out[s * 24 + t * 8 + i]);
                printf("\n");
            }
    }
    return 0;
}
