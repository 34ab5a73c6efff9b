"""Times the NVFP4 weight-only linear (gptqhip_fp4_gemm) on an MI355X and writes profiles/r15_fp4_linear.txt.

fp16 activations; (K, N) in {4096 x 4096, 4096 x 28672, 14336 x 4096}; M in {1, 16, 512, 4096}.  Per cell:
  (1) fp4     the new op (4.5 bits per weight)
  (2) dense   torch.matmul on an fp16 [K, N] weight dequantised once: the 2-bytes-per-weight floor of any dense path
  (3) gptq4   this project's 4-bit GPTQ gptqhip_gemm (group size 128) at the same shape (4.25 bits per weight)
  (4) fp8     gptqhip_fp8_gemm with row scales (8 bits per weight)
Event-timed.  Every call of a timed batch reads ANOTHER copy of the weights and the copies of each format add up to more than 600 MiB, over
twice the 256 MiB Infinity Cache, so no call finds its weights cached.  Reported: the median over batches of (batch time / calls).  For
M <= 16 the batch is captured in a graph and replayed (the host's launch cost is not what gets measured) and the algorithmic bytes
(codes + scales + x + out) and their fraction of 8 TB/s are given; for M >= 512 TFLOPS.  Last: the conversion-route A/B, both dtypes.

    python tests/dev/fp4_probe.py [--out FILE] [--quick]"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from gptqmodel_amd import ops  # noqa: E402

DEV = "cuda"
HBM_BYTES_PER_S = 8.0e12
ROTATE_BYTES = 600 << 20
SHAPES = ((4096, 4096), (4096, 28672), (14336, 4096))
ROWS = (1, 16, 512, 4096)


def timed(calls, batches=5, graph=False):
    """calls: a list of closures, one per weight copy -> median microseconds per call.  graph=True: the batch is captured once and replayed."""
    for c in calls[:2]:
        c()
    torch.cuda.synchronize()
    run = None
    if graph:
        try:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                for c in calls:
                    c()
            run = g.replay
            run()
            torch.cuda.synchronize()
        except Exception as e:  # noqa: BLE001 - fall back to eager timing, say so
            print(f"# (graph capture failed, timing eagerly: {type(e).__name__})", flush=True)
            torch.cuda.synchronize()
            run = None
    if run is None:
        def run():
            for c in calls:
                c()
    per_call = []
    for _ in range(batches):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        run()
        stop.record()
        stop.synchronize()
        per_call.append(start.elapsed_time(stop) * 1e3 / len(calls))
    return statistics.median(per_call)


def copies_for(nbytes):
    return max(2, -(-ROTATE_BYTES // nbytes))


def clones(t, n):
    return [t] + [t.clone() for _ in range(n - 1)]


def make_fp4(K, N):
    g = torch.Generator(device=DEV).manual_seed(K + N)
    packed = torch.randint(0, 256, (N, K // 2), dtype=torch.uint8, device=DEV, generator=g)
    scale = torch.randint(0x20, 0x50, (N, K // 16), dtype=torch.uint8, device=DEV, generator=g)      # 2^-3 .. 7.5
    w_t, s_t = ops.fp4_repack(packed, scale.view(torch.float8_e4m3fn))
    s2 = torch.tensor([3.17e-4], dtype=torch.float32, device=DEV)
    n = copies_for(K * N // 2)
    dense = ops.fp4_dequant(w_t, s_t, s2, K, N, out_dtype=torch.float16)
    return {"w_t": clones(w_t, n), "s_t": clones(s_t, n), "s2": s2, "dense": clones(dense, copies_for(K * N * 2))}


def make_gptq4(K, N):
    g = torch.Generator(device=DEV).manual_seed(7)
    qweight = torch.randint(-2 ** 31, 2 ** 31 - 1, (K // 8, N), dtype=torch.int32, device=DEV, generator=g)
    qzeros = torch.randint(-2 ** 31, 2 ** 31 - 1, (K // 128, N // 8), dtype=torch.int32, device=DEV, generator=g)
    scales = (torch.rand((K // 128, N), device=DEV, generator=g) * 0.01 + 0.005).to(torch.float16)
    qw_t, meta = ops.repack_tiled(qweight, qzeros, scales, None, 128, 4)
    n = copies_for(K * N // 2)
    return [(qw_t, meta)] + [(qw_t.clone(), meta.clone()) for _ in range(n - 1)]


def make_fp8(K, N):
    g = torch.Generator(device=DEV).manual_seed(9)
    codes = torch.randint(0, 0x78, (N, K), dtype=torch.uint8, device=DEV, generator=g)
    scale_inv = torch.rand((N,), device=DEV, generator=g) * 3000.0 + 500.0
    w_t, rs = ops.fp8_repack(codes, scale_inv, ops.FP8_SCALE_ROW, None)
    return {"w_t": clones(w_t, copies_for(K * N)), "rs": rs.reshape(-1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_fp4_linear.txt"))
    ap.add_argument("--quick", action="store_true", help="first shape only (a smoke run of the probe itself)")
    args = ap.parse_args()
    lines = []

    def emit(s=""):
        print(s, flush=True)
        lines.append(s)

    info = ops.device_info(0)
    emit(f"# NVFP4 weight-only linear, fp16 activations -- {info['arch']}, {info['cu_count']} CUs, torch {torch.__version__}")
    emit("# us per call, median of 5 batches (M <= 16: the batch captured in a graph and replayed, so host launch cost is excluded); every call "
         "of a batch reads another copy of the weights (copies x bytes > 600 MiB per format)")
    emit("# fp4 = gptqhip_fp4_gemm   dense = torch.matmul on fp16 weights   gptq4 = gptqhip_gemm, 4-bit, g128   fp8 = gptqhip_fp8_gemm, row scales")
    emit(f"{'K':>6} {'N':>6} {'M':>5} | {'fp4':>9} {'dense':>9} {'gptq4':>9} {'fp8':>9} | {'fp4/dense':>9} {'fp4/gptq4':>9} {'fp4/fp8':>8} | "
         f"{'MB':>8} {'GB/s':>7} {'of HBM':>6} | {'TFLOPS fp4':>10} {'dense':>7} {'gptq4':>7} {'fp8':>7}")
    cvt_rows = []
    for K, N in SHAPES[:1] if args.quick else SHAPES:
        L, G, E = make_fp4(K, N), make_gptq4(K, N), make_fp8(K, N)
        for M in ROWS:
            x = (torch.randn((M, K), device=DEV) * 0.5).to(torch.float16)
            gr = M <= 16
            cap = (lambda v: len(v)) if gr else (lambda v: min(len(v), 6))
            t_fp4 = timed([lambda i=i: ops.fp4_gemm(x, L["w_t"][i], L["s_t"][i], L["s2"], None, N) for i in range(cap(L["w_t"]))], graph=gr)
            t_dense = timed([lambda i=i: torch.matmul(x, L["dense"][i]) for i in range(cap(L["dense"]))], graph=gr)
            t_gptq = timed([lambda i=i: ops.gemm(x, G[i][0], G[i][1], None, None, N, 128, 4, torch.float16) for i in range(cap(G))], graph=gr)
            t_fp8 = timed([lambda i=i: ops.fp8_gemm(x, E["w_t"][i], E["rs"], None, N, ops.FP8_SCALE_ROW, None) for i in range(cap(E["w_t"]))],
                          graph=gr)
            nbytes = K * N // 2 + K * N // 16 + 4 + M * K * 2 + M * N * 2
            flops = 2.0 * M * K * N
            if M <= 16:
                bw = nbytes / (t_fp4 * 1e-6)
                tail = f"{nbytes / 1e6:8.2f} {bw / 1e9:7.0f} {bw / HBM_BYTES_PER_S:6.2f} | {'':>10} {'':>7} {'':>7} {'':>7}"
            else:
                tail = (f"{'':>8} {'':>7} {'':>6} | {flops / t_fp4 / 1e6:10.1f} {flops / t_dense / 1e6:7.1f} {flops / t_gptq / 1e6:7.1f} "
                        f"{flops / t_fp8 / 1e6:7.1f}")
            emit(f"{K:6d} {N:6d} {M:5d} | {t_fp4:9.1f} {t_dense:9.1f} {t_gptq:9.1f} {t_fp8:9.1f} | {t_fp4 / t_dense:9.2f} {t_fp4 / t_gptq:9.2f} "
                 f"{t_fp4 / t_fp8:8.2f} | {tail}")
            if M <= 512:
                row = [f"{K:6d} {N:6d} {M:5d} |"]
                for dt in (torch.float16, torch.bfloat16):
                    xd = x.to(dt)
                    for cvt in ("packed", "f32"):
                        t = timed([lambda i=i: ops.fp4_gemm(xd, L["w_t"][i], L["s_t"][i], L["s2"], None, N, cvt=cvt)
                                   for i in range(cap(L["w_t"]))], graph=gr)
                        row.append(f"{t:11.1f}")
                cvt_rows.append(" ".join(row))
        del L, G, E
        torch.cuda.empty_cache()
    emit()
    emit("# conversion routes, us per call (packed = v_cvt_scalef32_pk_{f16,bf16}_fp4 + a packed multiply by the block scale: v_pk_mul_f16, or "
         "widen / v_pk_mul_f32 / v_cvt_pk_bf16_f32 for bf16;  f32 = v_cvt_scalef32_pk_f32_fp4 + v_pk_mul_f32 + v_cvt_pk_{f16,bf16}_f32)")
    emit(f"{'K':>6} {'N':>6} {'M':>5} | {'fp16 packed':>11} {'fp16 f32':>11} {'bf16 packed':>11} {'bf16 f32':>11}")
    for r in cvt_rows:
        emit(r)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
