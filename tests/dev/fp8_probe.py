"""Times the FP8 weight-only linear (gptqhip_fp8_gemm) on an MI355X and writes profiles/r09_fp8_linear.txt.

fp16 activations; row and block (128, 128) scales; (K, N) in {4096 x 4096, 4096 x 28672, 14336 x 4096}; M in {1, 16, 512, 4096}.  Per cell:
  (1) fp8     the new op
  (2) ref     the reference's ROCm forward as it stands, restated in plain torch: cast + divide + transpose + matmul per call
              (TorchFP8Linear.dequantize_weight / _forward_dequant_matmul, fp8.py:384-387, 423-425)
  (3) dense   torch.matmul on an fp16 [K, N] weight dequantised once: the 2-bytes-per-weight floor of any dense path
  (4) gptq8   this project's 8-bit GPTQ gptqhip_gemm (group size 128) at the same shape: the same bytes per weight
Event-timed.  Every call of a timed batch reads ANOTHER copy of the weights and the copies add up to more than twice the 256 MiB Infinity
Cache, so no call finds its weights cached.  Reported: the median over batches of (batch time / calls).  For M <= 16 the algorithmic bytes
(weights + scales + x + out) and their fraction of 8 TB/s; for M >= 512 TFLOPS.  Last: the conversion-route A/B of the decode kernel.

    python tests/dev/fp8_probe.py [--out FILE] [--quick]"""
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
LAYOUTS = (("row", None), ("block", (128, 128)))


def timed(calls, batches=5, graph=False):
    """calls: a list of closures, one per weight copy -> median microseconds per call.  graph=True: the batch is captured once and replayed,
    so the host's launch cost (more than a batch-1 kernel's run time) is not what gets measured."""
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


def make_layer(K, N, method, block, copies):
    g = torch.Generator(device=DEV).manual_seed(K + N)
    codes = torch.randint(0, 0x78, (N, K), dtype=torch.uint8, device=DEV, generator=g) | \
        (torch.randint(0, 2, (N, K), dtype=torch.uint8, device=DEV, generator=g) << 7)
    shape = (N,) if method == "row" else (N // block[0], K // block[1])
    scale_inv = torch.rand(shape, device=DEV, generator=g) * 3000.0 + 500.0
    mode = ops.FP8_SCALE_MODES[method]
    w_t, rs = ops.fp8_repack(codes, scale_inv, mode, block)
    layer = {"mode": mode, "block": block, "rs": rs.reshape(-1), "scale_inv": scale_inv,
             "w_t": [w_t] + [w_t.clone() for _ in range(copies - 1)],
             "w_ckpt": [codes.view(torch.float8_e4m3fn)] + [codes.clone().view(torch.float8_e4m3fn) for _ in range(copies - 1)]}
    dense = ops.fp8_dequant(w_t, layer["rs"], K, N, mode, block, out_dtype=torch.float16)
    layer["dense"] = [dense] + [dense.clone() for _ in range(copies - 1)]
    return layer


def make_gptq8(K, N, copies):
    g = torch.Generator(device=DEV).manual_seed(7)
    qweight = torch.randint(-2 ** 31, 2 ** 31 - 1, (K // 4, N), dtype=torch.int32, device=DEV, generator=g)
    qzeros = torch.randint(-2 ** 31, 2 ** 31 - 1, (K // 128, N // 4), dtype=torch.int32, device=DEV, generator=g)
    scales = (torch.rand((K // 128, N), device=DEV, generator=g) * 0.01 + 0.005).to(torch.float16)
    qw_t, meta = ops.repack_tiled(qweight, qzeros, scales, None, 128, 8)
    return [(qw_t, meta)] + [(qw_t.clone(), meta.clone()) for _ in range(copies - 1)]


def ref_forward(x, w_ckpt, scale_inv, method, block):
    w = w_ckpt.to(x.dtype)
    s = scale_inv.to(x.dtype)
    if method == "row":
        s = s.view(-1, 1)
    else:
        s = s.repeat_interleave(block[0], dim=0).repeat_interleave(block[1], dim=1)
    return torch.matmul(x, (w / s).transpose(0, 1).contiguous())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09_fp8_linear.txt"))
    ap.add_argument("--quick", action="store_true", help="first shape only (a smoke run of the probe itself)")
    args = ap.parse_args()
    lines = []

    def emit(s=""):
        print(s, flush=True)
        lines.append(s)

    info = ops.device_info(0)
    emit(f"# FP8 weight-only linear, fp16 activations -- {info['arch']}, {info['cu_count']} CUs, torch {torch.__version__}")
    emit("# us per call, median of 5 batches (M <= 16: the batch captured in a graph and replayed, so host launch cost is excluded); every call of a batch reads another copy of the weights (copies x bytes > 600 MiB)")
    emit("# fp8 = gptqhip_fp8_gemm   ref = cast + divide + transpose + matmul per call   dense = torch.matmul on fp16 weights"
         "   gptq8 = gptqhip_gemm, 8-bit, g128")
    emit(f"{'K':>6} {'N':>6} {'scales':>6} {'M':>5} | {'fp8':>9} {'ref':>10} {'dense':>9} {'gptq8':>9} | {'fp8/dense':>9} {'fp8/gptq8':>9} | "
         f"{'MB':>8} {'GB/s':>7} {'of HBM':>6} | {'TFLOPS fp8':>10} {'ref':>7} {'dense':>7}")
    cvt_rows = []
    for K, N in SHAPES[:1] if args.quick else SHAPES:
        copies = max(2, -(-ROTATE_BYTES // (K * N)))
        gptq8 = make_gptq8(K, N, copies)
        for method, block in LAYOUTS:
            L = make_layer(K, N, method, block, copies)
            for M in ROWS:
                x = (torch.randn((M, K), device=DEV) * 0.5).to(torch.float16)
                n = copies if M <= 16 else min(copies, 6)
                gr = M <= 16
                t_fp8 = timed([lambda i=i: ops.fp8_gemm(x, L["w_t"][i], L["rs"], None, N, L["mode"], block) for i in range(n)], graph=gr)
                t_ref = timed([lambda i=i: ref_forward(x, L["w_ckpt"][i], L["scale_inv"], method, block) for i in range(min(n, 6))], batches=3, graph=gr)
                t_dense = timed([lambda i=i: torch.matmul(x, L["dense"][i]) for i in range(n)], graph=gr)
                t_gptq = timed([lambda i=i: ops.gemm(x, gptq8[i][0], gptq8[i][1], None, None, N, 128, 8, torch.float16) for i in range(n)], graph=gr)
                nbytes = K * N + L["rs"].numel() * 4 + M * K * 2 + M * N * 2
                flops = 2.0 * M * K * N
                if M <= 16:
                    bw = nbytes / (t_fp8 * 1e-6)
                    tail = f"{nbytes / 1e6:8.2f} {bw / 1e9:7.0f} {bw / HBM_BYTES_PER_S:6.2f} | {'':>10} {'':>7} {'':>7}"
                else:
                    tail = (f"{'':>8} {'':>7} {'':>6} | {flops / t_fp8 / 1e6:10.1f} {flops / t_ref / 1e6:7.1f} "
                            f"{flops / t_dense / 1e6:7.1f}")
                emit(f"{K:6d} {N:6d} {method:>6} {M:5d} | {t_fp8:9.1f} {t_ref:10.1f} {t_dense:9.1f} {t_gptq:9.1f} | "
                     f"{t_fp8 / t_dense:9.2f} {t_fp8 / t_gptq:9.2f} | {tail}")
                if M <= 16:
                    row = [f"{K:6d} {N:6d} {method:>6} {M:5d} |"]
                    for cvt in ("packed", "f32", "bits"):
                        t = timed([lambda i=i: ops.fp8_gemm(x, L["w_t"][i], L["rs"], None, N, L["mode"], block, cvt=cvt) for i in range(n)], graph=True)
                        row.append(f"{t:9.1f}")
                    cvt_rows.append(" ".join(row))
            del L
            torch.cuda.empty_cache()
        del gptq8
        torch.cuda.empty_cache()
    emit()
    emit("# conversion routes of the decode kernel, us per call (packed = v_cvt_scalef32_pk_f16_fp8, the default; f32 = v_cvt_pk_f32_fp8 +"
         " v_cvt_pk_f16_f32; bits = perm / shift / and / and-or bit placement, value * 2^-8)")
    emit(f"{'K':>6} {'N':>6} {'scales':>6} {'M':>5} | {'packed':>9} {'f32':>9} {'bits':>9}")
    for r in cvt_rows:
        emit(r)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
