"""Measurement tool (not a test): HipFp8MoeExperts' expert-grouped path (moe_align + moe_fp8_gate_up_grouped + moe_fp8_down_grouped +
moe_combine) against the two paths forward() runs without it -- the host-routed loop on ops.fp8_gemm (beyond 16 tokens) and the few-token fused
ops (up to 16 tokens).

    python tests/dev/moe_fp8_grouped_probe.py [--out profiles/r14_moe_fp8_grouped.txt] [--shapes qwen3,mixtral] [--layouts b128x128,row]
                                              [--tokens 1,4,16,17,64,256,1024] [--budget 0.1]

Shapes: Qwen3-30B-A3B (H 2048, I 768, E 128, k 8) and Mixtral-8x7B (H 4096, I 14336, E 8, k 2), row and (128, 128) block scales, fp16, random
finite codes.  Every figure is event-timed: warm-up, a three-call estimate, then the MEDIAN of three windows of about `budget` seconds (5 .. 200
calls) each, all variants of one point in the same process back to back.  The routing rotates through eight random routings per token count
(distinct experts per token), copied into the call's input tensors before every call in every variant, so that successive calls do not find
their weights in the 256 MiB Infinity Cache.  The tensors are the ones HF hands the module: int64 ids, fp16 routing weights.  Algorithmic bytes =
distinct experts touched (mean over the routings) x one expert's weight bytes + reciprocal scales, ONCE each; the HBM fraction is those bytes over
the graph-replay time against 8 TB/s -- an end-to-end figure of four launches, not a kernel's share of peak.  Every (unit, column tile) block
re-streams its tile, so the bytes actually moved grow with the number of units: long prefills are expected to lose to the loop."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from gptqmodel_amd.nn_modules.moe_fp8 import MAX_FAST_TOKENS, HipFp8MoeExperts  # noqa: E402
from gptqmodel_amd.nn_modules.qlinear.hip_fp8 import HipFp8Linear  # noqa: E402

SHAPES = {"qwen3": ("Qwen3-30B-A3B", 2048, 768, 128, 8), "mixtral": ("Mixtral-8x7B", 4096, 14336, 8, 2)}
LAYOUTS = {"b128x128": ("block", (128, 128)), "row": ("row", None)}
TOKENS = (1, 4, 16, 17, 64, 256, 1024)
DEV = "cuda"
HBM_PEAK = 8.0e12
N_ROUTES = 8
SPREAD = []      # (max - min) / median of every timing's three windows


def fp8_linear(gen, K, N, method, block):
    b = torch.randint(0, 256, (N, K), generator=gen, device=DEV, dtype=torch.int32).to(torch.uint8)
    b = torch.where((b & 0x7f) == 0x7f, b - 1, b)      # no NaN codes
    shape = (N,) if method == "row" else (N // block[0], K // block[1])
    s = torch.exp(torch.rand(shape, generator=gen, device=DEV) * 5.0 + 5.3)      # scale_inv log-uniform in about [200, 3e4]
    kw = dict(weight_scale_method=method, weight_block_size=block) if method == "block" else dict(weight_scale_method=method)
    lin = HipFp8Linear(bits=8, group_size=-1, sym=True, desc_act=False, in_features=K, out_features=N, bias=False, register_buffers=False, **kw)
    lin.register_buffer("weight", b.view(torch.float8_e4m3fn))
    lin.register_buffer("weight_scale_inv", s)
    lin.bias = None
    return lin.eval()


def timed(fn, budget):
    """us per call: warm-up, a three-call estimate, then the median of three windows of about `budget` seconds (5 .. 200 calls) each."""
    for i in range(3):
        fn(i)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def window(n):
        a.record()
        for i in range(n):
            fn(i)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3 / n
    n = int(min(200, max(5, budget * 1e6 / max(window(3), 1e-3))))
    t = sorted(window(n) for _ in range(3))
    SPREAD.append((t[2] - t[0]) / t[1])
    return t[1]


def probe(tag, layout, tokens, budget, emit):
    name, H, I, E, k = SHAPES[tag]
    method, block = LAYOUTS[layout]
    gen = torch.Generator(device=DEV).manual_seed(1234)
    g, u, d = [], [], []
    for _ in range(E):
        g.append(fp8_linear(gen, H, I, method, block))
        u.append(fp8_linear(gen, H, I, method, block))
        d.append(fp8_linear(gen, I, H, method, block))
    m = HipFp8MoeExperts.from_linears(g, u, d)
    del g, u, d
    torch.cuda.empty_cache()
    expert_bytes = m.gate_up_weight.shape[1] + m.down_weight.shape[1] + 4 * (m.gate_up_rscale[0].numel() + m.down_rscale[0].numel())
    emit(f"{name}  H={H} I={I} E={E} top_k={k} fp8 {layout} fp16   expert = {expert_bytes / 1e6:.2f} MB, layer = {E * expert_bytes / 1e6:.0f} MB")
    emit(f"{'T':>5} {'loop us':>10} {'few-token us':>13} {'grouped us':>11} {'graph us':>10} {'loop/grp':>9} {'few/grp':>9} {'experts':>8} "
         f"{'alg MB':>8} {'HBM frac':>9} {'max rel diff vs loop':>21}")
    rows = []
    for T in tokens:
        x = (torch.randn((T, H), generator=gen, device=DEV) * 0.5).half()
        routes = [torch.rand((T, E), generator=gen, device=DEV).topk(k, dim=-1).indices for _ in range(N_ROUTES)]
        w = torch.softmax(torch.randn((T, k), generator=gen, device=DEV), dim=-1).half()
        distinct = sum(int(r.unique().numel()) for r in routes) / N_ROUTES
        ids_in = routes[0].clone()

        def call(fn):
            def step(i):
                ids_in.copy_(routes[i % N_ROUTES])
                return fn(x, ids_in, w)
            return step

        m.grouped_routing = False
        t_loop = timed(call(m._forward_loop), budget)
        ref = m._forward_loop(x, routes[0], w).float()
        t_few = timed(call(m), budget) if T <= MAX_FAST_TOKENS else None
        m.grouped_routing, m.grouped_min_tokens, m.grouped_max_tokens = True, 1, 1 << 30
        assert m.grouped_path(T, k, torch.float16)
        t_grp = timed(call(m), budget)
        got = m(x, routes[0], w).float()
        diff = float((got - ref).abs().max() / ref.abs().max())
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=s):
                m(x, ids_in, w)
        torch.cuda.current_stream().wait_stream(s)
        m.grouped_routing = False

        def replay(i):
            ids_in.copy_(routes[i % N_ROUTES])
            graph.replay()
        t_graph = timed(replay, budget)
        m.check_status()
        alg = distinct * expert_bytes
        emit(f"{T:5d} {t_loop:10.1f} {(f'{t_few:13.1f}' if t_few is not None else ' ' * 12 + '-')} {t_grp:11.1f} {t_graph:10.1f} "
             f"{t_loop / t_grp:9.2f} {(f'{t_few / t_grp:9.2f}' if t_few is not None else ' ' * 8 + '-')} {distinct:8.1f} {alg / 1e6:8.1f} "
             f"{alg / (t_graph * 1e-6) / HBM_PEAK:9.1%} {diff:21.2e}")
        rows.append((T, t_loop, t_few, t_grp, t_graph))
        del graph
        m._grouped_captured.clear()
    emit("")
    del m
    torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default="qwen3,mixtral")
    ap.add_argument("--layouts", default="b128x128,row")
    ap.add_argument("--tokens", default=",".join(str(t) for t in TOKENS))
    ap.add_argument("--budget", type=float, default=0.1)
    args = ap.parse_args()
    tokens = [int(t) for t in args.tokens.split(",")]
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    def save():
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")
    prop = torch.cuda.get_device_properties(0)
    emit(f"# tests/dev/moe_fp8_grouped_probe.py on {torch.cuda.get_device_name(0)} ({getattr(prop, 'gcnArchName', '?')}, "
         f"{prop.multi_processor_count} CUs, torch {torch.__version__}): expert-grouped FP8 MoE path vs the host-routed loop and the few-token "
         f"fused ops, event-timed (median of three windows), us per experts call")
    results = {}
    for tag in args.shapes.split(","):
        for layout in args.layouts.split(","):
            results[(tag, layout)] = probe(tag, layout, tokens, args.budget, emit)
            save()
    # grouped_min_tokens: the smallest T from which grouped eager is not slower than the few-token ops on every shape (17 when it never is);
    # grouped_max_tokens: the largest measured T at which grouped eager is not slower than the loop on every shape (none: capture-only)
    t_min = MAX_FAST_TOKENS + 1
    for T in sorted((T for T in tokens if T <= MAX_FAST_TOKENS), reverse=True):
        if all(r[3] <= r[2] for rows in results.values() for r in rows if r[0] == T):
            t_min = T
        else:
            break
    ok_max = [T for T in tokens if all(r[3] <= r[1] for rows in results.values() for r in rows if r[0] == T)]
    emit(f"grouped_min_tokens (grouped eager <= few-token eager on every shape and layout from here up to 16): {t_min}")
    emit(f"grouped_max_tokens (largest measured T with grouped eager <= loop on every shape and layout): {max(ok_max) if ok_max else 'none (capture-only)'}")
    emit(f"measured T at which the loop is faster than grouped eager on some shape: {[T for T in tokens if T not in ok_max] or 'none'}")
    emit(f"spread of the three windows of a timing, (max - min) / median: worst {max(SPREAD):.1%}, median {sorted(SPREAD)[len(SPREAD) // 2]:.1%}")
    save()
    return 0


if __name__ == "__main__":
    sys.exit(main())
