"""Measurement tool (not a test): HipMoeExperts' expert-grouped path (moe_align + moe_gate_up_grouped + moe_down_grouped + moe_combine) against
the host-routed loop (what forward() runs beyond 16 tokens without it) and, up to 16 tokens, against the ungrouped fused ops.

    python tests/dev/moe_grouped_probe.py [--out profiles/r08_moe_grouped.txt] [--shapes qwen3,mixtral] [--tokens 1,2,...] [--budget 0.3]

Shapes: Qwen3-30B-A3B (H 2048, I 768, E 128, k 8, g128) and Mixtral-8x7B (H 4096, I 14336, E 8, k 2, g128), fp16, random codes.  Every figure is
event-timed around a window of `budget` seconds (5 .. 200 calls) after warm-up, all variants of one point in the same process back to back.  The
routing rotates through eight random routings per token count (distinct experts per token), copied into the call's input tensors before every
call in every variant, so that successive calls do not find their weights in the 256 MiB Infinity Cache (from 32 tokens on a single call
already touches more expert bytes than the cache holds on both shapes).  The tensors are the ones HF hands the module: int64 ids, fp16 routing
weights.  Algorithmic bytes = distinct experts touched (mean over the routings) x one expert's packed words + constants; the HBM fraction is
those bytes over the graph-replay time against 8 TB/s -- an end-to-end figure of four launches, not a kernel's share of peak."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from gptqmodel_amd.nn_modules.moe import MAX_FAST_TOKENS, HipMoeExperts  # noqa: E402
from gptqmodel_amd.nn_modules.qlinear.hip_gptq import HipGptqLinear  # noqa: E402

SHAPES = {"qwen3": ("Qwen3-30B-A3B", 2048, 768, 128, 8, 128), "mixtral": ("Mixtral-8x7B", 4096, 14336, 8, 2, 128)}
TOKENS = (1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024, 2048)
DEV = "cuda"
HBM_PEAK = 8.0e12
N_ROUTES = 8


def linear(gen, K, N, gs):
    lin = HipGptqLinear(bits=4, group_size=gs, sym=False, desc_act=False, in_features=K, out_features=N, bias=False, register_buffers=False)
    lin.register_buffer("qweight", torch.randint(-2**31, 2**31 - 1, (K // 8, N), generator=gen, device=DEV, dtype=torch.int64).to(torch.int32))
    lin.register_buffer("qzeros", torch.randint(-2**31, 2**31 - 1, (K // gs, N // 8), generator=gen, device=DEV, dtype=torch.int64).to(torch.int32))
    lin.register_buffer("scales", (torch.rand((K // gs, N), generator=gen, device=DEV) * 0.01 + 0.005).half())
    lin.register_buffer("g_idx", (torch.arange(K, device=DEV) // gs).to(torch.int32))
    lin.bias = None
    lin.qzero_format(format=2)
    return lin.eval()


def timed(fn, budget):
    """us per call: warm-up, a three-call estimate, then a window of about `budget` seconds."""
    for i in range(3):
        fn(i)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(3):
        fn(i)
    b.record()
    torch.cuda.synchronize()
    n = int(min(200, max(5, budget * 1e3 / max(a.elapsed_time(b) / 3, 1e-3))))
    a.record()
    for i in range(n):
        fn(i)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / n


def probe(tag, tokens, budget, emit):
    name, H, I, E, k, gs = SHAPES[tag]
    gen = torch.Generator(device=DEV).manual_seed(1234)
    g, u, d = [], [], []
    for _ in range(E):
        g.append(linear(gen, H, I, gs))
        u.append(linear(gen, H, I, gs))
        d.append(linear(gen, I, H, gs))
    m = HipMoeExperts.from_linears(g, u, d)
    del g, u, d
    expert_bytes = 4 * (m.gate_up_qweight.shape[1] + m.gate_up_meta.shape[1] + m.down_qweight.shape[1] + m.down_meta.shape[1])
    emit(f"{name}  H={H} I={I} E={E} top_k={k} g{gs} fp16   expert = {expert_bytes / 1e6:.2f} MB, layer = {E * expert_bytes / 1e6:.0f} MB")
    emit(f"{'T':>5} {'loop us':>10} {'ungrouped us':>13} {'grouped us':>11} {'graph us':>10} {'loop/grp':>9} {'ungr/grp':>9} {'experts':>8} "
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
        t_ungr = timed(call(m), budget) if T <= MAX_FAST_TOKENS else None
        m.grouped_routing, m.grouped_min_tokens, m.grouped_max_tokens = True, 1, 1 << 30
        t_grp = timed(call(m), budget)
        got = m(x, routes[0], w).float()
        diff = float((got - ref).abs().max() / ref.abs().max())
        m.grouped_routing = False
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            graph = torch.cuda.CUDAGraph()
            m.grouped_routing = True
            with torch.cuda.graph(graph, stream=s):
                m(x, ids_in, w)
            m.grouped_routing = False
        torch.cuda.current_stream().wait_stream(s)

        def replay(i):
            ids_in.copy_(routes[i % N_ROUTES])
            graph.replay()
        t_graph = timed(replay, budget)
        m.check_status()
        alg = distinct * expert_bytes
        emit(f"{T:5d} {t_loop:10.1f} {(f'{t_ungr:13.1f}' if t_ungr is not None else ' ' * 12 + '-')} {t_grp:11.1f} {t_graph:10.1f} "
             f"{t_loop / t_grp:9.2f} {(f'{t_ungr / t_grp:9.2f}' if t_ungr is not None else ' ' * 8 + '-')} {distinct:8.1f} {alg / 1e6:8.1f} "
             f"{alg / (t_graph * 1e-6) / HBM_PEAK:9.1%} {diff:21.2e}")
        rows.append((T, t_loop, t_ungr, t_grp, t_graph))
        del graph
        m._grouped_captured.clear()
    emit("")
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default="qwen3,mixtral")
    ap.add_argument("--tokens", default=",".join(str(t) for t in TOKENS))
    ap.add_argument("--budget", type=float, default=0.3)
    args = ap.parse_args()
    tokens = [int(t) for t in args.tokens.split(",")]
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
    emit(f"# tests/dev/moe_grouped_probe.py on {torch.cuda.get_device_name(0)}: expert-grouped MoE path vs the host-routed loop and the ungrouped "
         f"fused ops, event-timed, us per experts call")
    results = {t: probe(t, tokens, args.budget, emit) for t in args.shapes.split(",")}
    # grouped_min_tokens: the smallest T from which grouped eager is not slower than the ungrouped path on every shape (17 when it never is);
    # grouped_max_tokens: the largest measured T at which grouped eager is not slower than the loop on every shape (none: capture-only)
    t_min = MAX_FAST_TOKENS + 1
    for T in sorted((T for T in tokens if T <= MAX_FAST_TOKENS), reverse=True):
        if all(r[3] <= r[2] for rows in results.values() for r in rows if r[0] == T):
            t_min = T
        else:
            break
    ok_max = [T for T in tokens if all(r[3] <= r[1] for rows in results.values() for r in rows if r[0] == T)]
    emit(f"grouped_min_tokens (grouped eager <= ungrouped eager on every shape from here up to 16): {t_min}")
    emit(f"grouped_max_tokens (largest measured T with grouped eager <= loop on every shape): {max(ok_max) if ok_max else 'none (capture-only)'}")
    emit(f"measured T at which the loop is faster than grouped eager on some shape: {[T for T in tokens if T not in ok_max] or 'none'}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
