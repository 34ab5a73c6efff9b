"""Measurement tool (not a test): HipMoeExperts at T = 1 against the parent behaviour -- the HF-style host-routed loop over the un-fused
HipGptqLinear modules of every expert (one_hot + nonzero() on the routing, three plugin forwards and an index_add_ per active expert).

    python tests/dev/moe_decode_probe.py [--out profiles/r07_moe_decode.txt] [--iters 200] [--shapes qwen3,mixtral]

Shapes: Qwen3-30B-A3B (H 2048, I 768, E 128, k 8, g128) and Mixtral-8x7B (H 4096, I 14336, E 8, k 2, g128), fp16, random codes.  Timing is by
event around warm-up + `iters` iterations; the routing rotates through a fixed list that walks all experts, so successive calls do not find
their weights in the 256 MiB Infinity Cache (Qwen3: 16 routings x 19 MB; Mixtral: 4 routings x 352 MB).  The fused path is timed eager and
graph-replayed (one captured forward, the routing tensor overwritten in place before every replay); the two kernels are also timed alone for
their HBM fractions (algorithmic bytes = top_k experts' packed words + constants, over time, against 8 TB/s)."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from gptqmodel_amd import ops  # noqa: E402
from gptqmodel_amd.nn_modules.moe import HipMoeExperts  # noqa: E402
from gptqmodel_amd.nn_modules.qlinear.hip_gptq import HipGptqLinear  # noqa: E402

SHAPES = {"qwen3": ("Qwen3-30B-A3B", 2048, 768, 128, 8, 128), "mixtral": ("Mixtral-8x7B", 4096, 14336, 8, 2, 128)}
DEV = "cuda"
HBM_PEAK = 8.0e12


def linear_pair(gen, K, N, gs):
    """Two modules holding the same random checkpoint tensors (one for the parent loop, one to be stacked)."""
    qw = torch.randint(-2**31, 2**31 - 1, (K // 8, N), generator=gen, device=DEV, dtype=torch.int64).to(torch.int32)
    qz = torch.randint(-2**31, 2**31 - 1, (K // gs, N // 8), generator=gen, device=DEV, dtype=torch.int64).to(torch.int32)
    sc = (torch.rand((K // gs, N), generator=gen, device=DEV) * 0.01 + 0.005).half()
    out = []
    for _ in range(2):
        lin = HipGptqLinear(bits=4, group_size=gs, sym=False, desc_act=False, in_features=K, out_features=N, bias=False, register_buffers=False)
        lin.register_buffer("qweight", qw.clone())
        lin.register_buffer("qzeros", qz.clone())
        lin.register_buffer("scales", sc.clone())
        lin.register_buffer("g_idx", (torch.arange(K, device=DEV) // gs).to(torch.int32))
        lin.bias = None
        lin.qzero_format(format=2)
        out.append(lin.eval())
    return out


def parent_loop(gate, up, down, x, idx, w, E):
    """What the model ran before: the HF experts loop over per-expert plugin modules (host routing)."""
    final = torch.zeros_like(x)
    mask = torch.nn.functional.one_hot(idx, num_classes=E).permute(2, 1, 0)
    for e in torch.greater(mask.sum(dim=(-1, -2)), 0).nonzero():
        e = int(e[0])
        pos, tok = torch.where(mask[e])
        cur = x[tok]
        h = torch.nn.functional.silu(gate[e](cur)) * up[e](cur)
        final.index_add_(0, tok, (down[e](h) * w[tok, pos, None]).to(final.dtype))
    return final


def timed(fn, n_warm, n_iter):
    for i in range(n_warm):
        fn(i)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(n_iter):
        fn(i)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / n_iter      # us per call


def probe(tag, iters, emit):
    name, H, I, E, k, gs = SHAPES[tag]
    gen = torch.Generator(device=DEV).manual_seed(1234)
    pg, pu, pd, fg, fu, fd = [], [], [], [], [], []
    for _ in range(E):
        for (K, N), plist, flist in (((H, I), pg, fg), ((H, I), pu, fu), ((I, H), pd, fd)):
            a, b = linear_pair(gen, K, N, gs)
            a.post_init()
            plist.append(a)
            flist.append(b)
    fused = HipMoeExperts.from_linears(fg, fu, fd)
    assert fused.fast_path(1, k, torch.float16)
    n_routes = max(1, E // k)
    perm = torch.randperm(E, generator=torch.Generator().manual_seed(7))
    routes64 = [perm[r * k:(r + 1) * k].reshape(1, k).to(DEV) for r in range(n_routes)]
    routes32 = [r.to(torch.int32) for r in routes64]
    x = (torch.randn((1, H), generator=gen, device=DEV) * 0.5).half()
    w = torch.softmax(torch.randn((1, k), generator=gen, device=DEV), dim=-1)
    w16 = w.half()
    ids_in = routes32[0].clone()
    warm = 20

    t_parent = timed(lambda i: parent_loop(pg, pu, pd, x, routes64[i % n_routes], w16, E), warm, iters)

    def eager(i):
        ids_in.copy_(routes32[i % n_routes])
        fused(x, ids_in, w)
    t_eager = timed(eager, warm, iters)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fused(x, ids_in, w)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            fused(x, ids_in, w)
    torch.cuda.current_stream().wait_stream(s)

    def replay(i):
        ids_in.copy_(routes32[i % n_routes])
        g.replay()
    t_graph = timed(replay, warm, iters)

    act = torch.empty((k, I), dtype=torch.float16, device=DEV)
    out = torch.empty((1, H), dtype=torch.float16, device=DEV)
    st = torch.zeros(1, dtype=torch.int32, device=DEV)
    t_gu = timed(lambda i: ops.moe_gate_up(x, fused.gate_up_qweight, fused.gate_up_meta, routes32[i % n_routes], act, st, E, I, gs, torch.float16),
                 warm, iters)
    t_dn = timed(lambda i: ops.moe_down(act, fused.down_qweight, fused.down_meta, routes32[i % n_routes], w, out, st, E, gs, torch.float16),
                 warm, iters)
    fused.check_status()
    b_gu = k * 4 * (fused.gate_up_qweight.shape[1] + fused.gate_up_meta.shape[1])
    b_dn = k * 4 * (fused.down_qweight.shape[1] + fused.down_meta.shape[1])
    emit(f"{name}  H={H} I={I} E={E} top_k={k} g{gs} fp16  T=1  ({iters} iterations after {warm} warm-up, {n_routes} rotating routings)")
    emit(f"  parent loop (un-fused HipGptqLinear modules, host routing)   {t_parent:9.2f} us")
    emit(f"  HipMoeExperts eager                                          {t_eager:9.2f} us   parent / fused = {t_parent / t_eager:6.2f}")
    emit(f"  HipMoeExperts graph replay                                   {t_graph:9.2f} us   parent / fused = {t_parent / t_graph:6.2f}")
    emit(f"  moe_gate_up alone (eager launches back to back)              {t_gu:9.2f} us   {b_gu / 1e6:8.2f} MB  "
         f"{b_gu / (t_gu * 1e-6) / 1e12:5.2f} TB/s = {b_gu / (t_gu * 1e-6) / HBM_PEAK:5.1%} of 8 TB/s")
    emit(f"  moe_down alone (eager launches back to back)                 {t_dn:9.2f} us   {b_dn / 1e6:8.2f} MB  "
         f"{b_dn / (t_dn * 1e-6) / 1e12:5.2f} TB/s = {b_dn / (t_dn * 1e-6) / HBM_PEAK:5.1%} of 8 TB/s")
    emit("")
    return t_parent > t_eager


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--shapes", default="qwen3,mixtral")
    args = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
    emit(f"# tests/dev/moe_decode_probe.py on {torch.cuda.get_device_name(0)}: fused MoE experts vs the per-expert plugin loop, event-timed")
    ok = all([probe(t, max(200, args.iters), emit) for t in args.shapes.split(",")])
    emit("fused eager faster than the parent loop on every shape: " + ("yes" if ok else "NO"))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
