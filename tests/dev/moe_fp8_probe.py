"""Measurement tool (not a test): HipFp8MoeExperts at T = 1 and T = 16 against the parent behaviour -- the HF-style host-routed loop over the
un-fused HipFp8Linear modules of every expert (one_hot + nonzero() on the routing, three plugin forwards and an index_add_ per active expert)
-- and, for scale, the int4 fused ops of HipMoeExperts on the same shapes.

    python tests/dev/moe_fp8_probe.py [--out profiles/r10_moe_fp8.txt] [--iters 200] [--shapes qwen3,mixtral] [--layouts b128x128,row]

Shapes: Qwen3-30B-A3B (H 2048, I 768, E 128, k 8) and Mixtral-8x7B (H 4096, I 14336, E 8, k 2), fp16, random finite codes.  Timing is by event:
warm-up, then the median of three windows of at least `iters` iterations and about 0.2 s each; the routing rotates through a fixed list that
walks all experts, so successive calls do not find their weights in the 256 MiB Infinity Cache.  The fused path is timed eager and graph-replayed (one captured forward, the routing tensor overwritten
in place before every replay); the two kernels are also timed alone for their HBM fractions (algorithmic bytes = the DISTINCT routed experts'
weights + reciprocal scales, once each, over time, against 8 TB/s)."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from gptqmodel_amd import ops  # noqa: E402
from gptqmodel_amd.nn_modules.moe import HipMoeExperts  # noqa: E402
from gptqmodel_amd.nn_modules.moe_fp8 import HipFp8MoeExperts  # noqa: E402
from gptqmodel_amd.nn_modules.qlinear.hip_fp8 import HipFp8Linear  # noqa: E402
from gptqmodel_amd.nn_modules.qlinear.hip_gptq import HipGptqLinear  # noqa: E402

SHAPES = {"qwen3": ("Qwen3-30B-A3B", 2048, 768, 128, 8), "mixtral": ("Mixtral-8x7B", 4096, 14336, 8, 2)}
LAYOUTS = {"b128x128": ("block", (128, 128)), "row": ("row", None)}
TOKENS = (1, 16)
DEV = "cuda"
HBM_PEAK = 8.0e12
GS = 128


def fp8_pair(gen, K, N, method, block):
    """Two modules holding the same random checkpoint tensors (one for the parent loop, one to be stacked)."""
    b = torch.randint(0, 256, (N, K), generator=gen, device=DEV, dtype=torch.int32).to(torch.uint8)
    b = torch.where((b & 0x7f) == 0x7f, b - 1, b)      # no NaN codes
    shape = (N,) if method == "row" else (N // block[0], K // block[1])
    s = torch.exp(torch.rand(shape, generator=gen, device=DEV) * 5.0 + 5.3)      # scale_inv log-uniform in about [200, 3e4]
    kw = dict(weight_scale_method=method, weight_block_size=block) if method == "block" else dict(weight_scale_method=method)
    out = []
    for _ in range(2):
        lin = HipFp8Linear(bits=8, group_size=-1, sym=True, desc_act=False, in_features=K, out_features=N, bias=False, register_buffers=False, **kw)
        lin.register_buffer("weight", b.clone().view(torch.float8_e4m3fn))
        lin.register_buffer("weight_scale_inv", s.clone())
        lin.bias = None
        out.append(lin.eval())
    return out


def gptq_linear(gen, K, N):
    qw = torch.randint(-2**31, 2**31 - 1, (K // 8, N), generator=gen, device=DEV, dtype=torch.int64).to(torch.int32)
    qz = torch.randint(-2**31, 2**31 - 1, (K // GS, N // 8), generator=gen, device=DEV, dtype=torch.int64).to(torch.int32)
    lin = HipGptqLinear(bits=4, group_size=GS, sym=False, desc_act=False, in_features=K, out_features=N, bias=False, register_buffers=False)
    lin.register_buffer("qweight", qw)
    lin.register_buffer("qzeros", qz)
    lin.register_buffer("scales", (torch.rand((K // GS, N), generator=gen, device=DEV) * 0.01 + 0.005).half())
    lin.register_buffer("g_idx", (torch.arange(K, device=DEV) // GS).to(torch.int32))
    lin.bias = None
    lin.qzero_format(format=2)
    return lin.eval()


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


SPREAD = []      # (max - min) / median of every timing's three windows


def timed(fn, n_warm, n_iter):
    """us per call: the median of three event-timed windows of at least `n_iter` calls and about 0.2 s each, after warm-up."""
    for i in range(n_warm):
        fn(i)
    torch.cuda.synchronize()

    def window(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for i in range(n):
            fn(i)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3 / n
    pilot = window(20)
    n = int(min(max(n_iter, 2.0e5 / max(pilot, 1e-3)), 20000))
    t = sorted(window(n) for _ in range(3))
    SPREAD.append((t[2] - t[0]) / t[1])
    return t[1]


def make_routes(E, k, T):
    """Routings that walk all experts: token t of routing r takes k consecutive entries of a fixed permutation (distinct experts per token)."""
    perm = torch.randperm(E, generator=torch.Generator().manual_seed(7))
    n_routes = max(1, E // k)
    routes = []
    for r in range(n_routes):
        rows = [perm[(torch.arange(k) + ((r * T + t) * k)) % E] for t in range(T)]
        routes.append(torch.stack(rows).to(DEV))
    return routes


def hbm(b, t_us):
    return f"{b / 1e6:8.2f} MB  {b / (t_us * 1e-6) / 1e12:5.2f} TB/s = {b / (t_us * 1e-6) / HBM_PEAK:5.1%} of 8 TB/s"


def probe_int4(tag, iters, emit):
    """The int4 fused ops of the same shapes, each kernel alone: {T: (gate_up us, down us)}."""
    name, H, I, E, k = SHAPES[tag]
    gen = torch.Generator(device=DEV).manual_seed(99)
    lists = ([gptq_linear(gen, H, I) for _ in range(E)], [gptq_linear(gen, H, I) for _ in range(E)], [gptq_linear(gen, I, H) for _ in range(E)])
    fused = HipMoeExperts.from_linears(*lists)
    res = {}
    for T in TOKENS:
        routes32 = [r.to(torch.int32) for r in make_routes(E, k, T)]
        n = len(routes32)
        x = (torch.randn((T, H), generator=gen, device=DEV) * 0.5).half()
        w = torch.softmax(torch.randn((T, k), generator=gen, device=DEV), dim=-1)
        act = torch.empty((T * k, I), dtype=torch.float16, device=DEV)
        out = torch.empty((T, H), dtype=torch.float16, device=DEV)
        st = torch.zeros(1, dtype=torch.int32, device=DEV)
        t_gu = timed(lambda i: ops.moe_gate_up(x, fused.gate_up_qweight, fused.gate_up_meta, routes32[i % n], act, st, E, I, GS, torch.float16), 20, iters)
        t_dn = timed(lambda i: ops.moe_down(act, fused.down_qweight, fused.down_meta, routes32[i % n], w, out, st, E, GS, torch.float16), 20, iters)
        res[T] = (t_gu, t_dn)
        emit(f"{name} int4 g128 fused ops, T={T}: moe_gate_up {t_gu:9.2f} us, moe_down {t_dn:9.2f} us, sum {t_gu + t_dn:9.2f} us")
    del fused, lists
    torch.cuda.empty_cache()
    return res


def probe(tag, layout, iters, int4, emit):
    name, H, I, E, k = SHAPES[tag]
    method, block = LAYOUTS[layout]
    gen = torch.Generator(device=DEV).manual_seed(1234)
    pg, pu, pd, fg, fu, fd = [], [], [], [], [], []
    for _ in range(E):
        for (K, N), plist, flist in (((H, I), pg, fg), ((H, I), pu, fu), ((I, H), pd, fd)):
            a, b = fp8_pair(gen, K, N, method, block)
            a.post_init()
            plist.append(a)
            flist.append(b)
    fused = HipFp8MoeExperts.from_linears(fg, fu, fd)
    per_expert_gu = fused.gate_up_weight.shape[1] + 4 * fused.gate_up_rscale[0].numel()
    per_expert_dn = fused.down_weight.shape[1] + 4 * fused.down_rscale[0].numel()
    warm, faster = 20, True
    for T in TOKENS:
        assert fused.fast_path(T, k, torch.float16)
        routes64 = make_routes(E, k, T)
        routes32 = [r.to(torch.int32) for r in routes64]
        n = len(routes64)
        distinct = sum(int(r.unique().numel()) for r in routes64) / n
        x = (torch.randn((T, H), generator=gen, device=DEV) * 0.5).half()
        w = torch.softmax(torch.randn((T, k), generator=gen, device=DEV), dim=-1)
        w16 = w.half()
        ids_in = routes32[0].clone()

        t_parent = timed(lambda i: parent_loop(pg, pu, pd, x, routes64[i % n], w16, E), warm, iters)

        def eager(i):
            ids_in.copy_(routes32[i % n])
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
            ids_in.copy_(routes32[i % n])
            g.replay()
        t_graph = timed(replay, warm, iters)

        act = torch.empty((T * k, I), dtype=torch.float16, device=DEV)
        out = torch.empty((T, H), dtype=torch.float16, device=DEV)
        st = torch.zeros(1, dtype=torch.int32, device=DEV)
        mode, blk = fused._down_mode()
        t_gu = timed(lambda i: ops.moe_fp8_gate_up(x, fused.gate_up_weight, fused.gate_up_rscale, routes32[i % n], act, st, E, I,
                                                   fused.gate_up_block_cols), warm, iters)
        t_dn = timed(lambda i: ops.moe_fp8_down(act, fused.down_weight, fused.down_rscale, routes32[i % n], w, out, st, E, mode, blk), warm, iters)
        fused.check_status()
        i_gu, i_dn = int4[T]
        emit(f"{name}  H={H} I={I} E={E} top_k={k} fp8 {layout} fp16  T={T}  (3 windows of >= {iters} iterations after {warm} warm-up, {n} rotating routings, "
             f"{distinct:.1f} distinct experts per call)")
        emit(f"  parent loop (un-fused HipFp8Linear modules, host routing)    {t_parent:9.2f} us")
        emit(f"  HipFp8MoeExperts eager                                       {t_eager:9.2f} us   parent / fused = {t_parent / t_eager:6.2f}")
        emit(f"  HipFp8MoeExperts graph replay                                {t_graph:9.2f} us   parent / fused = {t_parent / t_graph:6.2f}")
        emit(f"  moe_fp8_gate_up alone (eager launches back to back)          {t_gu:9.2f} us   {hbm(distinct * per_expert_gu, t_gu)}")
        emit(f"  moe_fp8_down alone (eager launches back to back)             {t_dn:9.2f} us   {hbm(distinct * per_expert_dn, t_dn)}")
        emit(f"  int4 ops of the same shape: gate_up {i_gu:9.2f} us, down {i_dn:9.2f} us   fp8 / int4 = {t_gu / i_gu:5.2f} (gate_up) {t_dn / i_dn:5.2f} (down) "
             f"{(t_gu + t_dn) / (i_gu + i_dn):5.2f} (sum)")
        emit("")
        faster = faster and t_parent > t_eager
        del g
    del fused, pg, pu, pd
    torch.cuda.empty_cache()
    return faster


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--shapes", default="qwen3,mixtral")
    ap.add_argument("--layouts", default="b128x128,row")
    args = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
    prop = torch.cuda.get_device_properties(0)
    emit(f"# tests/dev/moe_fp8_probe.py on {torch.cuda.get_device_name(0)} ({getattr(prop, 'gcnArchName', '?')}, {prop.multi_processor_count} CUs, "
         f"torch {torch.__version__}): fused FP8 MoE experts vs the per-expert plugin loop, event-timed")
    ok = True
    for tag in args.shapes.split(","):
        int4 = probe_int4(tag, args.iters, emit)
        emit("")
        for layout in args.layouts.split(","):
            ok = probe(tag, layout, args.iters, int4, emit) and ok
    emit(f"spread of the three windows of a timing, (max - min) / median: worst {max(SPREAD):.1%}, median {sorted(SPREAD)[len(SPREAD) // 2]:.1%}")
    emit("fused eager faster than the parent loop on every point: " + ("yes" if ok else "NO"))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
