"""Fused FP8 MoE experts on the GPU: gptqhip_moe_fp8_gate_up / gptqhip_moe_fp8_down, HipFp8MoeExperts and fuse_moe_experts against the oracle of
tests/moe_fp8_oracle.py.

Bars, all from the project.  Stage one repeats the stated chain (each projection rounded once, silu rounded, the product rounded) up to the fp32
summation order: helpers.NORM_TOL against act_model, the stage-one bar of tests/test_gpu_moe.py.  Stage two sums the top_k expert outputs once in
fp32 and rounds once, which is NOT the reference's chain, so it -- fed act_model, both stages from x, the module, and the host-routed slow path
-- is held to float64 arithmetic with the bar of tests/test_gpu_moe.py / tests/test_gpu_fp8.py:
    rel64(got, y64) <= max(rel64(chain, y64), rel64(y_once, y64)) + 1e-4
tests/test_moe_fp8_cpu.py shows on the CPU that a float32 model of the contract fits that bar on every case here."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import fp8_oracle as F
import moe_fp8_oracle as MF
import moe_oracle as MO
from helpers import NORM_TOL, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
TDT = F.TORCH_DT
ACTS = ("fp16", "bf16")
_FUSED = {}


def dev(a, act=None):
    t = torch.from_numpy(np.array(a))     # (the oracle's arrays are read-only)
    return t.to(device=DEV, dtype=TDT[act]) if act else t.to(DEV)


def host(t):
    return t.detach().to("cpu", torch.float64).numpy()


def _linear(codes, scale_inv, method, block, name, bias=False):
    from gptqmodel_amd.nn_modules.qlinear.hip_fp8 import HipFp8Linear
    N, K = codes.shape
    kw = dict(weight_scale_method=method, weight_block_size=block) if method == "block" else dict(weight_scale_method=method)
    lin = HipFp8Linear(bits=8, group_size=-1, sym=True, desc_act=False, in_features=K, out_features=N, bias=bias, name=name, **kw)
    lin.weight.data = torch.from_numpy(np.array(codes)).view(torch.float8_e4m3fn)
    lin.weight_scale_inv.data = torch.from_numpy(np.array(scale_inv))
    return lin.to(DEV).eval()


def expert_linears(shape, layout, hi=6.0e4):
    """Fresh checkpoint-layout modules of every expert: ([gate], [up], [down])."""
    ex = MF.experts_of(shape, layout, hi)
    return tuple([_linear(*ex[e][name], *MF.proj_layout(layout, name), f"e{e}.{name}") for e in range(len(ex))] for name in MF.PROJ)


def fused_experts(shape, layout, hi=6.0e4):
    from gptqmodel_amd.nn_modules.moe_fp8 import HipFp8MoeExperts
    key = (shape, layout, hi)
    if key not in _FUSED:
        _FUSED[key] = HipFp8MoeExperts.from_linears(*expert_linears(shape, layout, hi))
    return _FUSED[key]


def stage_one(m, x, ids):
    from gptqmodel_amd import ops
    T, k = ids.shape
    a = torch.empty((T * k, m.intermediate_dim), dtype=x.dtype, device=DEV)
    st = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.moe_fp8_gate_up(x, m.gate_up_weight, m.gate_up_rscale, ids, a, st, m.num_experts, m.intermediate_dim, m.gate_up_block_cols)
    return a, st


def stage_two(m, a, ids, rw):
    from gptqmodel_amd import ops
    out = torch.empty((ids.shape[0], m.hidden_dim), dtype=a.dtype, device=DEV)
    st = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.moe_fp8_down(a, m.down_weight, m.down_rscale, ids, rw, out, st, m.num_experts, *m._down_mode())
    return out, st


def run_ops(m, x, ids, rw):
    """The two ops on a module's stacked buffers: (stage one [T k, I], output [T, H], status)."""
    a, st1 = stage_one(m, x, ids)
    y, st2 = stage_two(m, a, ids, rw)
    return a, y, int(st1.item()) | int(st2.item())


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("T", MF.TOKENS)
@pytest.mark.parametrize("shape,layout", MF.CASES)
def test_stages_and_module_against_the_oracle(shape, layout, T, act):
    c = MF.case(shape, layout, T, act)
    m = fused_experts(shape, layout)
    assert m.fast_path(T, c["ids"].shape[1], TDT[act])
    x, ids, rw = dev(c["x"], act), dev(c["ids"]), dev(c["rw"])
    a, y, st = run_ops(m, x, ids, rw)
    e1 = rel_err(host(a), c["act_model"])                                   # stage one: the stated chain up to the fp32 summation order
    y2, st2 = stage_two(m, dev(c["act_model"], act), ids, rw)               # stage two, fed act_model
    e2 = F.rel64(host(y2), c["y64"])
    e3 = F.rel64(host(y), c["y64"])                                         # both stages from x
    ym = m(x, ids.long(), rw.to(TDT[act]))                                  # the module, with the tensors HF hands it
    e4 = F.rel64(host(ym), c["y64"])
    b = MF.bar(c)
    print(f"{shape} {layout} T={T} {act}: stage1 {e1:.3e} (bar {NORM_TOL[act]:.0e}); stage2 {e2:.3e}, both {e3:.3e}, module {e4:.3e} "
          f"(bar {b:.3e}: chain {F.rel64(c['chain'], c['y64']):.3e}, one rounding {F.rel64(c['y_once'], c['y64']):.3e})")
    assert st == 0 and int(st2.item()) == 0
    m.check_status()
    assert e1 <= NORM_TOL[act], e1
    assert e2 <= b, (e2, b)
    assert e3 <= b, (e3, b)
    assert e4 <= b, (e4, b)
    assert torch.equal(ym, y)


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("T", MF.DEEP_TOKENS)
@pytest.mark.parametrize("shape,layout", MF.DEEP_CASES)
def test_deep_k_and_wide_top_k_against_the_oracle(shape, layout, T, act):
    """Waves whose contiguous range is several chunks long (rounds of kMoeAhead loads with a ragged last one, K blocks of 2 and 3 chunks that a
    wave boundary cuts) and top_k 7, 8 and 16 -- what each case reaches: tests/test_moe_wave_model_cpu.py.  The assertions and bars of
    test_stages_and_module_against_the_oracle."""
    c = MF.case(shape, layout, T, act)
    m = fused_experts(shape, layout)
    assert m.fast_path(T, c["ids"].shape[1], TDT[act])
    x, ids, rw = dev(c["x"], act), dev(c["ids"]), dev(c["rw"])
    a, y, st = run_ops(m, x, ids, rw)
    e1 = rel_err(host(a), c["act_model"])
    y2, st2 = stage_two(m, dev(c["act_model"], act), ids, rw)
    e2 = F.rel64(host(y2), c["y64"])
    e3 = F.rel64(host(y), c["y64"])
    ym = m(x, ids.long(), rw.to(TDT[act]))
    e4 = F.rel64(host(ym), c["y64"])
    b = MF.bar(c)
    print(f"deep {shape} {layout} T={T} {act}: stage1 {e1:.3e} (bar {NORM_TOL[act]:.0e}); stage2 {e2:.3e}, both {e3:.3e}, module {e4:.3e} "
          f"(bar {b:.3e}: chain {F.rel64(c['chain'], c['y64']):.3e}, one rounding {F.rel64(c['y_once'], c['y64']):.3e})")
    assert st == 0 and int(st2.item()) == 0
    m.check_status()
    assert e1 <= NORM_TOL[act], e1
    assert e2 <= b, (e2, b)
    assert e3 <= b, (e3, b)
    assert e4 <= b, (e4, b)
    assert torch.equal(ym, y)


@pytest.mark.parametrize("shape,layout", MF.CASES + MF.DEEP_CASES)
def test_stacked_layout_is_the_interleaved_kernel_weights(shape, layout):
    """Independent of the MoE kernels: gptqhip_fp8_dequant on expert e's view of each stacked buffer = the oracle's kernel weights, bit for bit."""
    from gptqmodel_amd import ops
    m = fused_experts(shape, layout)
    H, I, E, _ = MF._ALL_SHAPES[shape]
    ex = MF.experts_of(shape, layout)
    gu_block, d_block = MF.proj_layout(layout, "gate")[1], MF.proj_layout(layout, "down")[1]
    assert tuple(m.gate_up_weight.shape) == (E, 2 * I * H) and tuple(m.down_weight.shape) == (E, I * H)
    assert m.gate_up_rscale.shape[:2] == (E, 2 * I) and m.down_rscale.shape[0] == E
    for e in range(E):
        w, rs, mode, block, K, N = m.expert_view(e, "gate_up")
        assert w.data_ptr() % 16 == 0 and rs.data_ptr() % 16 == 0
        got = ops.fp8_dequant(w, rs, K, N, mode, block, torch.float32).cpu().numpy()
        want = MF.fused_rows(F.kernel_w(*ex[e]["gate"], gu_block), F.kernel_w(*ex[e]["up"], gu_block)).T
        assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(want).view(np.uint32)), ("gate_up", e)
        w, rs, mode, block, K, N = m.expert_view(e, "down")
        got = ops.fp8_dequant(w, rs, K, N, mode, block, torch.float32).cpu().numpy()
        want = F.kernel_w(*ex[e]["down"], d_block).T
        assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(want).view(np.uint32)), ("down", e)


@pytest.mark.parametrize("layout", ["tensor", "row", "b128x128"])
def test_post_initialised_modules_stack_to_the_same_buffers(layout):
    from gptqmodel_amd.nn_modules.moe_fp8 import HipFp8MoeExperts
    shape = "384x640e5k3"
    gate, up, down = expert_linears(shape, layout)
    for lin in gate + up + down:
        lin.post_init()
    m2, m = HipFp8MoeExperts.from_linears(gate, up, down), fused_experts(shape, layout)
    for name in ("gate_up_weight", "gate_up_rscale", "down_weight", "down_rscale"):
        assert torch.equal(getattr(m2, name), getattr(m, name)), name
    assert all(lin.weight.numel() == 0 and lin.rscale.numel() == 0 and not lin._ready for lin in gate + up + down)      # released


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("layout", ["row", "b128x128"])
def test_routing_corners(layout, act):
    shape = "384x640e5k3"
    H, I, E, k = MF.SHAPES[shape]
    m = fused_experts(shape, layout)
    x = MO.make_x(77, 4, H, act).astype(np.float64)
    _, rw = MO.make_routing(78, 4, E, k, act)
    # token 0: all slots on one expert; tokens 1 and 2 share expert 3 (in different slots); token 3: ids 0 and E - 1 together
    ids = np.array([[2, 2, 2], [3, 1, 0], [4, 3, 1], [0, E - 1, 2]], np.int32)
    ref = MF.evaluate(MF.experts_of(shape, layout), MF.weights64_of(shape, layout), layout, x, ids, rw, act)
    a, y, st = run_ops(m, dev(x, act), dev(ids), dev(rw))
    e1, e3 = rel_err(host(a), ref["act_model"]), F.rel64(host(y), ref["y64"])
    print(f"corners {layout} {act}: stage1 {e1:.3e}, both {e3:.3e} (bar {MF.bar(ref):.3e})")
    assert st == 0 and e1 <= NORM_TOL[act] and e3 <= MF.bar(ref)
    # run-to-run bit equality (no atomics, fixed summation order)
    a_b, y_b, _ = run_ops(m, dev(x, act), dev(ids), dev(rw))
    assert torch.equal(a, a_b) and torch.equal(y, y_b)
    # a zero routing weight contributes exactly nothing: swap that slot's expert for any other, the output keeps its bits
    rw0 = rw.copy()
    rw0[:, 1] = 0.0
    base = run_ops(m, dev(x, act), dev(ids), dev(rw0))[1]
    for other in range(E):
        ids2 = ids.copy()
        ids2[:, 1] = other
        assert torch.equal(run_ops(m, dev(x, act), dev(ids2), dev(rw0))[1], base), other


@pytest.mark.parametrize("layout", ["tensor", "b128x128"])
def test_out_of_range_ids_set_status_and_contribute_zero(layout):
    """Ids -1 and E dereference nothing by construction (the kernels test the id before forming any address from it)."""
    shape, act = "256x128e8k2", "fp16"
    H, I, E, k = MF.SHAPES[shape]
    m = fused_experts(shape, layout)
    c = MF.case(shape, layout, 5, act)
    x, rw = dev(c["x"], act), dev(c["rw"])
    _, clean, st = run_ops(m, x, dev(c["ids"]), rw)
    assert st == 0
    bad = c["ids"].copy()
    bad[1, 0], bad[3, 1] = -1, E
    a, y, st = run_ops(m, x, dev(bad), rw)
    assert st == 1
    keep = [0, 2, 4]
    assert torch.equal(y[keep], clean[keep])                       # the other tokens: bit-identical to the clean run
    assert not a[1 * k + 0].any() and not a[3 * k + 1].any()       # the bad slots' stage-one rows are zeros
    # ... and the bad slot contributes exactly zero: the token's output has the bits of a call with its remaining slot alone
    for t, j_ok in ((1, 1), (3, 0)):
        solo = run_ops(m, x[t:t + 1], dev(c["ids"][t:t + 1, j_ok:j_ok + 1]), dev(c["rw"][t:t + 1, j_ok:j_ok + 1]))[1]
        assert torch.equal(y[t:t + 1], solo), t
    # the module reports it from check_status(), never from forward()
    out = m(x, dev(bad).long(), rw)
    assert torch.equal(out[keep], clean[keep])
    with pytest.raises(IndexError, match="out of range"):
        m.check_status()
    m.check_status()                                               # cleared


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("shape,layout", [("384x640e5k3", "b128x128"), ("256x256e8k8", "row"), ("1280x128e3k2", "gu64x256_d32x128"),
                                          ("4224x128e3k2", "gu64x384_d32x128"), ("256x768e8k8", "gu128x128_d32x256")])
def test_a_tokens_bits_do_not_depend_on_its_batch(shape, layout, act):
    c = MF.case(shape, layout, 16, act)
    m = fused_experts(shape, layout)
    x, ids, rw = dev(c["x"], act), dev(c["ids"]), dev(c["rw"])
    a, y, _ = run_ops(m, x, ids, rw)
    k = ids.shape[1]
    for t in (0, 7, 15):
        a1, y1, _ = run_ops(m, x[t:t + 1].contiguous(), ids[t:t + 1].contiguous(), rw[t:t + 1].contiguous())
        assert torch.equal(a1, a[t * k:(t + 1) * k]) and torch.equal(y1, y[t:t + 1]), t


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("layout", ["tensor", "b128x128"])
def test_slow_path_beyond_sixteen_tokens(layout, act):
    """T = 17 takes the host-routed loop on ops.fp8_gemm over views of the stacked buffers (scales off a 16-byte boundary handed out as copies).
    It repeats the rounding structure of `chain` from stage one on (each expert's output rounded, its product with the routing weight rounded,
    index_add_ in the dtype), so it is held to the bar tests/test_gpu_moe.py holds its slow path to: helpers.NORM_TOL against `chain`."""
    shape = "256x128e8k2"
    c = MF.case(shape, layout, 17, act)
    m = fused_experts(shape, layout)
    assert not m.fast_path(17, c["ids"].shape[1], TDT[act])
    y = m(dev(c["x"], act), dev(c["ids"]).long(), dev(c["rw"]).to(TDT[act]))
    e = rel_err(host(y), c["chain"])
    print(f"slow path {shape} {layout} {act} T=17: vs chain {e:.3e} (bar {NORM_TOL[act]:.0e}); vs y64 {F.rel64(host(y), c['y64']):.3e}, "
          f"chain vs y64 {F.rel64(c['chain'], c['y64']):.3e}")
    assert e <= NORM_TOL[act], e
    with pytest.raises(IndexError):
        m(dev(c["x"], act), torch.full_like(dev(c["ids"]), 99).long(), dev(c["rw"]))


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("layout", ["row", "b128x128"])
def test_slow_and_fast_paths_at_sixteen_tokens(layout, act):
    shape = "384x640e5k3"
    c = MF.case(shape, layout, 16, act)
    m = fused_experts(shape, layout)
    x, ids, rw = dev(c["x"], act), dev(c["ids"]).long(), dev(c["rw"]).to(TDT[act])
    fast = m(x, ids, rw).clone()
    slow = m._forward_loop(x, ids, rw)
    e_slow, e_fast, b = F.rel64(host(slow), c["y64"]), F.rel64(host(fast), c["y64"]), MF.bar(c)
    print(f"T=16 {layout} {act}: slow {e_slow:.3e}, fast {e_fast:.3e} (bar {b:.3e}), slow vs fast {rel_err(host(slow), host(fast)):.3e}")
    assert e_slow <= b and e_fast <= b


def test_forward_replays_inside_a_graph_with_new_routing():
    shape, layout, act, T = "256x128e8k2", "b128x128", "fp16", 2
    H, I, E, k = MF.SHAPES[shape]
    m = fused_experts(shape, layout)
    xs = [dev(MO.make_x(200 + i, T, H, act), act) for i in range(3)]
    routes = [MO.make_routing(300 + i, T, E, k, act) for i in range(3)]
    eager = [m(x, dev(i), dev(w)).clone() for x, (i, w) in zip(xs, routes)]
    x_in, ids_in, w_in = xs[0].clone(), dev(routes[0][0]), dev(routes[0][1])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        m(x_in, ids_in, w_in)                                  # warm-up on the capture stream
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            out = m(x_in, ids_in, w_in)
    torch.cuda.current_stream().wait_stream(s)
    for n in (1, 2, 0, 1):                                     # overwrite the captured tensors in place: a different routing per replay
        x_in.copy_(xs[n])
        ids_in.copy_(dev(routes[n][0]))
        w_in.copy_(dev(routes[n][1]))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager[n]), n
    m.check_status()


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("layout", ["tensor", "row", "b128x128"])
def test_large_scale_inv_is_held_to_one_rounding(layout, act):
    """scale_inv up to 1e6: the reference's fp16 cast of scale_inv overflows and `chain` is useless, so the outputs are held to
    rel64(y_once, y64) + 1e-4 alone."""
    shape, T, hi = "384x640e5k3", 5, 1.0e6
    H, I, E, k = MF.SHAPES[shape]
    ex = MF.experts_of(shape, layout, hi)
    assert max(float(s.max()) for e in ex for _, s in e.values()) > 65504.0
    m = fused_experts(shape, layout, hi)
    x = MO.make_x(401, T, H, act).astype(np.float64)
    ids, rw = MO.make_routing(402, T, E, k, act)
    ref = MF.evaluate(ex, MF.weights64_of(shape, layout, hi), layout, x, ids, rw, act, with_chain=False)
    b = F.rel64(ref["y_once"], ref["y64"]) + 1e-4
    a, y, st = run_ops(m, dev(x, act), dev(ids), dev(rw))
    y2, _ = stage_two(m, dev(ref["act_model"], act), dev(ids), dev(rw))
    ym = m(dev(x, act), dev(ids).long(), dev(rw).to(TDT[act]))
    e1, e2, e3 = rel_err(host(a), ref["act_model"]), F.rel64(host(y2), ref["y64"]), F.rel64(host(y), ref["y64"])
    print(f"large scale_inv {layout} {act}: stage1 {e1:.3e}, stage2 {e2:.3e}, both {e3:.3e} (bar {b:.3e})")
    assert st == 0 and e1 <= NORM_TOL[act]
    assert e2 <= b, (e2, b)
    assert e3 <= b, (e3, b)
    assert torch.equal(ym, y)


# ---- fusion on a synthetic block -----------------------------------------------------------------------------------------------------------
class _Expert(nn.Module):
    def __init__(self, names, gate, up, down):
        super().__init__()
        for n, lin in zip(names, (gate, up, down)):
            setattr(self, n, lin)
        self.names = names
        self.act_fn = nn.SiLU()

    def forward(self, x):
        g, u, d = (getattr(self, n) for n in self.names)
        return d(self.act_fn(g(x)) * u(x))


class _Experts(nn.ModuleList):
    """A container of per-expert modules with the experts call of the installed transformers release: the HF loop."""

    def forward(self, hidden_states, top_k_index, top_k_weights):
        final = torch.zeros_like(hidden_states)
        mask = torch.nn.functional.one_hot(top_k_index, num_classes=len(self)).permute(2, 1, 0)
        for e in torch.greater(mask.sum(dim=(-1, -2)), 0).nonzero():
            pos, tok = torch.where(mask[e[0]])
            cur = self[int(e[0])](hidden_states[tok]) * top_k_weights[tok, pos, None]
            final.index_add_(0, tok, cur.to(final.dtype))
        return final


class _Block(nn.Module):
    def __init__(self, hidden, experts, top_k):
        super().__init__()
        self.gate = nn.Linear(hidden, len(experts), bias=False)
        self.experts = experts
        self.top_k = top_k

    def forward(self, hidden_states):
        probs = torch.softmax(self.gate(hidden_states).float(), dim=-1)
        w, idx = torch.topk(probs, self.top_k, dim=-1)
        w = (w / w.sum(dim=-1, keepdim=True)).to(hidden_states.dtype)
        return self.experts(hidden_states, idx, w)


def _block(shape, layout, names, lists=None, post_init=False):
    H, I, E, k = MF.SHAPES[shape]
    gate, up, down = lists if lists is not None else expert_linears(shape, layout)
    if post_init:
        for lin in gate + up + down:
            lin.post_init()
    blk = _Block(H, _Experts([_Expert(names, g, u, d) for g, u, d in zip(gate, up, down)]), k)
    blk.gate = blk.gate.to(DEV).half()
    torch.manual_seed(3)
    blk.gate.weight.data.normal_(0, 0.5)
    return blk.eval()


@pytest.mark.parametrize("names", [("gate_proj", "up_proj", "down_proj"), ("w1", "w3", "w2")])
def test_fuse_moe_experts_on_a_synthetic_block(names):
    from gptqmodel_amd.nn_modules.moe_fp8 import HipFp8MoeExperts
    from gptqmodel_amd.utils.moe import fuse_moe_experts
    shape, layout, act = "384x640e5k3", "b128x128", "fp16"
    H, I, E, k = MF.SHAPES[shape]
    ref_blk, blk = _block(shape, layout, names, post_init=True), _block(shape, layout, names)
    originals = [getattr(e, n) for e in blk.experts for n in names]
    assert fuse_moe_experts(blk) is True and isinstance(blk.experts, HipFp8MoeExperts) and not hasattr(blk, "_gptqhip_moe_skipped")
    assert all(lin.weight.numel() == 0 and lin.weight_scale_inv.numel() == 0 for lin in originals)       # per-expert buffers released
    assert blk.experts.gate_up_weight.shape[0] == E and blk.experts.down_weight.shape[0] == E
    x = dev(MO.make_x(91, 5, H, act), act)
    with torch.no_grad():
        want, got = ref_blk(x), blk(x)
        probs = torch.softmax(ref_blk.gate(x).float(), dim=-1)
        wts, idx = torch.topk(probs, k, dim=-1)
        wts = (wts / wts.sum(dim=-1, keepdim=True)).half()
    blk.experts.check_status()
    ref = MF.evaluate(MF.experts_of(shape, layout), MF.weights64_of(shape, layout), layout, host(x), idx.cpu().numpy().astype(np.int32),
                      host(wts).astype(np.float32), act)
    e_loop, e_got, b = F.rel64(host(want), ref["y64"]), F.rel64(host(got), ref["y64"]), MF.bar(ref)
    print(f"block {names}: own loop over HipFp8Linear {e_loop:.3e}, fused {e_got:.3e} (bar {b:.3e})")
    assert e_got <= b, (e_got, b)


def test_fuse_moe_experts_declines_without_touching_the_block():
    import test_gpu_moe as TG
    from gptqmodel_amd.nn_modules.moe import HipMoeExperts
    from gptqmodel_amd.utils.moe import fuse_moe_experts
    shape, layout, names = "256x128e8k2", "b128x128", ("gate_proj", "up_proj", "down_proj")
    H, I, E, k = MF.SHAPES[shape]
    ex = MF.experts_of(shape, layout)

    def untouched(blk, why):
        before = blk.experts
        sizes = [p.numel() for p in blk.experts.buffers()]
        assert fuse_moe_experts(blk) is False and blk.experts is before and why in blk._gptqhip_moe_skipped, getattr(blk, "_gptqhip_moe_skipped", None)
        assert [p.numel() for p in blk.experts.buffers()] == sizes

    # a bias on one projection
    gate, up, down = expert_linears(shape, layout)
    up[3] = _linear(*ex[3]["up"], *MF.proj_layout(layout, "up"), "biased.up", bias=True)
    untouched(_block(shape, layout, names, (gate, up, down)), "biases")
    # FP8 and GPTQ projections in one block (the int4 fixture of the same name has the same H, I, E)
    gate, up, down = expert_linears(shape, layout)
    assert MO.SHAPES[shape][:3] == (H, I, E)
    down[2] = TG.expert_linears(shape, "fp16")[2][2]
    untouched(_block(shape, layout, names, (gate, up, down)), "mix FP8")
    # one expert's gate / up quantised with another block size
    gate, up, down = expert_linears(shape, layout)
    for lst, name in ((gate, "gate"), (up, "up")):
        codes, _ = ex[5][name]
        lst[5] = _linear(codes, F.make_scale_inv(1, I, H, "block", (64, 128)), "block", (64, 128), f"other.{name}")
    untouched(_block(shape, layout, names, (gate, up, down)), "block size")
    # a GPTQ block still yields HipMoeExperts
    gptq = TG._block(shape, names)
    assert fuse_moe_experts(gptq) is True and isinstance(gptq.experts, HipMoeExperts)
