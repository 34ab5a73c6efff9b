"""Fused quantised MoE experts on the GPU: gptqhip_moe_gate_up / gptqhip_moe_down, HipMoeExperts and fuse_moe_experts against the numpy
oracle of the HF experts loop (tests/moe_oracle.py).

Bars.  Stage one repeats the reference's rounding chain up to the fp32 summation order: helpers.NORM_TOL against act_ref.  Stage two sums the
top_k expert outputs once in fp32 and rounds once, which is NOT the reference's chain, so it is held to float64 arithmetic instead:
    rel_err(got, y64) <= max(rel_err(chain, y64), rel_err(y64 rounded once, y64)) + 1e-4
(no worse than the reference chain or one output rounding, plus the fp32-partial-sum allowance of tests/test_gpu_decode_dynamic_range.py);
tests/test_moe_oracle_cpu.py shows on the CPU that the first term is the larger one on every case here."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import moe_oracle as MO
from helpers import NORM_TOL, TDT, WEIGHT_RANGE_DTYPES, f32_to_torch, rel_err, torch_to_f32

pytestmark = pytest.mark.gpu
DEV = "cuda"
_FUSED = {}


def _linear(t, K, N, gs, scale_dtype, name, g_idx=None):
    from gptqmodel_amd.nn_modules.qlinear.hip_gptq import HipGptqLinear
    qweight, qzeros, scales, gi = t
    lin = HipGptqLinear(bits=4, group_size=gs, sym=False, desc_act=g_idx is not None, in_features=K, out_features=N, bias=False, name=name)
    lin.qweight, lin.qzeros = torch.from_numpy(qweight), torch.from_numpy(qzeros)
    lin.scales, lin.g_idx = f32_to_torch(scales, scale_dtype), torch.from_numpy(gi if g_idx is None else g_idx)
    lin.qzero_format(format=2)
    return lin.to(DEV).eval()


def expert_linears(shape, scale_dtype):
    """Fresh checkpoint-layout modules of every expert: ([gate], [up], [down])."""
    H, I, E, _, gs = MO._ALL_SHAPES[shape]
    ex = MO.experts_of(shape, scale_dtype)
    return ([_linear(ex[e]["gate"], H, I, gs, scale_dtype, f"e{e}.gate") for e in range(E)],
            [_linear(ex[e]["up"], H, I, gs, scale_dtype, f"e{e}.up") for e in range(E)],
            [_linear(ex[e]["down"], I, H, gs, scale_dtype, f"e{e}.down") for e in range(E)])


def fused_experts(shape, scale_dtype):
    from gptqmodel_amd.nn_modules.moe import HipMoeExperts
    key = (shape, scale_dtype)
    if key not in _FUSED:
        _FUSED[key] = HipMoeExperts.from_linears(*expert_linears(shape, scale_dtype))
    return _FUSED[key]


def bar(c):
    return max(MO.rel64(c["chain"], c["y64"]), MO.rel64(c["y_once"], c["y64"])) + 1e-4


def dev(a, act=None):
    a = np.array(a)      # (the oracle's arrays are read-only)
    return f32_to_torch(a, act, DEV) if act else torch.from_numpy(a).to(DEV)


def run_ops(m, x, ids, rw, act):
    """The two ops on a module's stacked buffers: (stage one [T k, I], output [T, H], status)."""
    from gptqmodel_amd import ops
    T, k = ids.shape
    a = torch.empty((T * k, m.intermediate_dim), dtype=TDT[act], device=DEV)
    out = torch.empty((T, m.hidden_dim), dtype=TDT[act], device=DEV)
    st = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.moe_gate_up(x, m.gate_up_qweight, m.gate_up_meta, ids, a, st, m.num_experts, m.intermediate_dim, m.gate_up_group_size, m.scale_dtype)
    ops.moe_down(a, m.down_qweight, m.down_meta, ids, rw, out, st, m.num_experts, m.down_group_size, m.scale_dtype)
    return a, out, int(st.item())


@pytest.mark.parametrize("act,scale_dtype", WEIGHT_RANGE_DTYPES)
@pytest.mark.parametrize("T", MO.TOKENS)
@pytest.mark.parametrize("shape", sorted(MO.SHAPES))
def test_stages_and_module_against_the_oracle(shape, T, act, scale_dtype):
    from gptqmodel_amd import ops
    c = MO.case(shape, T, act, scale_dtype)
    m = fused_experts(shape, scale_dtype)
    assert m.fast_path(T, c["ids"].shape[1], TDT[act])
    x, ids, rw = dev(c["x"], act), dev(c["ids"]), dev(c["rw"])
    a, y, st = run_ops(m, x, ids, rw, act)
    # stage one: the reference's own chain up to the fp32 summation order
    e1 = rel_err(torch_to_f32(a), c["act_ref"])
    # stage two, fed act_ref
    y2 = torch.empty_like(y)
    st2 = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.moe_down(dev(c["act_ref"], act), m.down_qweight, m.down_meta, ids, rw, y2, st2, m.num_experts, m.down_group_size, m.scale_dtype)
    e2 = MO.rel64(torch_to_f32(y2), c["y64"])
    # both stages from x, and the module end to end with the tensors HF hands it (int64 indices, routing weights in the activation dtype)
    e3 = MO.rel64(torch_to_f32(y), c["y64"])
    ym = m(x, ids.long(), rw.to(TDT[act]))
    e4 = MO.rel64(torch_to_f32(ym), c["y64"])
    print(f"{shape} T={T} {act}x{scale_dtype}: stage1 {e1:.3e} (bar {NORM_TOL[act]:.0e}); stage2 {e2:.3e}, both {e3:.3e}, module {e4:.3e} "
          f"(bar {bar(c):.3e}: chain {MO.rel64(c['chain'], c['y64']):.3e}, one rounding {MO.rel64(c['y_once'], c['y64']):.3e})")
    assert st == 0 and int(st2.item()) == 0
    m.check_status()
    assert e1 <= NORM_TOL[act], e1
    assert e2 <= bar(c), (e2, bar(c))
    assert e3 <= bar(c), (e3, bar(c))
    assert e4 <= bar(c), (e4, bar(c))
    assert torch.equal(ym, y)


@pytest.mark.parametrize("act,scale_dtype", WEIGHT_RANGE_DTYPES)
@pytest.mark.parametrize("T", MO.DEEP_TOKENS)
@pytest.mark.parametrize("shape", sorted(MO.DEEP_SHAPES))
def test_deep_k_and_wide_top_k_against_the_oracle(shape, T, act, scale_dtype):
    """Waves that run several chunks (rounds of kMoeAhead loads with a ragged last one, chunks of one wave in different groups) and top_k 7, 8
    and 16 -- what each shape reaches: tests/test_moe_wave_model_cpu.py.  The assertions and bars of test_stages_and_module_against_the_oracle."""
    from gptqmodel_amd import ops
    c = MO.case(shape, T, act, scale_dtype)
    m = fused_experts(shape, scale_dtype)
    assert m.fast_path(T, c["ids"].shape[1], TDT[act])
    x, ids, rw = dev(c["x"], act), dev(c["ids"]), dev(c["rw"])
    a, y, st = run_ops(m, x, ids, rw, act)
    e1 = rel_err(torch_to_f32(a), c["act_ref"])
    y2 = torch.empty_like(y)
    st2 = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.moe_down(dev(c["act_ref"], act), m.down_qweight, m.down_meta, ids, rw, y2, st2, m.num_experts, m.down_group_size, m.scale_dtype)
    e2 = MO.rel64(torch_to_f32(y2), c["y64"])
    e3 = MO.rel64(torch_to_f32(y), c["y64"])
    ym = m(x, ids.long(), rw.to(TDT[act]))
    e4 = MO.rel64(torch_to_f32(ym), c["y64"])
    print(f"deep {shape} T={T} {act}x{scale_dtype}: stage1 {e1:.3e} (bar {NORM_TOL[act]:.0e}); stage2 {e2:.3e}, both {e3:.3e}, module {e4:.3e} "
          f"(bar {bar(c):.3e}: chain {MO.rel64(c['chain'], c['y64']):.3e}, one rounding {MO.rel64(c['y_once'], c['y64']):.3e})")
    assert st == 0 and int(st2.item()) == 0
    m.check_status()
    assert e1 <= NORM_TOL[act], e1
    assert e2 <= bar(c), (e2, bar(c))
    assert e3 <= bar(c), (e3, bar(c))
    assert e4 <= bar(c), (e4, bar(c))
    assert torch.equal(ym, y)


@pytest.mark.parametrize("act,scale_dtype", WEIGHT_RANGE_DTYPES)
@pytest.mark.parametrize("shape", ["2304x1536e4k4g256", "256x1408e8k8"])
def test_a_tokens_bits_do_not_depend_on_its_batch_or_the_run(shape, act, scale_dtype):
    c = MO.case(shape, 16, act, scale_dtype)
    m = fused_experts(shape, scale_dtype)
    x, ids, rw = dev(c["x"], act), dev(c["ids"]), dev(c["rw"])
    a, y, _ = run_ops(m, x, ids, rw, act)
    a_b, y_b, _ = run_ops(m, x, ids, rw, act)
    assert torch.equal(a, a_b) and torch.equal(y, y_b)               # two runs: the same bits
    k = ids.shape[1]
    for t in (0, 7, 15):                                             # a token alone: the bits it has inside the batch of 16
        a1, y1, _ = run_ops(m, x[t:t + 1].contiguous(), ids[t:t + 1].contiguous(), rw[t:t + 1].contiguous(), act)
        assert torch.equal(a1, a[t * k:(t + 1) * k]) and torch.equal(y1, y[t:t + 1]), t


@pytest.mark.parametrize("act,scale_dtype", WEIGHT_RANGE_DTYPES)
def test_routing_corners(act, scale_dtype):
    shape = "384x640e5k3"
    H, I, E, k, _ = MO.SHAPES[shape]
    m = fused_experts(shape, scale_dtype)
    w = MO.rounded_weights(shape, act, scale_dtype)
    x = MO.make_x(77, 4, H, act)
    _, rw = MO.make_routing(78, 4, E, k, act)
    # token 0: all slots on one expert; tokens 1 and 2 share expert 3 (in different slots); token 3: ids 0 and E - 1 together
    ids = np.array([[2, 2, 2], [3, 1, 0], [4, 3, 1], [0, E - 1, 2]], np.int32)
    ref = MO.evaluate(w, x, ids, rw, act)
    a, y, st = run_ops(m, dev(x, act), dev(ids), dev(rw), act)
    e1, e3 = rel_err(torch_to_f32(a), ref["act_ref"]), MO.rel64(torch_to_f32(y), ref["y64"])
    print(f"corners {act}x{scale_dtype}: stage1 {e1:.3e}, both {e3:.3e} (bar {bar(ref):.3e})")
    assert st == 0 and e1 <= NORM_TOL[act] and e3 <= bar(ref)
    # run-to-run bit equality (no atomics, fixed summation order)
    a_b, y_b, _ = run_ops(m, dev(x, act), dev(ids), dev(rw), act)
    assert torch.equal(a, a_b) and torch.equal(y, y_b)
    # a zero routing weight contributes exactly nothing: swap that slot's expert for any other, the output keeps its bits
    rw0 = rw.copy()
    rw0[:, 1] = 0.0
    base = run_ops(m, dev(x, act), dev(ids), dev(rw0), act)[1]
    for other in range(E):
        ids2 = ids.copy()
        ids2[:, 1] = other
        assert torch.equal(run_ops(m, dev(x, act), dev(ids2), dev(rw0), act)[1], base), other


def test_out_of_range_ids_set_status_and_contribute_zero():
    shape, act, sdt = "256x128e8k2", "fp16", "fp16"
    H, I, E, k, _ = MO.SHAPES[shape]
    m = fused_experts(shape, sdt)
    c = MO.case(shape, 5, act, sdt)
    x, rw = dev(c["x"], act), dev(c["rw"])
    _, clean, st = run_ops(m, x, dev(c["ids"]), rw, act)
    assert st == 0
    bad = c["ids"].copy()
    bad[1, 0], bad[3, 1] = -1, E
    a, y, st = run_ops(m, x, dev(bad), rw, act)
    assert st == 1
    keep = [0, 2, 4]
    assert torch.equal(y[keep], clean[keep])                       # the other tokens: bit-identical to the clean run
    assert not a[1 * k + 0].any() and not a[3 * k + 1].any()       # the bad slots' stage-one rows are zeros
    # ... and the bad slot contributes zero: the token's output is that of its remaining slot alone
    for t, j_ok in ((1, 1), (3, 0)):
        solo = MO.evaluate(MO.rounded_weights(shape, act, sdt), c["x"][t:t + 1], c["ids"][t:t + 1, j_ok:j_ok + 1], c["rw"][t:t + 1, j_ok:j_ok + 1], act)
        assert MO.rel64(torch_to_f32(y[t:t + 1]), solo["y64"]) <= bar(solo)
    # the module reports it from check_status(), never from forward()
    out = m(x, dev(bad).long(), rw)
    assert torch.equal(out[keep], clean[keep])
    with pytest.raises(IndexError, match="out of range"):
        m.check_status()
    m.check_status()                                               # cleared


@pytest.mark.parametrize("shape,T", [("256x128e8k2", 17), (MO.GS64_SHAPE, 5), (MO.GS64_SHAPE, 17)])
def test_slow_path_agrees_with_the_chain(shape, T):
    act = sdt = "fp16"
    c = MO.case(shape, T, act, sdt)
    m = fused_experts(shape, sdt)
    assert not (T <= 16 and m.fast_path(T, c["ids"].shape[1], TDT[act]))
    y = m(dev(c["x"], act), dev(c["ids"]).long(), dev(c["rw"]).to(TDT[act]))
    e = rel_err(torch_to_f32(y), c["chain"])
    print(f"slow path {shape} T={T}: {e:.3e}")
    assert e <= NORM_TOL[act]
    with pytest.raises(IndexError):
        m(dev(c["x"], act), torch.full_like(dev(c["ids"]), 99).long(), dev(c["rw"]))


@pytest.mark.parametrize("act,scale_dtype", WEIGHT_RANGE_DTYPES)
def test_slow_and_fast_paths_agree_at_sixteen_tokens(act, scale_dtype):
    shape = "384x640e5k3"
    c = MO.case(shape, 16, act, scale_dtype)
    m = fused_experts(shape, scale_dtype)
    x, ids, rw = dev(c["x"], act), dev(c["ids"]).long(), dev(c["rw"]).to(TDT[act])
    fast = m(x, ids, rw).clone()
    slow = m._forward_loop(x, ids, rw)
    e_slow, e_fast = rel_err(torch_to_f32(slow), c["chain"]), MO.rel64(torch_to_f32(fast), c["y64"])
    print(f"T=16 {act}x{scale_dtype}: slow vs chain {e_slow:.3e}, fast vs y64 {e_fast:.3e} (bar {bar(c):.3e}), slow vs fast "
          f"{rel_err(torch_to_f32(slow), torch_to_f32(fast)):.3e}")
    assert e_slow <= NORM_TOL[act] and e_fast <= bar(c)
    assert MO.rel64(torch_to_f32(slow), c["y64"]) <= bar(c)


def test_forward_replays_inside_a_graph_with_new_routing():
    shape, act, sdt = "256x128e8k2", "fp16", "fp16"
    H, I, E, k, _ = MO.SHAPES[shape]
    m = fused_experts(shape, sdt)
    xs = [dev(MO.make_x(200 + i, 1, H, act), act) for i in range(3)]
    routes = [MO.make_routing(300 + i, 1, E, k, act) for i in range(3)]
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


def _block(shape, names, container=_Experts, act_order_expert=None, post_init=False):
    H, I, E, k, gs = MO.SHAPES[shape]
    gate, up, down = expert_linears(shape, "fp16")
    if act_order_expert is not None:
        g_idx = (np.random.RandomState(5).permutation(I) // gs).astype(np.int32)
        down[act_order_expert] = _linear(MO.experts_of(shape, "fp16")[act_order_expert]["down"], I, H, gs, "fp16", "ao.down", g_idx=g_idx)
    blk = _Block(H, container([_Expert(names, g, u, d) for g, u, d in zip(gate, up, down)]), k).to(DEV).half().eval()
    torch.manual_seed(3)
    blk.gate.weight.data.normal_(0, 0.5)
    if post_init:
        from gptqmodel_amd.utils.model import gptqmodel_post_init
        blk._gptqhip_auto_fuse = False
        gptqmodel_post_init(blk)
    return blk


@pytest.mark.parametrize("names", [("gate_proj", "up_proj", "down_proj"), ("w1", "w3", "w2")])
def test_fuse_moe_experts_on_a_synthetic_block(names):
    from gptqmodel_amd.nn_modules.moe import HipMoeExperts
    from gptqmodel_amd.utils.moe import fuse_moe_experts
    shape, act = "384x640e5k3", "fp16"
    H, I, E, k, _ = MO.SHAPES[shape]
    ref_blk, blk = _block(shape, names, post_init=True), _block(shape, names)
    originals = [getattr(e, n) for e in blk.experts for n in names]
    assert fuse_moe_experts(blk) is True and isinstance(blk.experts, HipMoeExperts) and not hasattr(blk, "_gptqhip_moe_skipped")
    assert all(lin.qweight.numel() == 0 and lin.scales.numel() == 0 for lin in originals)       # per-expert buffers released
    assert blk.experts.gate_up_qweight.shape[0] == E and blk.experts.down_qweight.shape[0] == E
    x = dev(MO.make_x(91, 5, H, act), act)
    with torch.no_grad():
        want, got = ref_blk(x), blk(x)
        probs = torch.softmax(ref_blk.gate(x).float(), dim=-1)
        wts, idx = torch.topk(probs, k, dim=-1)
        wts = (wts / wts.sum(dim=-1, keepdim=True)).half()
    blk.experts.check_status()
    ref = MO.evaluate(MO.rounded_weights(shape, act, "fp16"), torch_to_f32(x), idx.cpu().numpy().astype(np.int32), torch_to_f32(wts), act)
    e_loop, e_got = MO.rel64(torch_to_f32(want), ref["y64"]), MO.rel64(torch_to_f32(got), ref["y64"])
    print(f"block {names}: own loop {e_loop:.3e}, fused {e_got:.3e} (bar {bar(ref):.3e}); loop vs oracle chain {rel_err(torch_to_f32(want), ref['chain']):.3e}")
    assert rel_err(torch_to_f32(want), ref["chain"]) <= NORM_TOL[act]
    assert e_got <= bar(ref), (e_got, bar(ref))
    # the same stacked buffers from modules that were already post_init()ed (interleaved in the tiled layout)
    pi = _block(shape, names, post_init=True)
    m2 = HipMoeExperts.from_linears(*([getattr(e, n) for e in pi.experts] for n in names))
    for name in ("gate_up_qweight", "gate_up_meta", "down_qweight", "down_meta"):
        assert torch.equal(getattr(m2, name), getattr(blk.experts, name)), name


def test_fuse_moe_experts_declines_without_touching_the_block():
    from gptqmodel_amd.utils.moe import auto_fuse_moe, fuse_moe_experts
    shape, names = "384x640e5k3", ("gate_proj", "up_proj", "down_proj")      # (five groups on the down side: a permutation exists)
    blk = _block(shape, names, act_order_expert=3)
    before = blk.experts
    sizes = [getattr(e, n).qweight.numel() for e in blk.experts for n in names]
    assert fuse_moe_experts(blk) is False and blk.experts is before
    assert "act-order" in blk._gptqhip_moe_skipped
    assert [getattr(e, n).qweight.numel() for e in blk.experts for n in names] == sizes
    # a bare ModuleList is indexed by its block's own forward: nothing to stand in for
    bare = _block(shape, names, container=nn.ModuleList)
    assert fuse_moe_experts(bare) is False and isinstance(bare.experts, nn.ModuleList) and "indexed" in bare._gptqhip_moe_skipped
    assert fuse_moe_experts(nn.Linear(4, 4)) is False
    model = nn.Sequential(blk)
    assert auto_fuse_moe(model) == 0 and model._gptqhip_moe_skipped[0][0] == "_Block"


def test_auto_fuse_on_the_dense_llama_fixture_is_unchanged():
    pytest.importorskip("transformers")
    from test_gpu_e2e_llama import _build
    from gptqmodel_amd.utils.model import _FusedGroup
    _, quant = _build(False, "layers_dims_only", torch.float16)       # gptqmodel_post_init -> auto_fuse (+ auto_fuse_moe at its tail)
    assert quant._gptqhip_fused_layers == 2 and quant._gptqhip_skipped_layers == []
    assert not hasattr(quant, "_gptqhip_moe_fused") and not hasattr(quant, "_gptqhip_moe_skipped")
    for layer in quant.model.layers:
        assert isinstance(layer.mlp.fused_gate_up, _FusedGroup) and isinstance(layer.self_attn.fused_q_proj_k_proj_v_proj, _FusedGroup)
        assert hasattr(layer, "_gptqhip_fused")
