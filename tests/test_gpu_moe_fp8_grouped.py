"""Expert-grouped fused FP8 MoE ops on the GPU: gptqhip_moe_align -> gptqhip_moe_fp8_gate_up_grouped -> gptqhip_moe_fp8_down_grouped ->
gptqhip_moe_combine, HipFp8MoeExperts' grouped path and fuse_moe_experts(grouped_routing=True) against the oracle of tests/moe_fp8_oracle.py at
the bars of tests/test_gpu_moe_fp8.py: stage one at helpers.NORM_TOL against act_model, everything after the combine at
    rel64(got, y64) <= max(rel64(chain, y64), rel64(y_once, y64)) + 1e-4.
Token counts 1, 5, 16, 17, 33, 70: units that are empty, partial, exactly full and several per expert.  The K summation order differs from the
few-token kernels': the two paths are held to the same bar, never to each other's bits.  tests/test_moe_fp8_grouped_cpu.py shows on the CPU that a
float32 model of the contract fits the bars on every case here, and what the deep shapes reach in the kernel's chunk deal."""
import numpy as np
import pytest
import torch

import fp8_oracle as F
import moe_fp8_oracle as MF
import moe_oracle as MO
from helpers import NORM_TOL, rel_err
from test_gpu_moe_fp8 import ACTS, TDT, _block, dev, fused_experts, expert_linears, host, run_ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOKENS = (1, 5, 16, 17, 33, 70)
DEEP_CASES = [("4224x128e3k2", "row"), ("4224x128e3k2", "b128x128"), ("4224x128e3k2", "gu64x384_d32x128"),
              ("128x4224e3k2", "tensor"), ("128x4224e3k2", "b128x128"), ("128x4224e3k2", "gu128x128_d32x384")]
DEEP_TOKENS = (5, 33)
_GROUPED = {}


def grouped_experts(shape, layout):
    """A module of its own with grouped_routing set (the shared one of test_gpu_moe_fp8.py keeps the default)."""
    from gptqmodel_amd.nn_modules.moe_fp8 import HipFp8MoeExperts
    key = (shape, layout)
    if key not in _GROUPED:
        _GROUPED[key] = HipFp8MoeExperts.from_linears(*expert_linears(shape, layout))
        _GROUPED[key].grouped_routing = True
        _GROUPED[key].grouped_min_tokens = 1
    return _GROUPED[key]


def sort_buffers(S, E):
    from gptqmodel_amd import ops
    mu = ops.moe_grouped_units(S, E)
    # poisoned: every word must be written by the op
    return (torch.full((16 * mu,), 12345, dtype=torch.int32, device=DEV), torch.full((mu,), 12345, dtype=torch.int32, device=DEV),
            torch.full((1,), 12345, dtype=torch.int32, device=DEV))


def run_grouped(m, x, ids, rw, act_in=None):
    """The four ops on a module's stacked buffers: (stage one [T k, I], output [T, H], status).  act_in: feed stage two this instead."""
    from gptqmodel_amd import ops
    T, k = ids.shape
    S, E, I, H = T * k, m.num_experts, m.intermediate_dim, m.hidden_dim
    ss, ue, nu = sort_buffers(S, E)
    st = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.moe_align(ids, ss, ue, nu, st, E)
    a = torch.zeros((S, I), dtype=x.dtype, device=DEV)
    ops.moe_fp8_gate_up_grouped(x, m.gate_up_weight, m.gate_up_rscale, ss, ue, nu, a, k, E, I, m.gate_up_block_cols)
    part = torch.full((S, H), float("nan"), dtype=torch.float32, device=DEV)      # a row no unit owns must never reach the output
    ops.moe_fp8_down_grouped(a if act_in is None else act_in, m.down_weight, m.down_rscale, ss, ue, nu, part, k, E, H, *m._down_mode())
    out = torch.empty((T, H), dtype=x.dtype, device=DEV)
    ops.moe_combine(part, ids, rw, out, st, E)
    return a, out, int(st.item())


def check_against_the_oracle(tag, shape, layout, T, act):
    c = MF.case(shape, layout, T, act)
    m = fused_experts(shape, layout)
    assert m.grouped_path(T, c["ids"].shape[1], TDT[act])
    x, ids, rw = dev(c["x"], act), dev(c["ids"]), dev(c["rw"])
    a, y, st = run_grouped(m, x, ids, rw)
    e1 = rel_err(host(a), c["act_model"])                                               # stage one: the stated chain up to the fp32 summation order
    _, y2, st2 = run_grouped(m, x, ids, rw, act_in=dev(c["act_model"], act))            # stage two + combine, fed act_model
    e2, e3, b = F.rel64(host(y2), c["y64"]), F.rel64(host(y), c["y64"]), MF.bar(c)
    print(f"{tag}{shape} {layout} T={T} {act}: stage1 {e1:.3e} (bar {NORM_TOL[act]:.0e}); stage2 {e2:.3e}, pipeline {e3:.3e} "
          f"(bar {b:.3e}: chain {F.rel64(c['chain'], c['y64']):.3e}, one rounding {F.rel64(c['y_once'], c['y64']):.3e})")
    assert st == 0 and st2 == 0
    assert e1 <= NORM_TOL[act], e1
    assert e2 <= b, (e2, b)
    assert e3 <= b, (e3, b)


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("T", TOKENS)
@pytest.mark.parametrize("shape,layout", MF.CASES)
def test_stages_against_the_oracle(shape, layout, T, act):
    check_against_the_oracle("", shape, layout, T, act)


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("T", DEEP_TOKENS)
@pytest.mark.parametrize("shape,layout", DEEP_CASES)
def test_deep_k_stages_against_the_oracle(shape, layout, T, act):
    """33 chunks over 8 or 16 waves: contiguous ranges longer than the look-ahead with a ragged last round, K blocks of 3 chunks that wave boundaries
    cut (share-end flushes), and a combine of five column blocks whose last is partial (part is NaN-poisoned by run_grouped) -- what each shape
    reaches: tests/test_moe_fp8_grouped_cpu.py.  The assertions and bars of test_stages_against_the_oracle."""
    check_against_the_oracle("deep ", shape, layout, T, act)


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("layout", ["b128x128", "row"])
def test_batch_independence(layout, act):
    shape, T = "384x640e5k3", 70
    c = MF.case(shape, layout, T, act)
    m = fused_experts(shape, layout)
    x, ids, rw = dev(c["x"], act), dev(c["ids"]), dev(c["rw"])
    a, y, _ = run_grouped(m, x, ids, rw)
    a_b, y_b, _ = run_grouped(m, x, ids, rw)
    assert torch.equal(a, a_b) and torch.equal(y, y_b)                                   # two runs: the same bits
    perm = torch.from_numpy(np.random.RandomState(4).permutation(T)).to(DEV)
    _, y_p, _ = run_grouped(m, x[perm].contiguous(), ids[perm].contiguous(), rw[perm].contiguous())
    assert torch.equal(y_p, y[perm])                                                     # permuted tokens: permuted rows, bit for bit
    for t in (0, 37, 69):                                                                # a token alone: the bits it has inside the batch
        _, y_1, _ = run_grouped(m, x[t:t + 1].contiguous(), ids[t:t + 1].contiguous(), rw[t:t + 1].contiguous())
        assert torch.equal(y_1[0], y[t]), t


@pytest.mark.parametrize("layout", ["b128x128", "row"])
def test_zero_routing_weight_contributes_exactly_nothing(layout):
    shape, act, T = "384x640e5k3", "fp16", 33
    H, I, E, k = MF.SHAPES[shape]
    c = MF.case(shape, layout, T, act)
    m = fused_experts(shape, layout)
    rw0 = c["rw"].copy()
    rw0[:, 1] = 0.0
    base = run_grouped(m, dev(c["x"], act), dev(c["ids"]), dev(rw0))[1]
    for other in range(E):      # swap that slot's expert for any other (the units change): the output keeps its bits
        ids2 = c["ids"].copy()
        ids2[:, 1] = other
        assert torch.equal(run_grouped(m, dev(c["x"], act), dev(ids2), dev(rw0))[1], base), other


@pytest.mark.parametrize("layout", ["tensor", "b128x128"])
def test_out_of_range_ids_set_status_and_contribute_zero(layout):
    """Ids -1 and E are in no unit (gptqhip_moe_align) and are skipped by the combine: nothing is dereferenced through them."""
    shape, act, T = "256x128e8k2", "fp16", 33
    H, I, E, k = MF.SHAPES[shape]
    m = fused_experts(shape, layout)
    c = MF.case(shape, layout, T, act)
    x, rw = dev(c["x"], act), dev(c["rw"])
    _, clean, st = run_grouped(m, x, dev(c["ids"]), rw)
    assert st == 0
    bad = c["ids"].copy()
    bad[1, 0], bad[20, 1] = -1, E
    _, y, st = run_grouped(m, x, dev(bad), rw)
    assert st == 1
    keep = [t for t in range(T) if t not in (1, 20)]
    assert torch.equal(y[keep], clean[keep])                       # the other tokens: bit-identical to the clean run
    for t, j_ok in ((1, 1), (20, 0)):                              # the bad slot contributes zero: the token's output is that of its remaining slot
        solo = MF.evaluate(MF.experts_of(shape, layout), MF.weights64_of(shape, layout), layout, c["x"][t:t + 1],
                           c["ids"][t:t + 1, j_ok:j_ok + 1], c["rw"][t:t + 1, j_ok:j_ok + 1], act)
        e = F.rel64(host(y[t:t + 1]), solo["y64"])
        assert e <= MF.bar(solo), (t, e, MF.bar(solo))


@pytest.mark.parametrize("T", [17, 70])
def test_module_grouped_path_equals_the_four_ops(T):
    shape, layout, act = "384x640e5k3", "b128x128", "fp16"
    c = MF.case(shape, layout, T, act)
    m = grouped_experts(shape, layout)
    x, ids, rw = dev(c["x"], act), dev(c["ids"]), dev(c["rw"])
    _, want, _ = run_grouped(m, x, ids, rw)
    got = m(x, ids.long(), rw.to(TDT[act]))                        # what HF hands it: int64 indices, routing weights in the activation dtype
    assert torch.equal(got, want)
    assert F.rel64(host(got), c["y64"]) <= MF.bar(c)
    m.check_status()
    # an eager call at another T shares the grow-only buffer set
    m(x[:5].contiguous(), ids[:5].long(), rw[:5].to(TDT[act]))
    assert len(m._grouped_eager) == 1 and len(m._grouped_captured) == 0
    # out-of-range ids: check_status(), never forward(); it raises once and clears
    bad = ids.clone()
    bad[2, 0] = m.num_experts
    m(x, bad.long(), rw)
    with pytest.raises(IndexError, match="out of range"):
        m.check_status()
    m.check_status()


def test_module_default_keeps_the_host_loop_at_seventeen_tokens():
    shape, layout, act, T = "256x128e8k2", "b128x128", "fp16", 17
    c = MF.case(shape, layout, T, act)
    m = fused_experts(shape, layout)
    assert m.grouped_routing is False
    x, ids, rw = dev(c["x"], act), dev(c["ids"]).long(), dev(c["rw"]).to(TDT[act])
    assert torch.equal(m(x, ids, rw), m._forward_loop(x, ids, rw))
    assert len(m._grouped_eager) == 0


def test_forward_is_captured_at_thirty_three_tokens_and_replays_with_new_routing():
    shape, layout, act, T = "256x128e8k2", "b128x128", "fp16", 33
    H, I, E, k = MF.SHAPES[shape]
    m = fused_experts(shape, layout)                                # the default flag: under capture T > 16 takes the grouped path
    assert m.grouped_routing is False
    captured_before = len(m._grouped_captured)
    xs = [dev(MO.make_x(400 + i, T, H, act), act) for i in range(3)]
    routes = [MO.make_routing(500 + i, T, E, k, act) for i in range(3)]
    eager = [run_grouped(m, x, dev(i), dev(w))[1] for x, (i, w) in zip(xs, routes)]
    x_in, ids_in, w_in = xs[0].clone(), dev(routes[0][0]), dev(routes[0][1])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            out = m(x_in, ids_in, w_in)
    torch.cuda.current_stream().wait_stream(s)
    for n in (1, 2, 0):                                             # overwrite the captured tensors in place: a different routing per replay
        x_in.copy_(xs[n])
        ids_in.copy_(dev(routes[n][0]))
        w_in.copy_(dev(routes[n][1]))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager[n]), n
    m.check_status()
    assert captured_before == 0 and len(m._grouped_captured) == 1


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("layout", ["tensor", "row", "b128x128"])
def test_large_scale_inv_is_held_to_one_rounding(layout, act):
    """scale_inv up to 1e6: the reference's fp16 cast of scale_inv overflows and `chain` is useless, so the outputs are held to
    rel64(y_once, y64) + 1e-4 alone (the bar of the few-token test of the same name)."""
    shape, T, hi = "384x640e5k3", 33, 1.0e6
    H, I, E, k = MF.SHAPES[shape]
    ex = MF.experts_of(shape, layout, hi)
    assert max(float(s.max()) for e in ex for _, s in e.values()) > 65504.0
    m = fused_experts(shape, layout, hi)
    x = MO.make_x(401, T, H, act).astype(np.float64)
    ids, rw = MO.make_routing(402, T, E, k, act)
    ref = MF.evaluate(ex, MF.weights64_of(shape, layout, hi), layout, x, ids, rw, act, with_chain=False)
    b = F.rel64(ref["y_once"], ref["y64"]) + 1e-4
    a, y, st = run_grouped(m, dev(x, act), dev(ids), dev(rw))
    _, y2, _ = run_grouped(m, dev(x, act), dev(ids), dev(rw), act_in=dev(ref["act_model"], act))
    e1, e2, e3 = rel_err(host(a), ref["act_model"]), F.rel64(host(y2), ref["y64"]), F.rel64(host(y), ref["y64"])
    print(f"large scale_inv {layout} {act} T={T}: stage1 {e1:.3e}, stage2 {e2:.3e}, pipeline {e3:.3e} (bar {b:.3e})")
    assert st == 0 and e1 <= NORM_TOL[act]
    assert e2 <= b, (e2, b)
    assert e3 <= b, (e3, b)


def test_fuse_moe_experts_with_grouped_routing_on_a_synthetic_block():
    from gptqmodel_amd.nn_modules.moe_fp8 import HipFp8MoeExperts
    from gptqmodel_amd.utils.moe import fuse_moe_experts
    shape, layout, act, T = "384x640e5k3", "b128x128", "fp16", 40
    H, I, E, k = MF.SHAPES[shape]
    names = ("gate_proj", "up_proj", "down_proj")
    blk = _block(shape, layout, names)
    assert fuse_moe_experts(blk, grouped_routing=True) is True and isinstance(blk.experts, HipFp8MoeExperts) and blk.experts.grouped_routing is True
    x = dev(MO.make_x(92, T, H, act), act)
    with torch.no_grad():
        got = blk(x)
        probs = torch.softmax(blk.gate(x).float(), dim=-1)
        wts, idx = torch.topk(probs, k, dim=-1)
        wts = (wts / wts.sum(dim=-1, keepdim=True)).half()
    blk.experts.check_status()
    assert len(blk.experts._grouped_eager) == 1                    # (served by the grouped path, not the host loop)
    ref = MF.evaluate(MF.experts_of(shape, layout), MF.weights64_of(shape, layout), layout, host(x), idx.cpu().numpy().astype(np.int32),
                      host(wts).astype(np.float32), act)
    e, b = F.rel64(host(got), ref["y64"]), MF.bar(ref)
    print(f"block T={T}: grouped {e:.3e} (bar {b:.3e})")
    assert e <= b, (e, b)
    blk2 = _block(shape, layout, names)
    assert fuse_moe_experts(blk2, grouped_routing=False) is True and blk2.experts.grouped_routing is False
