"""Expert-grouped fused MoE ops on the GPU: gptqhip_moe_align bit for bit against the numpy model (tests/moe_grouped_model.py), the two grouped
stages + gptqhip_moe_combine, HipMoeExperts' grouped path and fuse_moe_experts(grouped_routing=True) against the oracle of the HF experts loop
(tests/moe_oracle.py) at the bars of tests/test_gpu_moe.py: stage one at helpers.NORM_TOL against act_ref, everything after the combine at
    rel_err(got, y64) <= max(rel_err(chain, y64), rel_err(y64 rounded once, y64)) + 1e-4.
Token counts 1, 5, 16, 17, 33, 70: units that are empty, partial, exactly full and several per expert."""
import numpy as np
import pytest
import torch

import moe_grouped_model as GM
import moe_oracle as MO
from helpers import NORM_TOL, TDT, WEIGHT_RANGE_DTYPES, rel_err, torch_to_f32
from test_gpu_moe import _block, bar, dev, expert_linears, fused_experts, run_ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOKENS = (1, 5, 16, 17, 33, 70)
_GROUPED = {}


def grouped_experts(shape, scale_dtype):
    """A module of its own with grouped_routing set (the shared one of test_gpu_moe.py keeps the default)."""
    from gptqmodel_amd.nn_modules.moe import HipMoeExperts
    key = (shape, scale_dtype)
    if key not in _GROUPED:
        _GROUPED[key] = HipMoeExperts.from_linears(*expert_linears(shape, scale_dtype))
        _GROUPED[key].grouped_routing = True
        _GROUPED[key].grouped_min_tokens = 1
    return _GROUPED[key]


def sort_buffers(S, E):
    from gptqmodel_amd import ops
    mu = ops.moe_grouped_units(S, E)
    # poisoned: every word must be written by the op
    return (torch.full((16 * mu,), 12345, dtype=torch.int32, device=DEV), torch.full((mu,), 12345, dtype=torch.int32, device=DEV),
            torch.full((1,), 12345, dtype=torch.int32, device=DEV))


def run_align(ids, E):
    from gptqmodel_amd import ops
    ss, ue, nu = sort_buffers(ids.numel(), E)
    st = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.moe_align(ids, ss, ue, nu, st, E)
    return ss, ue, nu, st


def run_grouped(m, x, ids, rw, act, act_in=None):
    """The four ops on a module's stacked buffers: (stage one [T k, I], output [T, H], status).  act_in: feed stage two this instead."""
    from gptqmodel_amd import ops
    T, k = ids.shape
    S, E, I, H = T * k, m.num_experts, m.intermediate_dim, m.hidden_dim
    ss, ue, nu, st = run_align(ids, E)
    a = torch.zeros((S, I), dtype=TDT[act], device=DEV)
    ops.moe_gate_up_grouped(x, m.gate_up_qweight, m.gate_up_meta, ss, ue, nu, a, k, E, I, m.gate_up_group_size, m.scale_dtype)
    part = torch.full((S, H), float("nan"), dtype=torch.float32, device=DEV)      # a row no unit owns must never reach the output
    ops.moe_down_grouped(a if act_in is None else act_in, m.down_qweight, m.down_meta, ss, ue, nu, part, k, E, H, m.down_group_size, m.scale_dtype)
    out = torch.empty((T, H), dtype=TDT[act], device=DEV)
    ops.moe_combine(part, ids, rw, out, st, E)
    return a, out, int(st.item())


def assert_align_matches_model(ids_np, E):
    ss, ue, nu, st = run_align(dev(ids_np), E)
    want = GM.align(ids_np, E)
    assert int(nu.item()) == want[2] and int(st.item()) == want[3]
    assert np.array_equal(ss.cpu().numpy(), want[0]) and np.array_equal(ue.cpu().numpy(), want[1])


@pytest.mark.parametrize("E,top_k", [(8, 2), (5, 3), (128, 8), (256, 8), (512, 1)])
def test_align_is_bit_exact_with_the_model(E, top_k):
    for name, ids in GM.routing_cases(E, top_k).items():
        assert_align_matches_model(ids, E)
    assert_align_matches_model(np.array([[E - 1, 0, E // 2]], np.int32), E)            # more experts than slots (at E >= 5)
    # more slots than one pass of the sixteen waves covers (every wave walks several 64-slot steps), a count that is no multiple of 64
    rng = np.random.RandomState(E)
    assert_align_matches_model(rng.randint(0, E, size=(2311, 1)).astype(np.int32), E)
    skew = np.where(rng.rand(1500, top_k) < 0.7, 1 % E, rng.randint(0, E, size=(1500, top_k))).astype(np.int32)
    skew[rng.randint(0, 1500, 9), 0] = -3
    assert_align_matches_model(skew, E)


@pytest.mark.parametrize("act,scale_dtype", WEIGHT_RANGE_DTYPES)
@pytest.mark.parametrize("T", TOKENS)
@pytest.mark.parametrize("shape", sorted(MO.SHAPES))
def test_stages_against_the_oracle(shape, T, act, scale_dtype):
    c = MO.case(shape, T, act, scale_dtype)
    m = fused_experts(shape, scale_dtype)
    assert m.grouped_path(T, c["ids"].shape[1], TDT[act])
    x, ids, rw = dev(c["x"], act), dev(c["ids"]), dev(c["rw"])
    a, y, st = run_grouped(m, x, ids, rw, act)
    e1 = rel_err(torch_to_f32(a), c["act_ref"])                                          # stage one: the reference's own chain
    _, y2, st2 = run_grouped(m, x, ids, rw, act, act_in=dev(c["act_ref"], act))          # stage two + combine, fed act_ref
    e2, e3 = MO.rel64(torch_to_f32(y2), c["y64"]), MO.rel64(torch_to_f32(y), c["y64"])
    print(f"{shape} T={T} {act}x{scale_dtype}: stage1 {e1:.3e} (bar {NORM_TOL[act]:.0e}); stage2 {e2:.3e}, pipeline {e3:.3e} (bar {bar(c):.3e})")
    assert st == 0 and st2 == 0
    assert e1 <= NORM_TOL[act], e1
    assert e2 <= bar(c), (e2, bar(c))
    assert e3 <= bar(c), (e3, bar(c))
    if T <= 16:      # the ungrouped ops serve this too: both inside the bar (the K-step summation order differs, so not bit-equal)
        _, yu, stu = run_ops(m, x, ids, rw, act)
        assert stu == 0 and MO.rel64(torch_to_f32(yu), c["y64"]) <= bar(c)


@pytest.mark.parametrize("act,scale_dtype", WEIGHT_RANGE_DTYPES)
@pytest.mark.parametrize("T", (5, 33))
@pytest.mark.parametrize("shape", ["4224x128e3k2", "128x4224e3k2", "2304x1536e4k4g256"])
def test_deep_k_stages_against_the_oracle(shape, T, act, scale_dtype):
    """Waves that run several chunks (rounds of kGroupedAhead loads with a ragged last one, chunks of one wave in different groups) and a combine
    of 3 and 5 column blocks whose last is partial (part is NaN-poisoned by run_grouped) -- what each shape reaches:
    tests/test_moe_wave_model_cpu.py.  The assertions and bars of test_stages_against_the_oracle."""
    c = MO.case(shape, T, act, scale_dtype)
    m = fused_experts(shape, scale_dtype)
    assert m.grouped_path(T, c["ids"].shape[1], TDT[act])
    x, ids, rw = dev(c["x"], act), dev(c["ids"]), dev(c["rw"])
    a, y, st = run_grouped(m, x, ids, rw, act)
    e1 = rel_err(torch_to_f32(a), c["act_ref"])
    _, y2, st2 = run_grouped(m, x, ids, rw, act, act_in=dev(c["act_ref"], act))
    e2, e3 = MO.rel64(torch_to_f32(y2), c["y64"]), MO.rel64(torch_to_f32(y), c["y64"])
    print(f"deep {shape} T={T} {act}x{scale_dtype}: stage1 {e1:.3e} (bar {NORM_TOL[act]:.0e}); stage2 {e2:.3e}, pipeline {e3:.3e} (bar {bar(c):.3e})")
    assert st == 0 and st2 == 0
    assert e1 <= NORM_TOL[act], e1
    assert e2 <= bar(c), (e2, bar(c))
    assert e3 <= bar(c), (e3, bar(c))
    if T <= 16:      # the ungrouped ops serve this too: both inside the bar
        _, yu, stu = run_ops(m, x, ids, rw, act)
        eu = MO.rel64(torch_to_f32(yu), c["y64"])
        print(f"deep {shape} T={T} {act}x{scale_dtype}: ungrouped ops {eu:.3e}")
        assert stu == 0 and eu <= bar(c)


def test_deep_k_module_grouped_path_equals_the_four_ops():
    shape, act, sdt, T = "2304x1536e4k4g256", "fp16", "fp16", 33
    c = MO.case(shape, T, act, sdt)
    m = grouped_experts(shape, sdt)
    x, ids, rw = dev(c["x"], act), dev(c["ids"]), dev(c["rw"])
    _, want, _ = run_grouped(m, x, ids, rw, act)
    got = m(x, ids.long(), rw.to(TDT[act]))
    assert torch.equal(got, want)
    assert MO.rel64(torch_to_f32(got), c["y64"]) <= bar(c)
    m.check_status()
    assert len(m._grouped_eager) == 1


@pytest.mark.parametrize("act,scale_dtype", WEIGHT_RANGE_DTYPES)
def test_batch_independence(act, scale_dtype):
    shape, T = "384x640e5k3", 70
    c = MO.case(shape, T, act, scale_dtype)
    m = fused_experts(shape, scale_dtype)
    x, ids, rw = dev(c["x"], act), dev(c["ids"]), dev(c["rw"])
    a, y, _ = run_grouped(m, x, ids, rw, act)
    a_b, y_b, _ = run_grouped(m, x, ids, rw, act)
    assert torch.equal(a, a_b) and torch.equal(y, y_b)                                   # two runs: the same bits
    perm = torch.from_numpy(np.random.RandomState(4).permutation(T)).to(DEV)
    _, y_p, _ = run_grouped(m, x[perm].contiguous(), ids[perm].contiguous(), rw[perm].contiguous(), act)
    assert torch.equal(y_p, y[perm])                                                     # permuted tokens: permuted rows, bit for bit
    for t in (0, 37, 69):                                                                # a token alone: the bits it has inside the batch
        _, y_1, _ = run_grouped(m, x[t:t + 1].contiguous(), ids[t:t + 1].contiguous(), rw[t:t + 1].contiguous(), act)
        assert torch.equal(y_1[0], y[t]), t


def test_zero_routing_weight_contributes_exactly_nothing():
    shape, act, sdt, T = "384x640e5k3", "fp16", "fp16", 33
    H, I, E, k, _ = MO.SHAPES[shape]
    c = MO.case(shape, T, act, sdt)
    m = fused_experts(shape, sdt)
    rw0 = c["rw"].copy()
    rw0[:, 1] = 0.0
    base = run_grouped(m, dev(c["x"], act), dev(c["ids"]), dev(rw0), act)[1]
    for other in range(E):      # swap that slot's expert for any other (the units change): the output keeps its bits
        ids2 = c["ids"].copy()
        ids2[:, 1] = other
        assert torch.equal(run_grouped(m, dev(c["x"], act), dev(ids2), dev(rw0), act)[1], base), other


def test_out_of_range_ids_set_status_and_contribute_zero():
    shape, act, sdt, T = "256x128e8k2", "fp16", "fp16", 33
    H, I, E, k, _ = MO.SHAPES[shape]
    m = fused_experts(shape, sdt)
    c = MO.case(shape, T, act, sdt)
    x, rw = dev(c["x"], act), dev(c["rw"])
    _, clean, st = run_grouped(m, x, dev(c["ids"]), rw, act)
    assert st == 0
    bad = c["ids"].copy()
    bad[1, 0], bad[20, 1] = -1, E
    _, y, st = run_grouped(m, x, dev(bad), rw, act)
    assert st == 1
    keep = [t for t in range(T) if t not in (1, 20)]
    assert torch.equal(y[keep], clean[keep])                       # the other tokens: bit-identical to the clean run
    for t, j_ok in ((1, 1), (20, 0)):                              # the bad slot contributes zero: the token's output is that of its remaining slot
        solo = MO.evaluate(MO.rounded_weights(shape, act, sdt), c["x"][t:t + 1], c["ids"][t:t + 1, j_ok:j_ok + 1], c["rw"][t:t + 1, j_ok:j_ok + 1], act)
        assert MO.rel64(torch_to_f32(y[t:t + 1]), solo["y64"]) <= bar(solo)


@pytest.mark.parametrize("T", [17, 70])
def test_module_grouped_path_equals_the_four_ops(T):
    shape, act, sdt = "384x640e5k3", "fp16", "fp16"
    c = MO.case(shape, T, act, sdt)
    m = grouped_experts(shape, sdt)
    x, ids, rw = dev(c["x"], act), dev(c["ids"]), dev(c["rw"])
    _, want, _ = run_grouped(m, x, ids, rw, act)
    got = m(x, ids.long(), rw.to(TDT[act]))                        # what HF hands it: int64 indices, routing weights in the activation dtype
    assert torch.equal(got, want)
    assert MO.rel64(torch_to_f32(got), c["y64"]) <= bar(c)
    m.check_status()
    # an eager call at another T shares the grow-only buffer set
    m(x[:5].contiguous(), ids[:5].long(), rw[:5].to(TDT[act]))
    assert len(m._grouped_eager) == 1 and len(m._grouped_captured) == 0
    # out-of-range ids: check_status(), never forward()
    bad = ids.clone()
    bad[2, 0] = m.num_experts
    m(x, bad.long(), rw)
    with pytest.raises(IndexError, match="out of range"):
        m.check_status()
    m.check_status()                                               # cleared


def test_module_default_keeps_the_host_loop_at_seventeen_tokens():
    shape, act, sdt, T = "256x128e8k2", "fp16", "fp16", 17
    c = MO.case(shape, T, act, sdt)
    m = fused_experts(shape, sdt)
    assert m.grouped_routing is False
    x, ids, rw = dev(c["x"], act), dev(c["ids"]).long(), dev(c["rw"]).to(TDT[act])
    assert torch.equal(m(x, ids, rw), m._forward_loop(x, ids, rw))


def test_forward_is_captured_at_thirty_three_tokens_and_replays_with_new_routing():
    shape, act, sdt, T = "256x128e8k2", "fp16", "fp16", 33
    H, I, E, k, _ = MO.SHAPES[shape]
    m = fused_experts(shape, sdt)                                   # the default flag: under capture T > 16 takes the grouped path
    assert m.grouped_routing is False
    xs = [dev(MO.make_x(400 + i, T, H, act), act) for i in range(3)]
    routes = [MO.make_routing(500 + i, T, E, k, act) for i in range(3)]
    eager = [run_grouped(m, x, dev(i), dev(w), act)[1] for x, (i, w) in zip(xs, routes)]
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
    assert len(m._grouped_captured) == 1


def test_fuse_moe_experts_with_grouped_routing_on_a_synthetic_block():
    from gptqmodel_amd.nn_modules.moe import HipMoeExperts
    from gptqmodel_amd.utils.moe import fuse_moe_experts
    shape, act, T = "384x640e5k3", "fp16", 40
    H, I, E, k, _ = MO.SHAPES[shape]
    blk = _block(shape, ("gate_proj", "up_proj", "down_proj"))
    assert fuse_moe_experts(blk, grouped_routing=True) is True and isinstance(blk.experts, HipMoeExperts) and blk.experts.grouped_routing is True
    x = dev(MO.make_x(92, T, H, act), act)
    with torch.no_grad():
        got = blk(x)
        probs = torch.softmax(blk.gate(x).float(), dim=-1)
        wts, idx = torch.topk(probs, k, dim=-1)
        wts = (wts / wts.sum(dim=-1, keepdim=True)).half()
    blk.experts.check_status()
    assert len(blk.experts._grouped_eager) == 1                    # (served by the grouped path, not the host loop)
    ref = MO.evaluate(MO.rounded_weights(shape, act, "fp16"), torch_to_f32(x), idx.cpu().numpy().astype(np.int32), torch_to_f32(wts), act)
    e = MO.rel64(torch_to_f32(got), ref["y64"])
    print(f"block T={T}: grouped {e:.3e} (bar {bar(ref):.3e})")
    assert e <= bar(ref), (e, bar(ref))
    blk2 = _block(shape, ("gate_proj", "up_proj", "down_proj"))
    assert fuse_moe_experts(blk2, grouped_routing=False) is True and blk2.experts.grouped_routing is False
