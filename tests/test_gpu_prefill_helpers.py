"""The three small kernels that run before and after the prefill GEMM, each against a plain reference at the shapes where they take another
path (tests/prefill_helper_model.py names the shapes and tests/test_prefill_helper_model_cpu.py shows what they reach and that the bars are
attainable):

  rmsnorm_gather_kernel<ACT, R, IT>   all five (R, IT) instantiations with partly live and wholly dead pieces, later trips of the grid-stride
                                      loop, eps from a rounding detail to the deciding term, rows from all-zero to the top of the dtype's range
                                      -- against O.rmsnorm_ref, <= 2 ulps of the 16-bit dtype and <= 1e-3 of the elements differing
  gather_cols_lds_kernel<R, IT>,      the act-order gather on raw 16-bit patterns, bit for bit; the simple kernel by both of its conditions and in
  gather_cols_kernel                  its second row-loop trip
  splitk_reduce_kernel<ACT, SP>       SP = 7 and the generic body (9 .. 25 slabs: batches of eight and remainders) through forced split-K plans

Every test prints the figures it asserts on (pytest -s shows them)."""
import numpy as np
import pytest
import torch

import prefill_helper_model as P
from helpers import assert_forward_close, f32_to_torch, rel_err, synth_gptq, torch_to_bits, torch_to_f32
from oracle import gptq_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ops():
    from gptqmodel_amd import ops as _ops
    return _ops


def _perm_t(perm):
    return None if perm is None else torch.from_numpy(np.ascontiguousarray(perm, dtype=np.int32)).to(DEV)


def _norm(ops, h, w, eps, act, perm=None):
    return ops.rmsnorm_gather(f32_to_torch(h, act, DEV), f32_to_torch(w, act, DEV), eps, _perm_t(perm))


def _ref_bits(h, w, eps, act, chunk=1024):
    """O.rmsnorm_ref on the whole [M, K] array (it reduces over the last axis), in row chunks to bound the float64 temporaries."""
    return np.concatenate([P.bits16(O.rmsnorm_ref(h[i:i + chunk], w, eps, act), act) for i in range(0, h.shape[0], chunk)])


def _hold_to_bar(got_bits, ref_bits, tag):
    worst, fraction = P.distance(got_bits, ref_bits)
    print(f"{tag}: worst {worst} ulps, {fraction:.2e} of {got_bits.size} elements differ")
    assert worst <= P.BAR_ULPS, f"{tag}: max distance {worst} ulps"
    assert fraction <= P.BAR_FRACTION, f"{tag}: {fraction:.2e} of the elements differ"
    return worst, fraction


def _act_order_perm(K, seed):
    """The permutation an act-order checkpoint brings: stable argsort of a synth_gptq g_idx."""
    gs = 128 if K % 128 == 0 else 8
    return O.act_order_perm(synth_gptq(seed, 4, K, 8, gs, desc_act=True)[3])


# ---- RMSNorm + gather ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", P.ACTS)
@pytest.mark.parametrize("K", P.K_LIST)
def test_rmsnorm_gather_every_instantiation_and_mask_state(ops, act, K):
    """Every K of the list at M = 1, 3, R + 1 and 9, with a permutation and without: the bar against O.rmsnorm_ref; the permuted output is the plain
    one gathered, bit for bit; an identity permutation gives the bits of perm = None.  K = 3584 and 11008 take the permutation of an act-order
    checkpoint, the others a random one."""
    h, w = P.plain_case(P.VARIANT_ROWS, K, act)
    ref = _ref_bits(h, w, 1e-5, act)
    perm = _act_order_perm(K, K) if K in (3584, 11008) else np.random.RandomState(K).permutation(K).astype(np.int32)
    assert sorted(perm.tolist()) == list(range(K))
    for M in P.variant_rows_of(K):
        g = P.norm_geometry(M, K)
        plain = torch_to_bits(_norm(ops, h[:M], w, 1e-5, act))
        _hold_to_bar(plain, ref[:M], f"{act} K={K} M={M} <{g.R},{g.IT}>")
        gathered = torch_to_bits(_norm(ops, h[:M], w, 1e-5, act, perm))
        assert np.array_equal(gathered, plain[:, perm]), (act, K, M, "permuted output != plain output gathered")
        identity = torch_to_bits(_norm(ops, h[:M], w, 1e-5, act, np.arange(K)))
        assert np.array_equal(identity, plain), (act, K, M, "identity permutation != perm None")


_trip_ref = {}


def _trip_case(M, K, act):
    """Inputs, permutation and reference bits of one loop-trip shape: computed once and shared."""
    if (M, K, act) not in _trip_ref:
        h, w = P.plain_case(M, K, act)
        perm = np.random.RandomState(M + K).permutation(K).astype(np.int32)
        ref = _ref_bits(h, w, 1e-5, act)[:, perm]
        ref.setflags(write=False)
        _trip_ref[(M, K, act)] = (h, w, perm, ref)
    return _trip_ref[(M, K, act)]


@pytest.mark.parametrize("act", P.ACTS)
@pytest.mark.parametrize("M,K", P.TRIP_SHAPES)
def test_rmsnorm_gather_later_trips_of_the_row_loop(ops, act, M, K):
    """More passes than blocks: request(m_next), the reuse of red[] and rows[], and the row clamp in a pass of a later trip that has fewer than R
    live rows.  ALL rows against the reference; a second run bit-equal; and single rows run alone (M = 1) give the bits they have inside the
    big call -- the rows of a pass share red[] and rows[], this is the check that they do not leak into each other."""
    h, w, perm, ref = _trip_case(M, K, act)
    g = P.norm_geometry(M, K)
    assert g.trips >= 2 and P.short_pass_in_later_trip(g, M)
    ht, wt, pt = f32_to_torch(h, act, DEV), f32_to_torch(w, act, DEV), _perm_t(perm)
    out = ops.rmsnorm_gather(ht, wt, 1e-5, pt)
    again = ops.rmsnorm_gather(ht, wt, 1e-5, pt)
    assert torch.equal(out, again)
    got = torch_to_bits(out)
    _hold_to_bar(got, ref, f"{act} M={M} K={K} <{g.R},{g.IT}> trips={g.trips}")
    per_trip = g.grid * g.R
    rows = sorted({0, g.R - 1, per_trip - 1, per_trip, per_trip + 1, (g.trips - 1) * per_trip, M - 2, M - 1})
    assert rows[-1] == M - 1
    assert {P.trip_of_row(g, m) for m in rows} == set(range(g.trips))
    for m in rows:
        alone = torch_to_bits(ops.rmsnorm_gather(ht[m:m + 1].contiguous(), wt, 1e-5, pt))
        assert np.array_equal(alone[0], got[m]), (act, M, K, f"row {m} (trip {P.trip_of_row(g, m)}) differs from the same row run alone")


@pytest.mark.parametrize("act", P.ACTS)
@pytest.mark.parametrize("K", P.EPS_K)
@pytest.mark.parametrize("eps", P.EPS_LIST)
def test_rmsnorm_gather_eps_and_dynamic_range(ops, act, K, eps):
    """eps = 1e-6 (Qwen), 1e-5, 1e-3 on thirteen rows, one per family (prefill_helper_model.family_case): eps from 1e-2 to 100 times the mean
    square, a massive-activation row, +0 and -0 padding rows, a one-hot row, a 2^-14 .. 2^10 span, the top of the range, a tiny row, a plain
    one; weights with negative, large and near-zero entries.  The bar holds for EVERY family on its own, so that a quiet family cannot hide
    behind a loud one.  A NaN and an inf in two extra rows leave the bits of the other rows alone.
    Left out on purpose (the docstring of family_case says why): bf16 subnormal inputs / fp32-denormal squares, and bf16 rows whose fp32 sum of
    squares overflows while their mean does not."""
    h, w = P.family_case(K, act, eps)
    ref = _ref_bits(h, w, eps, act)
    perm = np.random.RandomState(K + 1).permutation(K).astype(np.int32)
    got = torch_to_bits(_norm(ops, h, w, eps, act))
    failures = []
    for f, name in enumerate(P.FAMILIES):
        worst, fraction = P.distance(got[f], ref[f])
        print(f"{act} K={K} eps={eps:g} {name}: worst {worst} ulps, {fraction:.2e} of {K} elements differ")
        if not P.meets_bar(worst, fraction):
            failures.append((name, worst, fraction))
    assert not failures, (act, K, eps, failures)
    assert np.array_equal(torch_to_bits(_norm(ops, h, w, eps, act, perm)), got[:, perm])
    # poisoned neighbours: rows 13 (a NaN) and 14 (an inf) share passes with row 12 (R = 4 and R = 2 alike)
    h2 = np.concatenate([h, P.poisoned_rows(K, act)])
    got2 = torch_to_bits(_norm(ops, h2, w, eps, act))
    assert np.array_equal(got2[:P.FAMILY_ROWS], got), (act, K, eps, "a NaN / inf row changed its neighbours")


# ---- the act-order gather ----------------------------------------------------------------------------------------------------------------------
def _gather_case(ops, M, K, seed):
    """Random 16-bit PATTERNS through gather_cols against x[:, perm]; the first row starts with -0, +-inf, NaNs with payloads and the smallest
    subnormal of either dtype: nothing is a number here."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-32768, 32768, (M, K), generator=g, dtype=torch.int32).to(torch.int16)
    x[0, :8] = torch.tensor([0x8000, 0x7C00, 0xFC00, 0x7E01, 0xFFFF, 0x7F80, 0x7FC1, 0x0001], dtype=torch.int32).to(torch.int16)
    x = x.to(DEV)
    perm = torch.randperm(K, generator=g).to(torch.int32).to(DEV)
    out = ops.gather_cols(x, perm)
    assert torch.equal(out, x[:, perm.long()]), (M, K, P.gather_geometry(M, K))


@pytest.mark.parametrize("K", P.K_LIST)
def test_gather_cols_lds_every_instantiation_bit_exact(ops, K):
    for M in P.GATHER_LDS_ROWS:
        assert P.gather_geometry(M, K).kernel == "lds"
        _gather_case(ops, M, K, 17 * K + M)


@pytest.mark.parametrize("M,K", P.TRIP_SHAPES)
def test_gather_cols_lds_later_trips_of_the_row_loop(ops, M, K):
    g = P.gather_geometry(M, K)
    assert g.kernel == "lds" and g.trips >= 2 and P.short_pass_in_later_trip(g, M)
    _gather_case(ops, M, K, M + K)


@pytest.mark.parametrize("M,K", P.GATHER_SIMPLE_SHAPES)
def test_gather_cols_simple_kernel_bit_exact(ops, M, K):
    """Fewer than 8 rows, or rows longer than the LDS kernel stages (Llama-70B's down_proj has K = 28672); 1030 rows: the second trip of the loop
    `m += gridDim.y`."""
    assert P.gather_geometry(M, K).kernel == "simple"
    _gather_case(ops, M, K, 3 * M + K)


def test_act_order_gemm_beyond_the_lds_gather_limit(ops):
    """An act-order layer whose K is beyond the LDS gather's limit through ops.gemm: the simple gather in front of the prefill kernel."""
    K, N, gs, M, act = 16512, 32, 128, 40, "fp16"
    assert P.gather_geometry(M, K).kernel == "simple"
    qweight, qzeros, scales, g_idx = synth_gptq(16512, 4, K, N, gs, desc_act=True)
    x = O.round_to(np.random.RandomState(40).randn(M, K).astype(np.float32) * 0.5, act)
    sc = f32_to_torch(scales, "fp16", DEV)
    perm = _perm_t(O.act_order_perm(g_idx))
    qw_t, meta = ops.repack_tiled(torch.from_numpy(qweight).to(DEV), torch.from_numpy(qzeros).to(DEV), sc, perm, gs, 4)
    try:
        ops.set_tuning(0, 2, 0)
        plan = ops.plan_describe(M, K, N, gs, 4, True)
        assert plan.startswith("tiled") and plan.endswith("gather=1"), plan
        out = ops.gemm(f32_to_torch(x, act, DEV), qw_t, meta, None, perm, N, gs, 4, sc.dtype)
    finally:
        ops.set_tuning(0, 0, 0)
    assert_forward_close(torch_to_f32(out), O.forward_gptq(x, qweight, qzeros, scales, g_idx, 4, None, act, "fp16"), act, tag=plan)


# ---- split-K reduce ----------------------------------------------------------------------------------------------------------------------------
def _splitk_layer(split, act):
    M, N, gs = P.SPLITK_SHAPE
    K = 128 * split
    qweight, qzeros, scales, g_idx = synth_gptq(2600 + split, 4, K, N, gs)
    rng = np.random.RandomState(split)
    x = O.round_to(rng.randn(M, K).astype(np.float32) * 0.5, act)
    bias = O.round_to(rng.randn(N).astype(np.float32) * 0.1, act)
    return M, K, N, gs, (qweight, qzeros, scales, g_idx), x, bias


def _tiled(ops, layer, gs):
    qweight, qzeros, scales, _ = layer
    sc = f32_to_torch(scales, "fp16", DEV)
    return ops.repack_tiled(torch.from_numpy(qweight).to(DEV), torch.from_numpy(qzeros).to(DEV), sc, None, gs, 4) + (sc.dtype,)


@pytest.mark.parametrize("act", P.ACTS)
@pytest.mark.parametrize("split", P.SPLITK_SPLITS)
def test_split_k_reduce_sp7_and_generic_body(ops, act, split):
    """One 128-row chunk of K per slab, `split` slabs: the rounded output with bias against the oracle, two runs bit-equal, and the unrounded fp32
    sums (partial_f32) against the float64 product of x and the oracle's dequantised weights at the project's bar for fp32 partials (1e-5)."""
    M, K, N, gs, layer, x, bias = _splitk_layer(split, act)
    qw_t, meta, sdt = _tiled(ops, layer, gs)
    xt, bt = f32_to_torch(x, act, DEV), f32_to_torch(bias, act, DEV)
    try:
        ops.set_tuning(split, 2, 0)
        plan = ops.plan_describe(M, K, N, gs)
        assert plan.startswith("tiled") and f"splits={split} " in plan, plan
        outs = [ops.gemm(xt, qw_t, meta, bt, None, N, gs, 4, sdt) for _ in range(2)]
        parts = [ops.gemm(xt, qw_t, meta, None, None, N, gs, 4, sdt, partial_f32=True) for _ in range(2)]
    finally:
        ops.set_tuning(0, 0, 0)
    assert torch.equal(outs[0], outs[1]) and torch.equal(parts[0], parts[1])
    assert_forward_close(torch_to_f32(outs[0]), O.forward_gptq(x, *layer, 4, bias, act, "fp16"), act, tag=(split, plan))
    wq = O.dequant_gptq(*layer, 4, "fp16")
    if act != "fp16":
        wq = O.round_to(wq, act)         # the reference casts its weights to the activation dtype (O.forward_gptq)
    exact = x.astype(np.float64) @ wq.astype(np.float64)
    e = rel_err(parts[0].cpu().numpy().astype(np.float64), exact)
    print(f"{act} split={split} ({P.generic_reduce_trips(split) if split > 8 else 'SP=7'}): fp32 partials rel err {e:.2e}")
    assert parts[0].dtype == torch.float32 and e <= 1e-5, (split, e)


@pytest.mark.parametrize("act", P.ACTS)
def test_split_k_generic_body_same_bits_whatever_the_tile(ops, act):
    """The geometry property of test_tile_geometry_does_not_change_a_single_bit on the generic reduce body (12 slabs: a batch of eight and a
    remainder of three): 64-, 128-, 32- and 96-row tiles and 64-row tiles of 128-column blocks give the same bits."""
    split = 12
    M, K, N, gs, layer, x, bias = _splitk_layer(split, act)
    qw_t, meta, sdt = _tiled(ops, layer, gs)
    xt, bt = f32_to_torch(x, act, DEV), f32_to_torch(bias, act, DEV)
    outs = {}
    try:
        for variant in (3, 2, 32, 96, 1064):
            ops.set_tuning(split, 2, variant)
            plan = ops.plan_describe(M, K, N, gs)
            assert f"splits={split} " in plan, plan
            outs[plan.split(" splits=")[0]] = torch_to_bits(ops.gemm(xt, qw_t, meta, bt, None, N, gs, 4, sdt))
    finally:
        ops.set_tuning(0, 0, 0)
    assert len(outs) == 5, sorted(outs)
    first = next(iter(outs.values()))
    for name, o in outs.items():
        assert np.array_equal(o, first), (act, name)
