"""GPU tests of every kernel family over the DYNAMIC RANGE of the WEIGHTS: scales, zero-points and code patterns.

Every other test draws scales as rand * 0.01 + 0.005 -- one and a half binades, positive, normal -- with uniform codes and zero-points.  Here
(tests/helpers.py weight_range_layer): scales made of fp16 subnormals only, a ladder from 2^-14 (bf16: 2^-60) to the largest the reference's
fp16 weights stay finite with (2048 at 4 bits, 64 at 8), exponents that differ between neighbouring groups (group_ramp) and between the 16
lanes of a column tile (column_ramp), one huge group among tiny ones, negative scales, exact +-0 scales; codes within one step of the
zero-point (what a trained checkpoint holds -- and the worst cancellation for the raw-code decode form 5, y = sum_g s_g (2^24 lo_g +
2^20 hi_g - z_g sum x_g)), on the zero-point (every weight 0), and at the ends of the code range with z in {0, max}.

Activations are randn rows times a power of two chosen per row from the float64 product, so that the largest |y_exact| of a row is in
[1, 64] where fp16's normal range of x allows it and in [2^-10, 6e4] always (tests/test_weight_range_families_cpu.py checks that, and that the
reference's weights and outputs are finite): the rounded output of EVERY row is judged.  All waves of a row see one magnitude: the
activation range is tests/test_gpu_decode_dynamic_range.py's job.

References and bars are that file's: y_exact = x64 @ (s64[g] (q - z[g])), y_rw = x64 @ the reference's rounded weights, y_oracle =
O.matmul_round.  fp32 partial sums <= 1e-4 per row (against y_exact for the exact-arithmetic forms, against y_rw for the calls that keep the
reference's per-weight rounding); rounded outputs of the exact forms no further from y_exact than 1.05 x the reference chain or one rounding
of the output dtype; rounded outputs of the per-weight-rounding calls through assert_forward_close (strict_atol for the decode kernel, the
default gate for the prefill kernel).  Shapes are the smallest at which each code path exists (test_shapes_reach_the_code_paths).

Out of scope: non-finite scales; bf16 scales whose weights overflow fp16 activations."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from helpers import (TDT, WEIGHT_RANGE_DECODE_SHAPES, WEIGHT_RANGE_DTYPES, WEIGHT_RANGE_MAIN, WEIGHT_RANGE_TILED, assert_forward_close, f32_to_torch,
                     np_repack_tiled, rel_err, torch_to_bits, torch_to_f32, weight_exact_f64, weight_range_layer, weight_range_layer_of,
                     weight_range_main_families, weight_range_rows, weight_range_side_families, weight_scale_families)
from oracle import gptq_oracle as O

gpu = pytest.mark.gpu
DEV = "cuda:0"
# (GPTQHIP_DECODE_BITFAITHFUL=1 in the environment: every batch-1 call keeps the reference's per-weight rounding -- no exact form to expect)
EXACT_DEFAULT = os.environ.get("GPTQHIP_DECODE_BITFAITHFUL", "0") in ("", "0")
OUT_ROUNDING = {"fp16": 2.0 ** -11, "bf16": 2.0 ** -8}          # one rounding of the output dtype (the bars of test_gpu_decode_forms.py)
FORMS = [-1, 3, 4]
DT_IDS = [f"{a}-s{s}" for a, s in WEIGHT_RANGE_DTYPES]
ENTRIES = [("gemm", 1), ("decode", 1), ("decode", 2), ("decode", 4), ("decode", 16)]


def test_shapes_reach_the_code_paths():
    """Host logic (no GPU): the planner sends every shape of this file where the file says it goes."""
    from gptqmodel_amd import ops
    plan = lambda *a: dict(kv.split("=") for kv in ops.plan_describe(*a).split(" ")[1:])   # noqa: E731
    for name, (bits, K, N, gs, desc) in WEIGHT_RANGE_DECODE_SHAPES.items():
        for M in (1,) if desc else ((1, 2, 4) if name == "2048x8192g128" else (1, 2, 4, 16)):
            d = ops.plan_describe(M, K, N, gs, bits, desc)
            assert d.startswith("skinny launches=1 mt=1 ") and " regular=1 splits=1 " in d, (name, M, d)
            assert ops.decode_supported(K, N, gs, desc, M) == (name != "512x256g128-actorder"), (name, M)
    # act-order: the small layer is gathered in front of the kernel, the 16-chunk one rides the in-kernel permutation (4-deep ring)
    assert plan(1, 512, 256, 128, 4, True)["gather"] == "1" and plan(1, 2048, 1024, 128, 4, True) == dict(plan(1, 2048, 1024, 128, 4, True), gather="0", depth="4")
    # 1408 = 11 chunks over 6 waves x 2: a padded last ring round; 8192 columns = 512 tiles = two per CU, 16 chunks at depth 4: the persistent-tile kernel
    assert plan(1, 1408, 256, 64)["waves"] == "6" and plan(1, 1408, 256, 64)["depth"] == "2" and 6 * 2 > 1408 // 128
    assert 8192 // 16 == 2 * 256 and (2048 // 128) % 4 == 0 and 4 <= (2048 // 128) // 4 <= 16
    assert plan(2, 2048, 8192, 128)["depth"] == plan(4, 2048, 8192, 128)["depth"] == "4" and plan(4, 512, 256, 128)["depth"] == "2"     # 2..4 rows: exact / per-weight
    for M, mt in ((24, "2"), (48, "4")):                                                   # 17..64 rows of the decode kernel
        bits, K, N, gs, _ = WEIGHT_RANGE_DECODE_SHAPES[WEIGHT_RANGE_MAIN]
        assert ops.plan_describe(M, K, N, gs, bits).startswith(f"skinny launches=1 mt={mt} "), M
    want = {"tiled-384x264g128": "tiled bm=48 splits=1 ", "tiled-256x136g64": "tiled bm=64 splits=1 ", "tiled8-256x128g64": "tiled bm=64 splits=1 ",
            "tiled-n128-384x264g128": "tiled bm=64 bn=128 splits=1 ", "tiled-splitk-384x264g128": "tiled bm=64 splits=3 "}
    try:
        for name, (bits, K, N, gs, M, tuning) in WEIGHT_RANGE_TILED.items():
            ops.set_tuning(*tuning)
            assert ops.plan_describe(M, K, N, gs, bits).startswith(want[name]), (name, ops.plan_describe(M, K, N, gs, bits))
    finally:
        ops.set_tuning(0, 0, 0)


@pytest.fixture(scope="module")
def ops():
    from gptqmodel_amd import ops as _ops
    try:
        yield _ops
    finally:
        _ops.set_decode_form(-1)
        _ops.set_tuning(0, 0, 0)


@pytest.fixture(scope="module")
def layers(ops):
    """(shape, scale family, code family, scale dtype) -> the layer, built and repacked once; per activation dtype its rows and the three
    references, once (a case at M rows uses the first M)."""
    cache = {}

    def get(shape, sfam, cfam, sdt):
        key = (shape, sfam, cfam, sdt)
        if key not in cache:
            bits, K, N, gs, rows, (qweight, qzeros, scales, g_idx) = weight_range_layer_of(shape, sfam, cfam, sdt)
            desc = not np.array_equal(g_idx, np.arange(K) // gs)
            sc = f32_to_torch(scales, sdt, DEV)
            perm = torch.from_numpy(O.act_order_perm(g_idx)).to(DEV) if desc else None
            qw_t, meta = ops.repack_tiled(torch.from_numpy(qweight).to(DEV), torch.from_numpy(qzeros).to(DEV), sc, perm, gs, bits)
            cache[key] = SimpleNamespace(bits=bits, K=K, N=N, gs=gs, rows=rows, raw=(qweight, qzeros, scales, g_idx), qw_t=qw_t, meta=meta,
                                         sdt=sc.dtype, scl=sdt, perm=perm, refs={})
        return cache[key]

    return get


def _refs(L, act):
    """-> (x, x64 @ s (q - z), x64 @ the reference's rounded weights, the oracle's rounded output) for L.rows rows."""
    if act not in L.refs:
        qweight, qzeros, scales, g_idx = L.raw
        w_exact = weight_exact_f64(qweight, qzeros, scales, g_idx, L.bits)
        w_rounded = O.round_to(O.dequant_gptq(qweight, qzeros, scales, g_idx, L.bits, L.scl), act)
        x = weight_range_rows(act, w_exact, L.rows, seed=L.K // 128 + L.N // 16)
        x64 = x.astype(np.float64)
        L.refs[act] = (x, x64 @ w_exact, x64 @ w_rounded.astype(np.float64), O.matmul_round(x, w_rounded, None, act).astype(np.float64))
    return L.refs[act]


def _expects_exact(ops, act, sdt, M, form, K, N, gs):
    """Which calls take an exact-arithmetic form (include/gptqhip.h gptqhip_set_decode_form; as _expects_exact of the activation-range file, plus
    the scale dtype, form 3, the group size and the plan).  One group constant per 128-row chunk only.  fp16 x fp16: one row under the default
    (form 5) and under form 3, 2..4 rows (the group-factored dequant of the four-row staging) where the plan has the 4-deep ring -- on short K the
    planner takes the 2-deep ring, whose row staging keeps the per-weight rounding.  bf16 activations: one row under the default (form 5 through
    the f16 matrix pipe); form 3 has no bf16 variant.  fp16 activations with bf16 scales, form 4, more rows and GPTQHIP_DECODE_BITFAITHFUL=1
    keep the reference's per-weight rounding."""
    if gs % 128 != 0 or form == 4 or (form == -1 and not EXACT_DEFAULT):
        return False
    if act == "fp16":
        return sdt == "fp16" and (M == 1 or (M <= 4 and " depth=4 " in ops.plan_describe(M, K, N, gs)))
    return form == -1 and M == 1


def _row_rel_err(got, ref):
    """rel_err of every row on its own (rows of one call must not hide behind the largest)."""
    return max(rel_err(got[m:m + 1], ref[m:m + 1]) for m in range(got.shape[0]))


def _check(tag, act, exact, part, out, y_exact, y_rw, y_oracle, strict_atol=True):
    """part: fp32 partial sums, out: rounded output (float64 copies) of one call pair -> the list of failed bars (every figure is printed)."""
    bad = []
    if not np.isfinite(part).all() or not np.isfinite(out).all():
        return [(tag, "non-finite output")]
    e_exact, e_rw = _row_rel_err(part, y_exact), _row_rel_err(part, y_rw)
    print(f"{tag}: {'exact' if exact else 'per-weight'}: partial f32 rel err {e_exact:.3e} vs the exact product, {e_rw:.3e} vs the rounded weights")
    if (e_exact if exact else e_rw) > 1e-4:
        bad.append((tag, f"partial f32 rel err {e_exact:.3e} vs the exact product, {e_rw:.3e} vs the reference's rounded weights"))
    if not exact:
        try:
            assert_forward_close(out, y_oracle, act, tag=tag, strict_atol=strict_atol)
        except AssertionError as e:
            bad.append((tag, "rounded output", str(e)[:300]))
        return bad
    worst = (0.0, 0.0)
    for m in range(out.shape[0]):                                  # EVERY row: 2^-10 <= max |y_exact| <= 6e4 (the CPU test)
        scale = np.abs(y_exact[m]).max()
        err, err_ref = np.abs(out[m] - y_exact[m]).max() / scale, np.abs(y_oracle[m] - y_exact[m]).max() / scale
        worst = max(worst, (err, err_ref))
        if err > max(err_ref * 1.05, OUT_ROUNDING[act]) + 1e-7:
            bad.append((tag, f"row {m}: rounded output {err:.3e} from the exact product, reference chain {err_ref:.3e}"))
    print(f"{tag}: rounded output at worst {worst[0]:.3e} from the exact product (reference chain there: {worst[1]:.3e})")
    return bad


def _run_decode_entries(ops, L, act, form, entries, tag):
    x, y_exact, y_rw, y_oracle = _refs(L, act)
    bad = []
    for entry, M in entries:
        xd = f32_to_torch(x[:M], act, DEV)
        ops.set_decode_form(form)
        try:
            if entry == "gemm":
                part = ops.gemm(xd, L.qw_t, L.meta, None, L.perm, L.N, L.gs, L.bits, L.sdt, partial_f32=True)
                out = ops.gemm(xd, L.qw_t, L.meta, None, L.perm, L.N, L.gs, L.bits, L.sdt)
            else:
                xin = xd if M > 1 else xd[0]
                part = ops.decode_linear(xin, L.qw_t, L.meta, None, L.K, L.N, L.gs, L.bits, L.sdt, out_glue=ops.OUT_PARTIAL_F32, perm=L.perm, M=M)
                out = ops.decode_linear(xin, L.qw_t, L.meta, None, L.K, L.N, L.gs, L.bits, L.sdt, perm=L.perm, M=M)
            torch.cuda.synchronize()
        finally:
            ops.set_decode_form(-1)
        assert part.dtype == torch.float32 and out.dtype == TDT[act]
        bad += _check(tag + (entry, M), act, _expects_exact(ops, act, L.scl, M, form, L.K, L.N, L.gs), torch_to_f32(part).reshape(M, L.N).astype(np.float64),
                      torch_to_f32(out).reshape(M, L.N).astype(np.float64), y_exact[:M], y_rw[:M], y_oracle[:M])
    assert not bad, bad


MAIN_CASES = [pytest.param(a, s, sf, cf, id=f"{a}-s{s}-{sf}-{cf}") for a, s in WEIGHT_RANGE_DTYPES for sf, cf in weight_range_main_families(a, s)]
SIDE_CASES = [pytest.param(a, s, sf, cf, id=f"{a}-s{s}-{sf}-{cf}") for a, s in WEIGHT_RANGE_DTYPES for sf, cf in weight_range_side_families(s)]


@gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("act,sdt,sfam,cfam", MAIN_CASES)
def test_decode_over_the_weight_range(ops, layers, act, sdt, sfam, cfam, form):
    """The main shape: every scale family and every code family, gptqhip_gemm at one row and the decode op at 1, 2, 4, 16 rows."""
    _run_decode_entries(ops, layers(WEIGHT_RANGE_MAIN, sfam, cfam, sdt), act, form, ENTRIES, (act, sdt, sfam, cfam, form))


@gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("shape", [s for s in WEIGHT_RANGE_DECODE_SHAPES if s != WEIGHT_RANGE_MAIN])
@pytest.mark.parametrize("act,sdt,sfam,cfam", SIDE_CASES)
def test_decode_code_paths_over_the_weight_range(ops, layers, act, sdt, sfam, cfam, shape, form):
    """Four constants per chunk, a padded last ring round, two tiles per CU, the persistent-tile kernel, act-order (gathered / in the kernel)."""
    if shape == "512x256g128-actorder":
        entries = [("gemm", 1)]
    elif shape == "2048x1024g128-actorder":
        entries = [("gemm", 1), ("decode", 1)]
    elif shape == "2048x8192g128":
        entries = ENTRIES[:4]
    else:
        entries = ENTRIES
    _run_decode_entries(ops, layers(shape, sfam, cfam, sdt), act, form, entries, (act, sdt, sfam, cfam, shape, form))


@gpu
@pytest.mark.parametrize("M", [24, 48])
@pytest.mark.parametrize("act,sdt,sfam,cfam", SIDE_CASES)
def test_skinny_17_to_64_rows_over_the_weight_range(ops, layers, act, sdt, sfam, cfam, M):
    _run_decode_entries(ops, layers(WEIGHT_RANGE_MAIN, sfam, cfam, sdt), act, -1, [("gemm", M)], (act, sdt, sfam, cfam, "skinny"))


@gpu
@pytest.mark.parametrize("shape", list(WEIGHT_RANGE_TILED))
@pytest.mark.parametrize("act,sdt,sfam,cfam", SIDE_CASES)
def test_tiled_prefill_over_the_weight_range(ops, layers, act, sdt, sfam, cfam, shape):
    """The MFMA-tiled prefill kernel (4- and 8-bit, a forced 128-column-block plan, a split-K plan): per-weight rounding everywhere; the
    forced plans run twice and must give the same bits."""
    L = layers(shape, sfam, cfam, sdt)
    M, tuning = WEIGHT_RANGE_TILED[shape][4:]
    x, y_exact, y_rw, y_oracle = _refs(L, act)
    xd = f32_to_torch(x, act, DEV)
    bias = O.round_to(np.random.RandomState(3).randn(L.N).astype(np.float32) * 0.1, act)
    try:
        ops.set_tuning(*tuning)
        part = ops.gemm(xd, L.qw_t, L.meta, None, None, L.N, L.gs, L.bits, L.sdt, partial_f32=True)
        outs = [ops.gemm(xd, L.qw_t, L.meta, None, None, L.N, L.gs, L.bits, L.sdt) for _ in range(2)]
        parts2 = ops.gemm(xd, L.qw_t, L.meta, None, None, L.N, L.gs, L.bits, L.sdt, partial_f32=True)
        with_bias = ops.gemm(xd, L.qw_t, L.meta, f32_to_torch(bias, act, DEV), None, L.N, L.gs, L.bits, L.sdt)
        torch.cuda.synchronize()
    finally:
        ops.set_tuning(0, 0, 0)
    assert np.array_equal(torch_to_bits(outs[0]), torch_to_bits(outs[1])) and np.array_equal(torch_to_f32(part), torch_to_f32(parts2))   # fixed reduction order
    tag = (act, sdt, sfam, cfam, shape)
    bad = _check(tag, act, False, torch_to_f32(part).astype(np.float64), torch_to_f32(outs[0]).astype(np.float64), y_exact, y_rw, y_oracle, strict_atol=False)
    assert not bad, bad
    w_rounded = O.round_to(O.dequant_gptq(*L.raw, L.bits, L.scl), act)
    assert_forward_close(torch_to_f32(with_bias), O.matmul_round(x, w_rounded, bias, act), act, tag=tag + ("bias",))


# ---- every weight exactly 0 --------------------------------------------------------------------------------------------------------------
def _zero_layer_calls(ops, L, act, form, bias):
    """-> [(entry, M, exact form?, fp32 partial sums | None, rounded output)] of an at_zero_point layer on plain randn rows."""
    x = _refs(L, act)[0]
    bd = None if bias is None else f32_to_torch(bias, act, DEV)
    res = []
    ops.set_decode_form(form)
    try:
        for entry, M in ENTRIES + [("gemm", 24), ("tiled", 33)]:
            xd = f32_to_torch(x[:M], act, DEV)
            if entry == "tiled":
                ops.set_tuning(0, 2, 0)
            try:
                if entry != "decode":
                    part = ops.gemm(xd, L.qw_t, L.meta, None, None, L.N, L.gs, L.bits, L.sdt, partial_f32=True)
                    out = ops.gemm(xd, L.qw_t, L.meta, bd, None, L.N, L.gs, L.bits, L.sdt)
                else:
                    xin = xd if M > 1 else xd[0]
                    part = ops.decode_linear(xin, L.qw_t, L.meta, None, L.K, L.N, L.gs, L.bits, L.sdt, out_glue=ops.OUT_PARTIAL_F32, M=M)
                    out = ops.decode_linear(xin, L.qw_t, L.meta, bd, L.K, L.N, L.gs, L.bits, L.sdt, M=M)
                torch.cuda.synchronize()
            finally:
                if entry == "tiled":
                    ops.set_tuning(0, 0, 0)
            exact = entry != "tiled" and M <= 16 and _expects_exact(ops, act, L.scl, M, form, L.K, L.N, L.gs)
            res.append((entry, M, exact, torch_to_f32(part).reshape(M, L.N).astype(np.float64), torch_to_f32(out).reshape(M, L.N)))
    finally:
        ops.set_decode_form(-1)
    return x, res


def _cancellation_bound(L, x):
    """The standard fp32 accumulation bound of a sum of K terms that cancel exactly: |part[n]| <= K 2^-24 sum_k |x_k| |s_g(k),n| z_g(k),n
    (the exact forms add s_g x_k q_k and subtract s_g z_g x_k, with q = z: the terms' magnitudes are |x s| z twice, u = 2^-24)."""
    qweight, qzeros, scales, g_idx = L.raw
    g = O.normalize_g_idx(g_idx, scales.shape[0])
    sz = np.abs(np.asarray(scales, np.float64))[g] * O.unpack_cols(qzeros, L.bits).astype(np.float64)[g]
    return L.K * 2.0 ** -24 * (np.abs(x.astype(np.float64)) @ sz)


@gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("sfam", ["u0.01", "signed", "group_ramp", "zero_groups"])
@pytest.mark.parametrize("act,sdt", WEIGHT_RANGE_DTYPES, ids=DT_IDS)
def test_at_zero_point_gives_exactly_the_bias(ops, layers, act, sdt, sfam, with_bias, form):
    """Every code on its zero-point: the reference's output is the bias, bit for bit.  The calls that keep the per-weight rounding must return exactly
    that (and exactly 0 as fp32 partial sums); the exact-arithmetic forms cancel s (sum x q - z sum x) in fp32 and are held to the fp32 accumulation
    bound of _cancellation_bound -- derived, not measured; the observed share of it is printed."""
    L = layers(WEIGHT_RANGE_MAIN, sfam, "at_zero_point", sdt)
    bias = O.round_to(np.random.RandomState(3).randn(L.N).astype(np.float32) * 0.1, act) if with_bias else None
    x, res = _zero_layer_calls(ops, L, act, form, bias)
    want = np.zeros(L.N, np.float32) if bias is None else bias
    bad = []
    for entry, M, exact, part, out in res:
        if not np.isfinite(part).all() or not np.isfinite(out).all():
            bad.append((entry, M, "non-finite"))
        elif not exact:
            if part.any() or not np.array_equal(out, np.broadcast_to(want, out.shape)):
                bad.append((entry, M, "per-weight rounding: not exactly the bias", float(np.abs(part).max()), float(np.abs(out - want).max())))
        else:
            bound = _cancellation_bound(L, x[:M])
            ratio = float((np.abs(part) / np.maximum(bound, 1e-300)).max())
            print(f"{(act, sdt, sfam, with_bias, form, entry, M)}: exact form, |partial| at most {ratio:.3e} of the fp32 accumulation bound (largest {np.abs(part).max():.3e})")
            if ratio > 1.0:
                bad.append((entry, M, "exact form: outside the fp32 accumulation bound", ratio))
            # the rounded output: the bias plus at most that residue, rounded once
            lim = bound * 1.01 + np.abs(want)[None, :] * OUT_ROUNDING[act] + 2.0 ** -24
            if (np.abs(out.astype(np.float64) - want[None, :]) > lim).any():
                bad.append((entry, M, "exact form: rounded output further from the bias than the bound"))
    assert not bad, bad


# Inherent to decode form 5 (the issue's section 4: exactly these parametrisations, strict, figures beside them): under the
# default form on fp16 x fp16 and bf16 x bf16 the one-row calls cancel s (2^24 lo + 2^20 hi - z sum x) in fp32 on the groups that sit on their
# zero-points.  Measured on an MI355X: kernel error -- largest |fp32 partial sum| 7.04e-06 (fp16) / 2.31e-06 (bf16), i.e. 5.9e-02 / 1.9e-02 of the
# accumulation bound of _cancellation_bound; rounded output 7.03e-06 / 2.31e-06 from 0 and 7.63e-06 / 0 from the bias.  Reference-chain error: 0.
FORM5_RESIDUE = pytest.mark.xfail(condition=EXACT_DEFAULT, strict=True, reason="decode form 5 leaves fp32 cancellation noise on an all-zero layer")
ZERO_SCALE_PARAMS = [pytest.param(a, s, b, f, id=f"{a}-s{s}-{b}-{f}", marks=[FORM5_RESIDUE] if f == -1 and (a == "bf16" or s == "fp16") else [])
                     for a, s in WEIGHT_RANGE_DTYPES for b in (False, True) for f in FORMS]


@gpu
@pytest.mark.parametrize("act,sdt,with_bias,form", ZERO_SCALE_PARAMS)
def test_zero_scales_give_exactly_zero(ops, layers, act, sdt, with_bias, form):
    """zero_groups x at_zero_point: a quarter of the groups have scale +-0 and uniform codes, the others sit on their zero-points -- every weight
    is 0 and every form must return exactly 0 (exactly the bias): a zero scale times anything finite is zero, and no NaN from 0 x inf.

    Expected to fail (strict) under the default form (-1) where it resolves to form 5 -- [fp16-sfp16-*--1] and [bf16-sbf16-*--1], at gptqhip_gemm M = 1 and
    the decode op M = 1: the zero-scale groups do contribute exactly 0, but on the groups that sit on their zero-points form 5 cancels
    s (2^24 lo + 2^20 hi - z sum x) in fp32 and leaves rounding noise.  Measured (MI355X): largest |fp32 partial sum| 7.04e-06 (fp16) / 2.31e-06
    (bf16) = 5.9e-02 / 1.9e-02 of the accumulation bound of _cancellation_bound; rounded output 7.03e-06 / 2.31e-06 from 0, 7.63e-06 / 0 from the
    bias; the reference chain gives exactly 0 (its error is 0).  Forms 3 and 4, 2..48 rows and the prefill kernel return exactly 0.  Inherent to
    the form; test_at_zero_point_gives_exactly_the_bias[*zero_groups*] holds the same calls to the derived bound."""
    L = layers(WEIGHT_RANGE_MAIN, "zero_groups", "at_zero_point", sdt)
    bias = O.round_to(np.random.RandomState(3).randn(L.N).astype(np.float32) * 0.1, act) if with_bias else None
    x, res = _zero_layer_calls(ops, L, act, form, bias)
    want = np.zeros(L.N, np.float32) if bias is None else bias
    bad = []
    for entry, M, exact, part, out in res:
        bound = _cancellation_bound(L, x[:M])
        print(f"{(act, sdt, with_bias, form, entry, M)}: {'exact' if exact else 'per-weight'}: largest |partial| {np.abs(part).max():.3e} "
              f"({float((np.abs(part) / np.maximum(bound, 1e-300)).max()):.3e} of the fp32 accumulation bound of the non-zero groups), largest |out - bias| {np.abs(out - want).max():.3e}")
        if not np.isfinite(part).all() or not np.isfinite(out).all():
            bad.append((entry, M, "non-finite"))
        elif part.any() or not np.array_equal(out, np.broadcast_to(want, out.shape)):
            bad.append((entry, M, "exact" if exact else "per-weight", float(np.abs(part).max()), float(np.abs(out - want).max())))
    assert not bad, bad


# ---- integer and rounding work, bit for bit ----------------------------------------------------------------------------------------------
BITEXACT_SHAPES = [(4, 512, 256, 128), (8, 256, 128, 64)]


def _bit_families(sdt, bits):
    names = []
    for act, s in WEIGHT_RANGE_DTYPES:
        if s == sdt:
            names += [n for n in weight_scale_families(act, sdt, bits) if n not in names]
    return names


@gpu
@pytest.mark.parametrize("desc", [False, True])
@pytest.mark.parametrize("bits,K,N,gs", BITEXACT_SHAPES)
@pytest.mark.parametrize("sdt", ["fp16", "bf16"])
def test_repack_tiled_bit_exact_on_the_families(ops, sdt, bits, K, N, gs, desc):
    """gptqhip_repack_tiled packs the raw scale bits beside 0xE400 | z: sign bit set, subnormal exponent field, z in {0, max}, every family."""
    for sfam in _bit_families(sdt, bits):
        for cfam in ("random", "extremes"):
            qweight, qzeros, scales, g_idx = weight_range_layer(sfam, cfam, bits, K, N, gs, sdt, desc_act=desc, seed=17)
            sc = f32_to_torch(scales, sdt, DEV)
            perm_np = O.act_order_perm(g_idx) if desc else None
            perm = torch.from_numpy(perm_np).to(DEV) if desc else None
            qw_t, meta = ops.repack_tiled(torch.from_numpy(qweight).to(DEV), torch.from_numpy(qzeros).to(DEV), sc, perm, gs, bits)
            e_qw, e_meta = np_repack_tiled(qweight, qzeros, torch_to_bits(sc), perm_np, gs, bits)
            assert np.array_equal(qw_t.cpu().numpy(), e_qw), (sfam, cfam)
            assert np.array_equal(meta.cpu().numpy(), e_meta), (sfam, cfam)
            _, meta2 = ops.repack_tiled(None, torch.from_numpy(qzeros).to(DEV), sc, None, gs, bits)
            assert np.array_equal(meta2.cpu().numpy(), e_meta), (sfam, cfam)


@gpu
@pytest.mark.parametrize("desc", [False, True])
@pytest.mark.parametrize("bits,K,N,gs", BITEXACT_SHAPES)
@pytest.mark.parametrize("sdt", ["fp16", "bf16"])
def test_dequant_kernels_bit_exact_on_the_families(ops, sdt, bits, K, N, gs, desc):
    """gptqhip_dequant, gptqhip_dequant_tiled and gptqhip_embedding against O.dequant_gptq as bit patterns (signed zeros included), every scale
    family x {uniform, near-zero-point, extreme} codes."""
    bad = []
    ids = torch.from_numpy(np.random.RandomState(2).permutation(K)[:64].astype(np.int64)).to(DEV)
    for sfam in _bit_families(sdt, bits):
        for cfam in ("random", "near_zero_point", "extremes"):
            qweight, qzeros, scales, g_idx = weight_range_layer(sfam, cfam, bits, K, N, gs, sdt, desc_act=desc, seed=23)
            want = O.dequant_gptq(qweight, qzeros, scales, g_idx, bits, sdt)
            want = want.astype(np.float16).view(np.uint16) if sdt == "fp16" else O.bf16_bits(want)
            qw, qz, sc = torch.from_numpy(qweight).to(DEV), torch.from_numpy(qzeros).to(DEV), f32_to_torch(scales, sdt, DEV)
            perm = torch.from_numpy(O.act_order_perm(g_idx)).to(DEV) if desc else None
            qw_t, meta = ops.repack_tiled(qw, qz, sc, perm, gs, bits)
            inv = None
            if desc:
                inv = torch.empty_like(perm)
                inv[perm.long()] = torch.arange(K, dtype=torch.int32, device=DEV)
            got = {"dequant": torch_to_bits(ops.dequant(qw, qz, sc, torch.from_numpy(g_idx).to(DEV), gs, bits)),
                   "dequant_tiled": torch_to_bits(ops.dequant_tiled(qw_t, meta, perm, K, N, gs, bits, sc.dtype)),
                   "embedding": torch_to_bits(ops.embedding(ids, qw_t, meta, inv, K, N, gs, bits, sc.dtype))}
            for name, g in got.items():
                w = want[ids.cpu().numpy()] if name == "embedding" else want
                if not np.array_equal(g, w):
                    d = g != w
                    i = tuple(np.argwhere(d)[0])
                    bad.append((name, sfam, cfam, int(d.sum()), f"first at {i}: got {int(g[i]):#06x} want {int(w[i]):#06x}"))
    assert not bad, bad
