"""CPU checks of the weight-side dynamic-range families of tests/helpers.py (weight_range_layer / weight_range_rows) and of the oracle at
those ranges -- what tests/test_gpu_weight_dynamic_range.py leans on:

  * the tensors are what the family names say (subnormal-only scales, the exponent spread of group_ramp, the share of zero scales,
    the code sets);
  * O.dequant_gptq equals torch CPU arithmetic -- scales[g] * (codes - zeros[g]) in the scale dtype, then the cast to each activation
    dtype -- bit for bit, signed zeros included: the oracle is the reference's arithmetic where no golden fixture reaches;
  * for every case the GPU tests run, the reference's rounded weights and O.forward_gptq are finite and every activation row's largest
    |y_exact| lies in [2^-10, 6e4] -- the GPU tests judge the rounded output of EVERY row (at_zero_point: y_exact = 0 by construction)."""
import numpy as np
import pytest
import torch

from helpers import (TDT, WEIGHT_CODE_FAMILIES, WEIGHT_RANGE_DECODE_SHAPES, WEIGHT_RANGE_DTYPES, WEIGHT_RANGE_MAIN, WEIGHT_RANGE_TILED,
                     bits_to_torch, f32_to_torch, torch_to_bits, weight_exact_f64, weight_range_layer, weight_range_layer_of,
                     weight_range_main_families, weight_range_rows, weight_range_side_families, weight_scale_families, weight_scale_top)
from oracle import gptq_oracle as O

SMALL = {4: (512, 256, 128), 8: (256, 128, 64)}         # the 4-bit main shape and the 8-bit shape of the GPU tests


def _bits(a_f32, dtype):
    return np.asarray(a_f32, np.float32).astype(np.float16).view(np.uint16) if dtype == "fp16" else O.bf16_bits(a_f32)


def _in_binade(s, base):
    """base <= s <= 2 base up to one rounding of the scale dtype."""
    s = s.astype(np.float64)
    return bool((s >= base * (1 - 2.0 ** -8)).all() and (s <= 2 * base * (1 + 2.0 ** -8)).all())


def _all_scale_families(sdt, bits):
    names = []
    for act, s in WEIGHT_RANGE_DTYPES:
        if s == sdt:
            names += [n for n in weight_scale_families(act, sdt, bits) if n not in names]
    return names


@pytest.mark.parametrize("bits", [4, 8])
@pytest.mark.parametrize("sdt", ["fp16", "bf16"])
def test_scale_families_are_what_they_say(sdt, bits):
    K, N, gs = SMALL[bits]
    G = K // gs
    names = _all_scale_families(sdt, bits)
    assert {"group_ramp", "column_ramp", "outlier_group", "signed", "zero_groups", "u0.001", "u0.01", "u1", f"u{weight_scale_top(bits):g}"} <= set(names)
    assert ("sub" in names) == (sdt == "fp16") and ("u2^-14" in names) and (sdt == "fp16" or {"u2^-60", "u2^60", "u2^-24"} <= set(names))
    for fam in names:
        _, _, s, _ = weight_range_layer(fam, "random", bits, K, N, gs, sdt, seed=3)
        assert s.shape == (G, N) and s.dtype == np.float32 and np.isfinite(s).all()
        assert np.array_equal(O.round_to(s, sdt), s), fam                         # exactly representable in the scale dtype
        if fam == "sub":
            n = s.astype(np.float64) * 2.0 ** 24
            assert np.array_equal(n, np.rint(n)) and n.min() >= 1 and n.max() <= 1023 and len(np.unique(n)) > 0.3 * min(n.size, 1023)      # fp16 subnormals only
        elif fam.startswith("u"):
            m = 2.0 ** int(fam[3:]) if fam.startswith("u2^") else float(fam[1:])
            assert (s >= np.float32(m) * (1 - 2.0 ** -8)).all() and (s <= 2 * m * (1 + 2.0 ** -8)).all() and s.max() > 1.9 * m and s.min() < 1.1 * m, fam
            assert ((2 ** bits - 1) * s.astype(np.float64)).max() <= 65504.0 or (sdt == "bf16" and fam == "u2^60")
        elif fam == "group_ramp":
            assert _in_binade(s, 0.01 * 2.0 ** (((7 * np.arange(G)) % 21) - 10.0)[:, None]), fam
        elif fam == "column_ramp":
            assert _in_binade(s, 0.01 * 2.0 ** ((np.arange(N) % 16) - 8.0)[None, :]), fam
        elif fam == "outlier_group":
            big = s >= weight_scale_top(bits)
            assert (big.sum(axis=0) == 1).all() and (s[~big] <= 2.0 ** -19).all() and (s[~big] >= 2.0 ** -20).all() and (s[big] <= 2 * weight_scale_top(bits)).all()
        elif fam == "signed":
            neg = np.signbit(s).mean()
            assert 0.4 < neg < 0.6 and _in_binade(np.abs(s), 0.01)
        elif fam == "zero_groups":
            zero = s == 0.0
            assert 0.18 < zero.mean() < 0.32 and np.signbit(s[zero]).any() and not np.signbit(s[zero]).all() and _in_binade(s[~zero], 0.01)
    # group_ramp: (7 g) mod 21 - 10 walks -10, -3, 4: neighbouring groups 2^7 and 2^14 apart (K = 512 at group size 128 already has all three)
    _, _, s, _ = weight_range_layer("group_ramp", "random", 4, 512, 256, 32, sdt)
    e = np.floor(np.log2(s[:, 0].astype(np.float64) / 0.0099))
    assert e.max() - e.min() == 14 and np.abs(np.diff(e)).max() == 14 and np.abs(np.diff(e)).min() == 7


@pytest.mark.parametrize("bits", [4, 8])
@pytest.mark.parametrize("desc", [False, True])
def test_code_families_are_what_they_say(bits, desc):
    K, N, gs = SMALL[bits]
    maxq = 2 ** bits - 1
    for fam in WEIGHT_CODE_FAMILIES:
        for sfam in ("u0.01", "zero_groups"):
            qw, qz, s, g_idx = weight_range_layer(sfam, fam, bits, K, N, gs, "fp16", desc_act=desc, seed=5)
            assert qw.shape == (K * bits // 32, N) and qw.dtype == np.int32 and qz.shape == (K // gs, N * bits // 32) and qz.dtype == np.int32
            assert g_idx.dtype == np.int32 and np.array_equal(np.sort(g_idx), np.arange(K) // gs) and (desc == (not np.array_equal(g_idx, np.arange(K) // gs)))
            q, z = O.unpack_rows(qw, bits).astype(np.int64), O.unpack_cols(qz, bits).astype(np.int64)
            zk = z[g_idx]
            if fam == "random":
                assert len(np.unique(q)) == maxq + 1 and len(np.unique(z)) > 0.8 * (maxq + 1)
            elif fam == "near_zero_point":
                assert np.abs(q - zk).max() == 1 and len(np.unique(z)) > 0.8 * (maxq + 1) and 0.5 < (q != zk).mean() < 0.75
            elif fam == "at_zero_point":
                assert np.array_equal(q, zk) if sfam == "u0.01" else (np.array_equal(q[s[g_idx] != 0], zk[s[g_idx] != 0]) and (q != zk)[s[g_idx] == 0].mean() > 0.8)
                assert not O.dequant_gptq(qw, qz, s, g_idx, bits, "fp16").any()                                   # every weight is +-0
            elif fam == "extremes":
                assert set(np.unique(q)) == {0, maxq} and set(np.unique(z)) == {0, maxq}
            else:
                assert (z == 1 << (bits - 1)).all() and len(np.unique(q)) == maxq + 1


@pytest.mark.parametrize("bits", [4, 8])
@pytest.mark.parametrize("sdt", ["fp16", "bf16"])
def test_oracle_dequant_equals_torch_cpu_bit_for_bit(sdt, bits):
    """Every scale family x code family: O.dequant_gptq against torch CPU scales[g] * (codes - zeros[g]) in the scale dtype, and the cast to
    each activation dtype against O.round_to -- as uint16 bit patterns (so -0.0 != +0.0)."""
    K, N, gs = SMALL[bits]
    for i, sfam in enumerate(_all_scale_families(sdt, bits)):
        for j, cfam in enumerate(WEIGHT_CODE_FAMILIES):
            desc = bool((i + j) & 1)
            qw, qz, s, g_idx = weight_range_layer(sfam, cfam, bits, K, N, gs, sdt, desc_act=desc, seed=11 + i)
            w = O.dequant_gptq(qw, qz, s, g_idx, bits, sdt)
            q = torch.from_numpy(O.unpack_rows(qw, bits).astype(np.int16))
            z = torch.from_numpy(O.unpack_cols(qz, bits).astype(np.int16))
            g = torch.from_numpy(g_idx.astype(np.int64))
            wt = f32_to_torch(s, sdt)[g] * (q - z[g])
            assert wt.dtype == TDT[sdt]
            assert np.array_equal(torch_to_bits(wt), _bits(w, sdt)), (sfam, cfam, sdt, bits)
            t2 = O.torch_cpu_dequant_gptq(torch.from_numpy(qw), torch.from_numpy(qz), f32_to_torch(s, sdt), torch.from_numpy(g_idx), bits)
            assert np.array_equal(torch_to_bits(t2), _bits(w, sdt)), (sfam, cfam, sdt, bits)
            for act in ("fp16", "bf16"):
                if act == "fp16" and sfam == "u2^60":
                    continue                                                 # (the reference's fp16 weights are inf there: out of scope)
                assert np.array_equal(torch_to_bits(wt.to(TDT[act])), _bits(O.round_to(w, act), act)), (sfam, cfam, sdt, act, bits)
                assert np.array_equal(torch_to_bits(bits_to_torch(_bits(w, sdt), sdt).to(TDT[act])), _bits(O.round_to(w, act), act))


def _gpu_cases():
    cases = []
    for act, sdt in WEIGHT_RANGE_DTYPES:
        for shape in WEIGHT_RANGE_DECODE_SHAPES:
            fams = weight_range_main_families(act, sdt) if shape == WEIGHT_RANGE_MAIN else weight_range_side_families(sdt)
            cases += [(shape, act, sdt, s, c) for s, c in fams]
        for shape in WEIGHT_RANGE_TILED:
            cases += [(shape, act, sdt, s, c) for s, c in weight_range_side_families(sdt)]
    return cases


def test_every_gpu_case_is_finite_and_no_row_is_left_out():
    worst_lo, worst_hi = np.inf, 0.0
    for shape, act, sdt, sfam, cfam in _gpu_cases():
        bits, K, N, gs, rows, (qw, qz, s, g_idx) = weight_range_layer_of(shape, sfam, cfam, sdt)
        w_rounded = O.round_to(O.dequant_gptq(qw, qz, s, g_idx, bits, sdt), act)
        assert np.isfinite(w_rounded).all(), (shape, act, sdt, sfam, cfam)
        w_exact = weight_exact_f64(qw, qz, s, g_idx, bits)
        x = weight_range_rows(act, w_exact, rows, seed=K // 128 + N // 16)
        assert np.array_equal(O.round_to(x, act), x) and np.isfinite(x).all()
        if act == "fp16":
            assert np.abs(x).max() < 65504.0
        y = O.matmul_round(x, w_rounded, None, act)                       # O.forward_gptq on the weights dequantised above
        assert np.isfinite(y).all(), (shape, act, sdt, sfam, cfam)
        top = np.abs(x.astype(np.float64) @ w_exact).max(axis=1)
        assert (top >= 2.0 ** -10).all() and (top <= 6.0e4).all(), (shape, act, sdt, sfam, cfam, top.min(), top.max())
        worst_lo, worst_hi = min(worst_lo, top.min()), max(worst_hi, top.max())
    print(f"largest |y_exact| per row over all cases: {worst_lo:.3e} .. {worst_hi:.3e}")


def test_at_zero_point_reference_output_is_exactly_the_bias():
    for act, sdt in WEIGHT_RANGE_DTYPES:
        for sfam in ("u0.01", "zero_groups", "signed"):
            bits, K, N, gs, rows, (qw, qz, s, g_idx) = weight_range_layer_of(WEIGHT_RANGE_MAIN, sfam, "at_zero_point", sdt)
            assert not weight_exact_f64(qw, qz, s, g_idx, bits).any()
            x = weight_range_rows(act, weight_exact_f64(qw, qz, s, g_idx, bits), 4)
            assert np.abs(x).max() > 1.0                                   # (a plain randn row: nothing to scale by)
            bias = O.round_to(np.random.RandomState(3).randn(N).astype(np.float32) * 0.1, act)
            assert np.array_equal(O.forward_gptq(x, qw, qz, s, g_idx, bits, bias, act, sdt), np.broadcast_to(bias, (4, N)))
            assert not O.forward_gptq(x, qw, qz, s, g_idx, bits, None, act, sdt).any()
