"""FP8 weight-only linear on the GPU at the shapes where the loop structure matters (tests/linear_wave_model.py says what each reaches and
tests/test_linear_wave_model_cpu.py asserts it): decode waves that run a second and a third trip of the look-ahead loop, the last one ragged;
K-block scales longer than a round and out of step with it; blocks shared by waves; 16-column tiles that straddle scale rows; the general
kernel with several K blocks of three chunks.  Same oracle and the same bar as tests/test_gpu_fp8.py:
    rel64(kernel, y64) <= max(rel64(chain, y64), rel64(y_once, y64)) + 1e-4
and, where a wrong scale on a quiet column could hide under a bar normalised by the loudest output, the element-by-element form of its
scale-ladder test, or single weights read out bit for bit."""
import numpy as np
import pytest
import torch

import fp8_oracle as F
import linear_wave_model as LM
from test_gpu_fp8 import TDT, bar, dev, host, mode_of, repacked

pytestmark = pytest.mark.gpu
_LAYERS = {}


def device_layer(K, N, layout):
    """The oracle's layer of this shape in the kernel layout, relaid once per process."""
    key = (K, N, layout)
    if key not in _LAYERS:
        method, block = LM.LAYOUTS[layout]
        _LAYERS[key] = repacked(*F.layer(K, N, method, block), method, block)
    return _LAYERS[key]


def gemm(x, layer, bias, N, layout, cvt="default"):
    from gptqmodel_amd import ops
    method, block = LM.LAYOUTS[layout]
    return ops.fp8_gemm(x, layer[0], layer[1].reshape(-1), bias, N, mode_of(method), block, cvt=cvt)


def check_cases(Ms, K, N, layout):
    method, block = LM.LAYOUTS[layout]
    layer = device_layer(K, N, layout)
    bad, worst = [], 0.0
    for M in Ms:
        for act in ("fp16", "bf16"):
            for with_bias in (False, True):
                c = F.case(M, K, N, method, block, act, with_bias)
                y = gemm(dev(c["x"], act), layer, dev(c["bias"], act) if with_bias else None, N, layout)
                assert y.dtype == TDT[act] and tuple(y.shape) == (M, N)
                e, b = F.rel64(host(y), c["y64"]), bar(c)
                worst = max(worst, e / b)
                print(f"fp8 M={M} K={K} N={N} {layout} {act} bias={int(with_bias)}: rel64 {e:.3e} bar {b:.3e} "
                      f"(chain {F.rel64(c['chain'], c['y64']):.3e}, once {F.rel64(c['y_once'], c['y64']):.3e})")
                if not e <= b:
                    bad.append((M, act, with_bias, e, b))
    print(f"fp8 K={K} N={N} {layout} M={Ms}: worst rel64 / bar {worst:.3f}")
    assert not bad, bad


# ---- dense against the oracle ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,N,layout", LM.FP8_TABLE_CASES)
def test_decode_kernel_deep_k_against_the_oracle(K, N, layout):
    check_cases((1, 16), K, N, layout)


@pytest.mark.parametrize("K,N,layout", LM.FP8_TABLE_CASES + LM.FP8_GENERAL_EXTRA)
def test_general_kernel_deep_k_against_the_oracle(K, N, layout):
    check_cases((17, 100), K, N, layout)


# ---- scale rows, element by element ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,N,layout", LM.FP8_SCALE_ROW_CASES)
def test_tiles_that_straddle_scale_rows_element_by_element(K, N, layout):
    """Neighbouring scale rows a factor >= 8 apart (linear_wave_model.scale_row_ladder), so the columns' outputs are binades apart and a
    column that takes its neighbour's scale is off by its own size.  Held to ONE rounding element by element, as the scale-ladder test:
    |got - y64| <= |y_once - y64| + 1e-4 S,  S[m, n] = sum_k |x[m, k] W[n, k]|.  16 rows: the decode kernel; 17 and 100: the general kernel
    (100: a second row block)."""
    block = LM.block_of(layout)
    codes, scale_inv = F.layer(K, N, "block", block)[0], LM.scale_row_ladder(N, K, block)
    layer = repacked(codes, scale_inv, "block", block)
    w64 = F.weights64(codes, scale_inv, block)
    bad = []
    for act in ("fp16", "bf16"):
        for M in (16, 17, 100):
            x = F.make_x(31 if M == 16 else 31 + M, M, K, act)
            got = host(gemm(dev(x, act), layer, None, N, layout))
            assert np.isfinite(got).all()
            excess = LM.elementwise_excess(got, x, w64, act)
            S = np.abs(x) @ np.abs(w64).T
            print(f"fp8 scale rows K={K} N={N} {layout} {act} M={M}: {int((excess > 0).sum())} of {excess.size} outside, "
                  f"worst |got - y64| / S {float((np.abs(got - x @ w64.T) / S).max()):.3e}, worst excess / S {float((excess / S).max()):.3e}")
            if (excess > 0).any():
                bad.append((act, M, int((excess > 0).sum()), sorted(set(np.argwhere(excess > 0)[:, 1].tolist()))[:20]))
    assert not bad, bad


# ---- single weights, bit for bit --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,N,layout", LM.FP8_TABLE_CASES)
def test_one_hot_sweep_over_every_chunk_bit_for_bit(K, N, layout):
    """One-hot activation rows, one in every chunk of K (linear_wave_model.one_hot_ks: every K-step, every row quarter, the first and the last
    byte of a lane's eight): row r of the output must be weight column k_r in the kernels' documented arithmetic -- the fp32 product of the code
    and the fp32 reciprocal -- rounded once, bit for bit, at every chunk, trip and look-ahead slot; rows of zeros must come out as zeros.
    The dequant of the same layer must give every weight, signs of zero included."""
    from gptqmodel_amd import ops
    method, block = LM.LAYOUTS[layout]
    codes, scale_inv = F.layer(K, N, method, block)
    layer = device_layer(K, N, layout)
    w_kernel = F.kernel_w(codes, scale_inv, block)                               # float32 [N, K]
    ks = LM.one_hot_ks(K // LM.CHUNK_K)
    rows = len(ks)
    padded = np.zeros((-(-rows // 16) * 16, K))
    padded[:rows] = LM.one_hot_x(K)
    for act in ("fp16", "bf16"):
        want = np.zeros((padded.shape[0], N))
        want[:rows] = F.round_to(w_kernel[:, ks], act).T
        x = dev(padded, act)
        got_general = host(gemm(x, layer, None, N, layout))                      # one launch, >= 32 rows
        got_decode = np.concatenate([host(gemm(x[r:r + 16].contiguous(), layer, None, N, layout)) for r in range(0, padded.shape[0], 16)])
        for name, got in (("general", got_general), ("decode", got_decode)):
            wrong = sorted(set(np.argwhere(got != want)[:, 0].tolist()))
            assert not wrong, (name, act, "rows (= chunks, below %d)" % rows, wrong)
    for act in ("fp16", "bf16", "fp32"):
        got = host(ops.fp8_dequant(layer[0], layer[1].reshape(-1), K, N, mode_of(method), block, out_dtype=TDT[act]))
        want = F.round_to(w_kernel, act).T
        assert np.array_equal(got, want) and np.array_equal(np.signbit(got), np.signbit(want)), act


# ---- invariance -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["row", "b24x1408"])
@pytest.mark.parametrize("act", ["fp16", "bf16"])
def test_bits_of_a_deep_layer_do_not_depend_on_the_batch(layout, act):
    K, N = 4224, LM.N_NARROW
    method, block = LM.LAYOUTS[layout]
    layer = device_layer(K, N, layout)
    c = F.case(16, K, N, method, block, act, True)
    x, bias = dev(c["x"], act), dev(c["bias"], act)
    y = gemm(x, layer, bias, N, layout)
    for t in (0, 7, 15):
        assert torch.equal(gemm(x[t:t + 1], layer, bias, N, layout)[0], y[t]), t


@pytest.mark.parametrize("layout", ["row", "b24x1408"])
def test_conversion_routes_agree_bit_for_bit_on_a_deep_layer(layout):
    K, N = 4224, LM.N_NARROW
    method, block = LM.LAYOUTS[layout]
    layer = device_layer(K, N, layout)
    c = F.case(16, K, N, method, block, "fp16", True)
    x, bias = dev(c["x"], "fp16"), dev(c["bias"], "fp16")
    base = gemm(x, layer, bias, N, layout)
    for cvt in ("packed", "f32", "bits"):
        assert torch.equal(gemm(x, layer, bias, N, layout, cvt=cvt), base), cvt
    xb, bb = x.to(torch.bfloat16), bias.to(torch.bfloat16)
    base = gemm(xb, layer, bb, N, layout)
    for cvt in ("packed", "f32"):
        assert torch.equal(gemm(xb, layer, bb, N, layout, cvt=cvt), base), cvt
