"""CPU check of the bf16 -> fp16 conversion SCHEME of decode form 5 (helpers.np_bf16_wave_to_f16: the numpy statement of bf16_wave_scale /
bf16pair_to_f16pair in gptqmodel_amd/csrc/gptqhip_skinny.hip) on the input families of tests/test_gpu_decode_dynamic_range.py.
These assertions are about the chosen INPUTS, not about the kernel: converted as specified (a two-sided power of two per group, round toward
zero), every family stays two orders of magnitude under the 1e-4 bar the GPU tests hold the kernel to -- and the down-only shift the scheme
replaces (k >= 0) does not, from activations around 1e-6 downwards, which is why those GPU cases fail on a library built before the fix."""
import numpy as np
import pytest

from helpers import RANGE_FAMILIES, dynamic_range_rows, np_bf16_wave_to_f16, rel_err, synth_gptq
from oracle import gptq_oracle as O

K, N, GS = 4096, 128, 128


@pytest.fixture(scope="module")
def w_exact():
    qweight, qzeros, scales, g_idx = synth_gptq(811, 4, K, N, GS)
    g = O.normalize_g_idx(g_idx, scales.shape[0])
    return np.asarray(scales, np.float64)[g] * (O.unpack_rows(qweight, 4).astype(np.int64) - O.unpack_cols(qzeros, 4).astype(np.int64)[g])


def _products(x, w, **kw):
    f16, up = np_bf16_wave_to_f16(x, 128, **kw)
    x_rec = f16.astype(np.float64) * up
    return x_rec, (x_rec @ w)[None], (x.astype(np.float64) @ w)[None]


@pytest.mark.parametrize("family", RANGE_FAMILIES["bf16"])
def test_two_sided_scale_keeps_every_family_far_under_the_bar(w_exact, family):
    x = dynamic_range_rows("bf16", family, 1, K)[0]
    x_rec, y_rec, y = _products(x, w_exact)
    assert rel_err(y_rec, y) <= 1e-6, family
    assert np.array_equal(np.signbit(x_rec), np.signbit(x))
    for c in range(K // 128):                # bit-exact wherever the group's spread stays below 2^31 (8 bits fit above fp16's 2^-24)
        a = np.abs(x[128 * c:128 * (c + 1)].astype(np.float64))
        if a.max() > 0 and a.max() / a[a > 0].min() < 2.0 ** 31:
            assert np.array_equal(x_rec[128 * c:128 * (c + 1)], x[128 * c:128 * (c + 1)].astype(np.float64)), (family, c)


@pytest.mark.parametrize("family", ["u1e-12", "u1e-09", "u1e-06", "chunk_only"])
def test_down_only_shift_misses_the_bar_on_small_inputs(w_exact, family):
    x = dynamic_range_rows("bf16", family, 1, K)[0]
    _, y_rec, y = _products(x, w_exact, down_only=True)
    assert rel_err(y_rec, y) > 1e-4, family


@pytest.mark.parametrize("family", ["u0.5", "u3000", "u1e+06"])
def test_down_only_shift_and_two_sided_scale_agree_from_ordinary_magnitudes_up(w_exact, family):
    x = dynamic_range_rows("bf16", family, 1, K)[0]
    _, y_old, _ = _products(x, w_exact, down_only=True)
    _, y_new, y = _products(x, w_exact)
    assert rel_err(y_old, y) <= 1e-6 and rel_err(y_new, y) <= 1e-6


def test_edges_of_the_exponent_choice():
    """Zero and bf16-subnormal maxima take k = 0; the clamp keeps 2^k and 2^-k normal floats at both ends of bf16's range."""
    tiny_normal = np.float32(2.0 ** -126)
    for vals, k_want in (([0.0, -0.0], 0), ([2.0 ** -130, 0.0], 0), ([tiny_normal, 0.0], -126), ([2.0 ** -120, 0.0], -126),
                         ([2.0 ** -100, 0.0], -114), ([1.0, 0.5], -14), ([2.0 ** 14, 1.0], 0), ([3.0e38, 1.0], 113)):
        x = O.round_to(np.array(vals * 64, np.float32), "bf16")
        f16, up = np_bf16_wave_to_f16(x, 128)
        assert np.all(up == 2.0 ** k_want), (vals, np.log2(up[0]))
        assert np.isfinite(f16.astype(np.float64)).all() and np.abs(f16.astype(np.float64)).max() < 2.0 ** 15
        assert np.float32(up[0]) == up[0] and np.float32(1.0 / up[0]) == 1.0 / up[0] and np.float32(up[0]) >= tiny_normal <= np.float32(1.0 / up[0])
