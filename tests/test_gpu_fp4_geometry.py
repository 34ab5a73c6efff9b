"""NVFP4 weight-only linear on the GPU at the depths where the decode kernel's look-ahead loop runs later trips (tests/linear_wave_model.py
says what each K reaches and tests/test_linear_wave_model_cpu.py asserts it): the one-tile variant at K = 4224 (wave 7: 4 + 1 chunks), 7040
(4 + 2, 4 + 3) and 8320 (4 + 4, 4 + 4 + 1); the four-tile variant at K = 4224 (wave 7: 2 + 2 + 1).  Oracle and bar of tests/test_gpu_fp4.py."""
import numpy as np
import pytest
import torch

import fp4_oracle as F4
import linear_wave_model as LM
from test_gpu_fp4 import TDT, check_cases, dev, device_layer, gemm, host, repacked, scalar

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("K", LM.FP4_DEEP_K)
def test_decode_kernel_deep_k_against_the_oracle(K):
    check_cases((1, 16), K, LM.N_NARROW, biases=(True,))


@pytest.mark.parametrize("K", LM.FP4_DEEP_K)
def test_one_hot_sweep_over_every_chunk_bit_for_bit(K):
    """One-hot activation rows, one in every chunk of K (linear_wave_model.one_hot_ks): row r of the output must be weight column k_r,
    round(fp32(code * s_blk) * s2) with a global scale that is no power of two, bit for bit at every chunk, trip and look-ahead slot, through
    the decode kernel (launches of 16 rows) and the general kernel; rows of zeros must come out as zeros.  The dequant of the same layer must
    give every weight."""
    from gptqmodel_amd import ops
    N = LM.N_NARROW
    codes, scale = F4.layer(K, N)
    layer = device_layer(K, N)
    w_kernel = F4.kernel_w(codes, scale, F4.S2)                                 # float32 [N, K]
    ks = LM.one_hot_ks(K // LM.CHUNK_K)
    rows = len(ks)
    padded = np.zeros((-(-rows // 16) * 16, K))
    padded[:rows] = LM.one_hot_x(K)
    for act in ("fp16", "bf16"):
        want = np.zeros((padded.shape[0], N))
        want[:rows] = F4.round_to(w_kernel[:, ks], act).T
        x = dev(padded, act)
        for cvt in ("default", "packed", "f32") if K == 4224 else ("default",):
            got_general = host(gemm(x, layer, None, N, cvt=cvt))
            got_decode = np.concatenate([host(gemm(x[r:r + 16].contiguous(), layer, None, N, cvt=cvt)) for r in range(0, padded.shape[0], 16)])
            for name, got in (("general", got_general), ("decode", got_decode)):
                wrong = sorted(set(np.argwhere(got != want)[:, 0].tolist()))
                assert not wrong, (name, act, cvt, "rows (= chunks, below %d)" % rows, wrong)
    for act in ("fp16", "bf16", "fp32"):
        got = host(ops.fp4_dequant(layer[0], layer[1], layer[2], K, N, out_dtype=TDT[act]))
        assert np.array_equal(got, F4.round_to(w_kernel, act).T), act


def test_wide_decode_variant_third_trip_gives_the_bits_of_the_narrow_one():
    """K = 4224, N = 16384: four tiles per block, two chunks per trip, wave 7 runs 2 + 2 + 1.  The layer is a random 32-column block repeated
    512 times (bias included), so EVERY 32-column group must equal that block run as a layer of its own on the one-tile variant (wave 7:
    4 + 1), which the first test of this file holds to the oracle at 48 columns.  Same chunks per wave, same order: same bits."""
    from gptqmodel_amd import ops
    K, N = LM.FP4_WIDE
    n_sub = 32
    codes, scale = F4.layer(K, n_sub)
    s2 = scalar(float(F4.S2))
    part = repacked(codes, scale) + (s2,)
    reps = N // n_sub
    whole = ops.fp4_repack(dev(F4.pack(codes)).repeat(reps, 1), dev(scale).repeat(reps, 1).view(torch.float8_e4m3fn)) + (s2,)
    for act in ("fp16", "bf16"):
        bias = dev(F4.round_to(np.random.RandomState(3).randn(n_sub), act), act)
        for M in (1, 16):
            x = dev(F4.make_x(7 + M, M, K, act), act)
            y, y_sub = gemm(x, whole, bias.repeat(reps), N), gemm(x, part, bias, n_sub)
            assert tuple(y.shape) == (M, N)
            assert torch.equal(y.view(M, reps, n_sub), y_sub[:, None, :].expand(M, reps, n_sub)), (act, M)
