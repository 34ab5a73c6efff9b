"""NVFP4 weight-only linear on the GPU: gptqhip_fp4_gemm (decode kernel up to 16 rows, general kernel above), gptqhip_fp4_dequant,
gptqhip_fp4_repack and HipFp4Linear against the oracle of tests/fp4_oracle.py.

Bar.  The kernels put the exact block-scaled weights on the matrix pipe, apply the global scale and the bias to the fp32 accumulator and round
once, which is NOT the reference's chain, so they are held to float64 arithmetic with the project's own bar from tests/test_gpu_fp8.py:
    rel64(kernel, y64) <= max(rel64(chain, y64), rel64(y_once, y64)) + 1e-4
(no worse than the reference's chain or one output rounding, plus the fp32-partial-sum allowance).  Where single weights are read out through
one-hot activations the documented arithmetic must come out bit for bit (the sign of a zero is not part of the contract)."""
import numpy as np
import pytest
import torch

import fp4_oracle as F4
import linear_wave_model as LM

pytestmark = pytest.mark.gpu
DEV = "cuda"
TDT = F4.TORCH_DT
_LAYERS = {}


def dev(a, act=None):
    t = torch.from_numpy(np.array(a))     # (the oracle's arrays are read-only)
    return t.to(device=DEV, dtype=TDT[act]) if act else t.to(DEV)


def host(t):
    return t.detach().to("cpu", torch.float64).numpy()


def scalar(s2):
    return None if s2 is None else torch.tensor([s2], dtype=torch.float32, device=DEV)


def repacked(codes, scale):
    from gptqmodel_amd import ops
    return ops.fp4_repack(dev(F4.pack(codes)), dev(scale).view(torch.float8_e4m3fn))


def device_layer(K, N):
    """The oracle's layer of this shape in the kernel layout, relaid once per process."""
    if (K, N) not in _LAYERS:
        _LAYERS[(K, N)] = repacked(*F4.layer(K, N)) + (scalar(float(F4.S2)),)
    return _LAYERS[(K, N)]


def gemm(x, layer, bias, N, cvt="default", out=None):
    from gptqmodel_amd import ops
    w_t, s_t, s2 = layer
    return ops.fp4_gemm(x, w_t, s_t, s2, bias, N, out=out, cvt=cvt)


def bar(c):
    return max(F4.rel64(c["chain"], c["y64"]), F4.rel64(c["y_once"], c["y64"])) + 1e-4


def check_cases(Ms, K, N, biases=(False, True)):
    layer = device_layer(K, N)
    bad = []
    for M in Ms:
        for act in ("fp16", "bf16"):
            for with_bias in biases:
                c = F4.case(M, K, N, act, with_bias)
                y = gemm(dev(c["x"], act), layer, dev(c["bias"], act) if with_bias else None, N)
                assert y.dtype == TDT[act] and tuple(y.shape) == (M, N)
                e, b = F4.rel64(host(y), c["y64"]), bar(c)
                print(f"fp4 M={M} K={K} N={N} {act} bias={int(with_bias)}: rel64 {e:.3e} bar {b:.3e} "
                      f"(chain {F4.rel64(c['chain'], c['y64']):.3e}, once {F4.rel64(c['y_once'], c['y64']):.3e})")
                if not e <= b:
                    bad.append((M, act, with_bias, e, b))
    assert not bad, bad


# K: one chunk; two; nine (an uneven split over eight waves); 32 (four per wave, a full look-ahead round).  N: one tile; three; seventeen.
@pytest.mark.parametrize("K", [128, 256, 1152, 4096])
@pytest.mark.parametrize("N", [16, 48, 272])
def test_decode_kernel_against_the_oracle(K, N):
    check_cases((1, 2, 3, 16), K, N)


# The decode kernel's wide variant, picked by (K, N) alone: four column tiles per block from 1024 tiles, two chunks in flight.  16400 columns =
# 1025 tiles: the last block holds one tile of its four.  K = 384: wave ranges of one chunk (three waves); K = 2176: 17 chunks on eight waves,
# ranges of 2 and 3, a second trip that consumes one.  (With the bias only: the oracle's chain at this width is most of the test's time.)
@pytest.mark.parametrize("K,N", [(384, 16384), (2176, 16400)])
def test_wide_decode_variant_against_the_oracle(K, N):
    check_cases((1, 16), K, N, biases=(True,))


@pytest.mark.parametrize("K,N,n_sub", [(2176, 16400, 272), (384, 16384, 16)])
def test_bits_do_not_depend_on_the_decode_variant(K, N, n_sub):
    """A wide layer's first n_sub columns taken as a layer of their own run on the one-tile-per-block variant of the decode kernel.  Same chunks per
    wave, same order: same bits."""
    codes, scale = F4.layer(K, N)
    s2 = scalar(float(F4.S2))
    whole, part = repacked(codes, scale) + (s2,), repacked(codes[:n_sub].copy(), scale[:n_sub].copy()) + (s2,)
    for act in ("fp16", "bf16"):
        for M in (1, 16):
            x = dev(F4.make_x(7 + M, M, K, act), act)
            bias = dev(F4.round_to(np.random.RandomState(3).randn(N), act), act)
            y, y_sub = gemm(x, whole, bias, N), gemm(x, part, bias[:n_sub].contiguous(), n_sub)
            assert torch.equal(y[:, :n_sub], y_sub), (act, M)


@pytest.mark.parametrize("K,N", [(256, 48), (1152, 272)])
def test_general_kernel_against_the_oracle(K, N):
    check_cases((17, 33, 100, 257), K, N)     # ragged row tiles; 272 columns = a ragged last wave (17 column tiles)


# ---- every code x every scale -----------------------------------------------------------------------------------------------------------------
def every_code_layer():
    """K = 128, N = 256: column n carries scale byte FINITE[n] in all its blocks (the 254 finite bytes; the last two columns +0 and -0), every
    16-block holds a permutation of the 16 codes."""
    N, K = 256, 128
    rng = np.random.RandomState(41)
    codes = np.stack([np.concatenate([rng.permutation(16) for _ in range(K // 16)]) for _ in range(N)]).astype(np.uint8)
    col = np.concatenate([F4.FINITE_CODES, np.array([0x00, 0x80], np.uint8)])
    scale = np.repeat(col[:, None], K // 16, axis=1)
    return codes, scale


@pytest.mark.parametrize("s2", [1.0, float(np.float32(0.0123))])
def test_every_code_times_every_scale_through_both_kernels_and_the_dequant(s2):
    """One-hot activation rows read single weights out.  With s2 = 1 the result must equal code * scale exactly; with a global scale that is
    no power of two it must equal round(fp32(code * scale) * s2) bit for bit.  Every conversion route gives the bits of the default."""
    from gptqmodel_amd import ops
    N, K = 256, 128
    codes, scale = every_code_layer()
    w_t, s_t = repacked(codes, scale)
    gs = scalar(s2)
    w_kernel = F4.kernel_w(codes, scale, s2)                              # float32 [N, K]
    eye = np.eye(K)
    for act in ("fp16", "bf16"):
        want = F4.round_to(w_kernel, act).T                               # [K, N]: row k of the output = weight column k
        if s2 == 1.0:
            assert np.array_equal(want, F4.block_weights64(codes, scale).T)        # exact in the dtype: the premise of the kernels
        x = dev(eye, act)
        for cvt in ("default", "packed", "f32"):
            got_general = host(ops.fp4_gemm(x, w_t, s_t, gs, None, N, cvt=cvt))
            got_decode = np.concatenate([host(ops.fp4_gemm(x[r:r + 16].contiguous(), w_t, s_t, gs, None, N, cvt=cvt)) for r in range(0, K, 16)])
            for name, got in (("general", got_general), ("decode", got_decode)):
                assert np.array_equal(got, want), (name, act, cvt, int((got != want).sum()))
        if s2 == 1.0:                                                      # a null global scale is 1.0
            assert np.array_equal(host(ops.fp4_gemm(x[:16].contiguous(), w_t, s_t, None, None, N)), want[:16])
            assert np.array_equal(host(ops.fp4_gemm(x, w_t, s_t, None, None, N)), want)
    for act in ("fp16", "bf16", "fp32"):
        got = host(ops.fp4_dequant(w_t, s_t, gs, K, N, out_dtype=TDT[act]))
        assert np.array_equal(got, F4.round_to(w_kernel, act).T), act
        if s2 == 1.0:
            assert np.array_equal(host(ops.fp4_dequant(w_t, s_t, None, K, N, out_dtype=TDT[act])), got), act
    # dense activations: the routes agree bit for bit on sums too
    for act in ("fp16", "bf16"):
        for M in (16, 40):
            x = dev(F4.make_x(5, M, K, act), act)
            base = ops.fp4_gemm(x, w_t, s_t, gs, None, N)
            for cvt in ("packed", "f32"):
                assert torch.equal(ops.fp4_gemm(x, w_t, s_t, gs, None, N, cvt=cvt), base), (act, M, cvt)


def test_dequant_rounds_the_fp32_product_where_it_is_an_fp16_tie():
    """s2 = 0.014662: for some of the code x scale products the fp32 product with s2 lies exactly between two fp16 values and the exact product
    does not, so rounding the exact product -- what a multiply folded into the fp16 conversion does -- and rounding the fp32 product differ by
    one ulp.  The dequant's contract is round(fp32(code * s_blk) * s2): its fp16 and bf16 outputs are its fp32 output rounded."""
    from gptqmodel_amd import ops
    N, K = 256, 128
    codes, scale = every_code_layer()
    s2 = np.float32(0.014662)
    blk = F4.block_weights64(codes, scale)
    assert ((blk * np.float64(s2)).astype(np.float16) != (blk.astype(np.float32) * s2).astype(np.float16)).any()   # the premise (numpy rounds once)
    w_t, s_t = repacked(codes, scale)
    gs = scalar(float(s2))
    w32 = ops.fp4_dequant(w_t, s_t, gs, K, N, out_dtype=torch.float32)
    assert np.array_equal(host(w32), F4.kernel_w(codes, scale, s2).T.astype(np.float64))
    for act in ("fp16", "bf16"):
        got = ops.fp4_dequant(w_t, s_t, gs, K, N, out_dtype=TDT[act])
        assert torch.equal(got, w32.to(TDT[act])), (act, int((got != w32.to(TDT[act])).sum()))


# ---- placement ----------------------------------------------------------------------------------------------------------------------------------
def test_nibble_and_block_placement():
    """A weight that is zero but for one code at (n, k) must show that code at exactly [k, n] of the dequant, whatever nibble, dword, lane,
    chunk and tile it falls in; a scale that differs in one 16-block must move that block only."""
    from gptqmodel_amd import ops
    N, K = 48, 256
    one = 0x38                                                                # e4m3 1.0
    for n in (0, 1, 15, 16, 33, 47):
        for k in (0, 1, 15, 16, 127, 128, 255):
            codes = np.zeros((N, K), np.uint8)
            codes[n, k] = 0x0D                                                # -3
            w_t, s_t = repacked(codes, np.full((N, K // 16), one, np.uint8))
            got = host(ops.fp4_dequant(w_t, s_t, None, K, N))
            want = np.zeros((K, N))
            want[k, n] = -3.0
            assert np.array_equal(got, want), (n, k, np.argwhere(got != 0).tolist())
    codes = np.full((N, K), 0x02, np.uint8)                                   # 1.0 everywhere
    for n, blk in ((0, 0), (17, 1), (17, 7), (32, 8), (47, 15)):
        scale = np.full((N, K // 16), one, np.uint8)
        scale[n, blk] = 0x45                                                  # 3.25
        w_t, s_t = repacked(codes, scale)
        got = host(ops.fp4_dequant(w_t, s_t, None, K, N))
        want = np.ones((K, N))
        want[16 * blk:16 * blk + 16, n] = 3.25
        assert np.array_equal(got, want), (n, blk)
        y = host(ops.fp4_gemm(dev(np.ones((2, K)), "fp16"), w_t, s_t, None, None, N))
        assert np.array_equal(y, np.tile(want.sum(axis=0), (2, 1))), (n, blk)
    # beyond chunk 1: K = 4224, where wave 7 of the decode kernel runs 4 + 1 chunks.  One block in the chunk of its second trip (the one its
    # surplus loads repeat), one in a first-trip chunk at u = 3 of wave 7 and of wave 0, one mid-round (linear_wave_model.FP4_DEEP_PLACEMENT)
    K = 4224
    codes = np.full((N, K), 0x02, np.uint8)
    for n, blk in LM.FP4_DEEP_PLACEMENT:
        scale = np.full((N, K // 16), one, np.uint8)
        scale[n, blk] = 0x45
        w_t, s_t = repacked(codes, scale)
        got = host(ops.fp4_dequant(w_t, s_t, None, K, N))
        want = np.ones((K, N))
        want[16 * blk:16 * blk + 16, n] = 3.25
        assert np.array_equal(got, want), (n, blk)
        y = host(ops.fp4_gemm(dev(np.ones((2, K)), "fp16"), w_t, s_t, None, None, N))          # 4224 and 4260: exact in fp16
        assert np.array_equal(y, np.tile(want.sum(axis=0), (2, 1))), (n, blk)


# ---- dynamic range --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [3, 19])
@pytest.mark.parametrize("act", ["fp16", "bf16"])
def test_global_scale_ladder_and_activation_range(act, M):
    """s2 climbs 2^-20 .. 2^8 (times 1.3: no power of two); activation rows sit next to the smallest normal fp16, at 1, and as high as keeps the
    outputs finite.  The rows' outputs are binades apart, so the bar is taken ROW BY ROW (each row against its own largest |y64|): a bar
    normalised by the largest output of the batch would see the loud row only.  Scale bytes are positive, 2^-6 .. 1.875: the chain's cast of
    fp32(scale) * s2 to fp16 stays finite at s2 = 2^8."""
    from gptqmodel_amd import ops
    N, K = 48, 384
    rng = np.random.RandomState(11 + M)
    codes = F4.make_codes(12, N, K)
    scale = rng.randint(0x08, 0x40, size=(N, K // 16)).astype(np.uint8)
    w_t, s_t = repacked(codes, scale)
    bad = []
    for p in (-20, -14, -8, -3, 0, 8):
        s2 = float(np.float32(1.3 * 2.0 ** p))
        big = min(1.4e4, 200.0 / s2)                    # (|randn| stays below 4.6 here: 1.4e4 x 4.6 is the fp16 maximum)
        amps = np.array([6.2e-5, 1.0, big] * 7)[:M]
        x = F4.round_to(np.clip(rng.randn(M, K) * amps[:, None], -6.5e4, 6.5e4), act)
        got = host(ops.fp4_gemm(dev(x, act), w_t, s_t, scalar(s2), None, N))
        ref = F4.y64(x, codes, scale, s2)
        once, chain = F4.round_to(ref, act), F4.chain(x, codes, scale, s2, None, act)
        assert np.isfinite(once).all() and np.isfinite(got).all()
        for m in range(M):
            e = F4.rel64(got[m], ref[m])
            b = max(F4.rel64(chain[m], ref[m]), F4.rel64(once[m], ref[m])) + 1e-4
            print(f"fp4 ladder {act} M={M} s2=1.3*2^{p} row {m} (amp {amps[m]:.1e}): rel64 {e:.3e} bar {b:.3e}")
            if not e <= b:
                bad.append((p, m, e, b))
    assert not bad, bad


@pytest.mark.parametrize("M", [16, 17])
def test_zero_scales_and_zero_codes_contribute_exactly_zero(M):
    """K = 256: in columns 16 .. 31 the second chunk's blocks hold either random codes under a scale byte of +-0 or only +-0 codes under the
    largest scales.  Those columns must come out bit-identical to the K = 128 layer made of the first chunk alone."""
    N, K = 48, 256
    codes, scale = (np.array(a) for a in F4.layer(K, N))
    rng = np.random.RandomState(23)
    for blk in range(8, 16):
        if blk % 2:
            scale[16:32, blk] = np.where(rng.rand(16) < 0.5, 0x00, 0x80)
        else:
            codes[16:32, 16 * blk:16 * blk + 16] = np.where(rng.rand(16, 16) < 0.5, 0x0, 0x8)
            scale[16:32, blk] = np.where(rng.rand(16) < 0.5, 0x7E, 0xFE)      # +-448
    for act in ("fp16", "bf16"):
        x = F4.make_x(24, M, K, act)
        s2 = scalar(float(F4.S2))
        full = gemm(dev(x, act), repacked(codes, scale) + (s2,), None, N)
        half = gemm(dev(x[:, :128].copy(), act), repacked(codes[:, :128].copy(), scale[:, :8].copy()) + (s2,), None, N)
        assert torch.equal(full[:, 16:32], half[:, 16:32]), act
        assert not torch.equal(full[:, :16], half[:, :16])          # (the other columns do have a second chunk)


# ---- invariance -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", ["fp16", "bf16"])
def test_bits_do_not_depend_on_the_run_the_batch_or_the_capture(act):
    K, N = 1152, 272
    layer = device_layer(K, N)
    c = F4.case(16, K, N, act, True)
    x, bias = dev(c["x"], act), dev(c["bias"], act)
    y = gemm(x, layer, bias, N)
    assert torch.equal(gemm(x, layer, bias, N), y)                                 # run to run
    for t in range(16):                                                            # row t alone, and as the last row of a shorter batch
        assert torch.equal(gemm(x[t:t + 1], layer, bias, N)[0], y[t]), t
        assert torch.equal(gemm(x[:t + 1], layer, bias, N), y[:t + 1]), t
    big = dev(F4.make_x(99, 40, K, act), act)                                       # the general kernel: run to run
    assert torch.equal(gemm(big, layer, bias, N), gemm(big, layer, bias, N))
    # a captured decode call replays to the eager bits
    xs = x[:3].clone()
    out = torch.zeros((3, N), dtype=TDT[act], device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        gemm(xs, layer, bias, N, out=out)                                           # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gemm(xs, layer, bias, N, out=out)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, y[:3])
    xs.copy_(x[5:8])
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, y[5:8])


# ---- module -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", ["fp16", "bf16"])
def test_module_pack_post_init_forward_dequantize(act):
    from gptqmodel_amd.nn_modules.qlinear.hip_fp4 import HipFp4Linear
    from gptqmodel_amd.utils.adapter import Lora
    from gptqmodel_amd.utils.const import DEVICE, FORMAT, METHOD
    from gptqmodel_amd.utils.importer import select_quant_linear
    K, N = 256, 48
    g = torch.Generator().manual_seed(3)
    lin = torch.nn.Linear(K, N, bias=True)
    with torch.no_grad():
        lin.weight.copy_(torch.randn(N, K, generator=g) * 0.05)
        lin.bias.copy_(torch.randn(N, generator=g) * 0.3)
    cls = select_quant_linear(4, 16, False, True, device=DEVICE.ROCM, format=FORMAT.NVFP4, quant_method=METHOD.NVFP4, pack=True)
    assert cls is HipFp4Linear
    m = cls(bits=4, group_size=16, sym=True, desc_act=False, in_features=K, out_features=N, bias=True, weight_block_size=16)
    m.pack(lin, None, None)                                    # the CPU quantiser fills the checkpoint buffers
    codes, scale = F4.unpack(m.weight.numpy()), m.weight_scale.view(torch.uint8).numpy().copy()
    s2, bias = float(m.weight_scale_2), m.bias.double().numpy()
    m = m.to(DEV).eval()
    m.post_init()
    m.post_init()                                              # idempotent
    assert m.weight.dtype == torch.uint8 and m.weight.numel() == K * N // 2 and m.weight_scale.dtype == torch.uint8
    assert m.weight_scale.numel() == K * N // 16 and m.weight_scale_2.is_cuda and m.weight_scale_2.numel() == 1
    x = F4.make_x(8, 6, K, act).reshape(2, 3, K)
    y = m(dev(x, act))
    assert tuple(y.shape) == (2, 3, N) and y.dtype == TDT[act]
    bias_act = F4.round_to(bias, act)                          # the module casts the fp16 bias to the activation dtype
    ref = F4.y64(x.reshape(6, K), codes, scale, s2, bias_act)
    e = F4.rel64(host(y).reshape(6, N), ref)
    b = max(F4.rel64(F4.chain(x.reshape(6, K), codes, scale, s2, bias_act, act), ref), F4.rel64(F4.round_to(ref, act), ref)) + 1e-4
    print(f"fp4 module {act}: rel64 {e:.3e} bar {b:.3e}")
    assert e <= b
    xb = F4.make_x(9, 40, K, act)
    big = m(dev(xb, act))                                      # 40 rows: the general kernel through the module
    refb = F4.y64(xb, codes, scale, s2, bias_act)
    assert tuple(big.shape) == (40, N)
    assert F4.rel64(host(big), refb) <= max(F4.rel64(F4.chain(xb, codes, scale, s2, bias_act, act), refb),
                                            F4.rel64(F4.round_to(refb, act), refb)) + 1e-4
    empty = m(torch.empty((0, K), dtype=TDT[act], device=DEV))
    assert tuple(empty.shape) == (0, N) and empty.dtype == TDT[act]
    assert tuple(m(torch.empty((2, 0, K), dtype=TDT[act], device=DEV)).shape) == (2, 0, N)
    want32 = F4.kernel_w(codes, scale, s2)
    for dt in ("fp32", "fp16", "bf16"):
        w = m.dequantize_weight(dtype=TDT[dt])
        assert tuple(w.shape) == (K, N) and w.dtype == TDT[dt] and w.is_cuda
        assert np.array_equal(host(w), F4.round_to(want32, dt).T), dt
    assert m.dequantize_weight(device="cpu").dtype == torch.float32
    with pytest.raises(RuntimeError, match="state_dict"):
        m.state_dict()
    # a Lora adapter rides on the output: out + (x @ A) @ B
    r = 8
    A = (torch.randn(K, r, generator=g) * 0.05).to(TDT[act])
    B = (torch.randn(r, N, generator=g) * 0.05).to(TDT[act])
    base = m(dev(x.reshape(6, K), act))
    m.adapter = Lora(rank=r, lora_A=A.to(DEV), lora_B=B.to(DEV))
    with_lora = m(dev(x.reshape(6, K), act))
    m.adapter = None
    want = host(base) + (torch.from_numpy(x.reshape(6, K)) @ A.double() @ B.double()).numpy()
    assert not torch.equal(with_lora, base)
    assert F4.rel64(host(with_lora), want) <= (2.0 ** -7 if act == "bf16" else 2.0 ** -10) * 3      # three roundings of the dtype (x A, (x A) B, the sum)
