"""FP8 weight-only linear on the GPU: gptqhip_fp8_gemm (decode kernel up to 16 rows, general kernel above), gptqhip_fp8_dequant and HipFp8Linear
against the oracle of tests/fp8_oracle.py.

Bar.  The kernels apply 1 / scale_inv to the fp32 accumulator and round once, which is NOT the reference's chain, so they are held to float64
arithmetic, with the project's own bar from tests/test_gpu_moe.py:
    rel64(kernel, y64) <= max(rel64(chain, y64), rel64(y_once, y64)) + 1e-4
(no worse than the reference's chain or one output rounding, plus the fp32-partial-sum allowance).  scale_inv stays <= 6e4 in these cases: the
reference casts scale_inv to the activation dtype, a larger one overflows fp16 there and the chain returns zeros.  The dynamic-range cases
(scale_inv 2^-20 .. 2^40) are held to one rounding alone, element by element (their docstring says how)."""
import numpy as np
import pytest
import torch

import fp8_oracle as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
TDT = F.TORCH_DT
LAYOUTS = {"tensor": ("tensor", None), "row": ("row", None), "b128x128": ("block", (128, 128)), "b16x128": ("block", (16, 128)),
           "b48x256": ("block", (48, 256))}
_LAYERS = {}


def divides(K, N, layout):
    method, block = LAYOUTS[layout]
    return block is None or (N % block[0] == 0 and K % block[1] == 0)


def dev(a, act=None):
    t = torch.from_numpy(np.array(a))     # (the oracle's arrays are read-only)
    return t.to(device=DEV, dtype=TDT[act]) if act else t.to(DEV)


def host(t):
    return t.detach().to("cpu", torch.float64).numpy()


def mode_of(method):
    from gptqmodel_amd import ops
    return ops.FP8_SCALE_MODES[method]


def repacked(codes, scale_inv, method, block):
    from gptqmodel_amd import ops
    return ops.fp8_repack(dev(codes), dev(scale_inv), mode_of(method), block)


def device_layer(K, N, layout):
    """The oracle's layer of this shape in the kernel layout, relaid once per process."""
    key = (K, N, layout)
    if key not in _LAYERS:
        method, block = LAYOUTS[layout]
        codes, scale_inv = F.layer(K, N, method, block)
        _LAYERS[key] = repacked(codes, scale_inv, method, block)
    return _LAYERS[key]


def gemm(x, w_t, rs, bias, N, layout, cvt="default"):
    from gptqmodel_amd import ops
    method, block = LAYOUTS[layout]
    return ops.fp8_gemm(x, w_t, rs.reshape(-1), bias, N, mode_of(method), block, cvt=cvt)


def bar(c):
    return max(F.rel64(c["chain"], c["y64"]), F.rel64(c["y_once"], c["y64"])) + 1e-4


def check_cases(Ms, K, N, layout):
    method, block = LAYOUTS[layout]
    w_t, rs = device_layer(K, N, layout)
    bad = []
    for M in Ms:
        for act in ("fp16", "bf16"):
            for with_bias in (False, True):
                c = F.case(M, K, N, method, block, act, with_bias)
                y = gemm(dev(c["x"], act), w_t, rs, dev(c["bias"], act) if with_bias else None, N, layout)
                assert y.dtype == TDT[act] and tuple(y.shape) == (M, N)
                e, b = F.rel64(host(y), c["y64"]), bar(c)
                print(f"fp8 M={M} K={K} N={N} {layout} {act} bias={int(with_bias)}: rel64 {e:.3e} bar {b:.3e} "
                      f"(chain {F.rel64(c['chain'], c['y64']):.3e}, once {F.rel64(c['y_once'], c['y64']):.3e})")
                if not e <= b:
                    bad.append((M, act, with_bias, e, b))
    assert not bad, bad


# K: one chunk; two; nine (an uneven split over eight waves); 32 (four per wave).  N: one tile; three; seventeen.  N = 256 is there for the
# (128, 128) blocks of published checkpoints, which none of the other widths divides.
DECODE_SHAPES = [(K, N, l) for K in (128, 256, 1152, 4096) for N in (16, 48, 272, 256) for l in LAYOUTS
                 if divides(K, N, l) and (N != 256 or l == "b128x128")]


@pytest.mark.parametrize("K,N,layout", DECODE_SHAPES)
def test_decode_kernel_against_the_oracle(K, N, layout):
    check_cases((1, 2, 3, 16), K, N, layout)


GENERAL_SHAPES = [(K, N, l) for K, N in ((256, 48), (1152, 272), (256, 256)) for l in LAYOUTS
                  if divides(K, N, l) and (N != 256 or l == "b128x128")]


@pytest.mark.parametrize("K,N,layout", GENERAL_SHAPES)
def test_general_kernel_against_the_oracle(K, N, layout):
    check_cases((17, 33, 100, 257), K, N, layout)     # ragged row tiles; 272 columns = a ragged last wave (17 column tiles)


# ---- every code ---------------------------------------------------------------------------------------------------------------------------------
def every_code_layer(N, pow2, method, block):
    """K = 256; every weight row is a permutation of the 254 finite bytes plus two zeros: +-0, every subnormal and +-448 are in every row."""
    rng = np.random.RandomState(77 + N)
    row = np.concatenate([F.FINITE_CODES, np.array([0x00, 0x80], np.uint8)])
    codes = np.stack([rng.permutation(row) for _ in range(N)])
    shape = () if method == "tensor" else (N,) if method == "row" else (N // block[0], 256 // block[1])
    if pow2:
        scale_inv = (2.0 ** rng.randint(-3, 10, size=shape)).astype(np.float32)
    else:
        scale_inv = np.exp(rng.uniform(np.log(0.3), np.log(3.0e4), size=shape)).astype(np.float32)
    return codes, scale_inv


@pytest.mark.parametrize("method,block", [("row", None), ("tensor", None), ("block", (16, 128))])
@pytest.mark.parametrize("pow2", [True, False])
def test_every_code_through_both_kernels_and_the_dequant(method, block, pow2):
    """One-hot activation rows read single weights out: the output must be the weight itself, rounded once.  With power-of-two scales
    code / scale_inv is exact in every step, so the output must equal round(code / scale_inv) computed in float64; with arbitrary scales
    the kernels' documented arithmetic -- the fp32 product of the code and the fp32 reciprocal -- must come out, rounded once, bit for bit."""
    from gptqmodel_amd import ops
    N, K = 48, 256
    codes, scale_inv = every_code_layer(N, pow2, method, block)
    w_t, rs = repacked(codes, scale_inv, method, block)
    assert np.array_equal(host(rs).reshape(-1), (np.float32(1.0) / scale_inv.reshape(-1)).astype(np.float64))   # the IEEE fp32 reciprocal
    w_kernel = F.kernel_w(codes, scale_inv, block)                       # float32 [N, K]
    w_exact = F.weights64(codes, scale_inv, block)
    eye = np.eye(K)
    for act in ("fp16", "bf16"):
        want = F.round_to(w_kernel, act).T                                # [K, N]: row k of the output = weight column k
        if pow2:
            assert np.array_equal(want, F.round_to(w_exact, act).T)
        x = dev(eye, act)
        got_general = host(ops.fp8_gemm(x, w_t, rs.reshape(-1), None, N, mode_of(method), block))
        got_decode = np.concatenate([host(ops.fp8_gemm(x[r:r + 16].contiguous(), w_t, rs.reshape(-1), None, N, mode_of(method), block))
                                     for r in range(0, K, 16)])
        for name, got in (("general", got_general), ("decode", got_decode)):
            assert np.array_equal(got, want), (name, act, int((got != want).sum()))      # (a sum that starts at +0 has no -0 to keep)
    for act in ("fp16", "bf16", "fp32"):
        got = host(ops.fp8_dequant(w_t, rs.reshape(-1), K, N, mode_of(method), block, out_dtype=TDT[act]))
        want = F.round_to(w_kernel, act).T
        assert np.array_equal(got, want) and np.array_equal(np.signbit(got), np.signbit(want)), act
    if not pow2 or method != "row":
        return
    # the conversion routes of the decode kernel give the same bits
    x = dev(F.make_x(5, 16, K, "fp16"), "fp16")
    base = ops.fp8_gemm(x, w_t, rs.reshape(-1), None, N, mode_of(method), block)
    for cvt in ("packed", "f32", "bits"):
        assert torch.equal(ops.fp8_gemm(x, w_t, rs.reshape(-1), None, N, mode_of(method), block, cvt=cvt), base), cvt
    xb = x.to(torch.bfloat16)
    assert torch.equal(ops.fp8_gemm(xb, w_t, rs.reshape(-1), None, N, mode_of(method), block, cvt="f32"),
                       ops.fp8_gemm(xb, w_t, rs.reshape(-1), None, N, mode_of(method), block))


def test_dequant_rounds_the_fp32_product_where_it_is_an_fp16_tie():
    """scale_inv = 669.26: for some codes the fp32 product code * fp32(1 / scale_inv) lies exactly between two fp16 values and the exact
    product does not, so rounding the exact product -- what a multiply folded into the fp16 conversion does -- and rounding the fp32 product
    differ by one ulp.  The dequant's contract is the fp32 product, rounded once: its fp16 and bf16 outputs are its fp32 output rounded."""
    from gptqmodel_amd import ops
    N, K = 48, 256
    codes, _ = every_code_layer(N, False, "tensor", None)
    scale_inv = np.float32(669.26)
    r = np.float32(1.0) / scale_inv
    exact, prod = F.E4M3[F.FINITE_CODES] * np.float64(r), F.E4M3[F.FINITE_CODES].astype(np.float32) * r
    assert (exact.astype(np.float16) != prod.astype(np.float16)).any()          # the premise (numpy rounds a float64 to fp16 once)
    w_t, rs = repacked(codes, scale_inv, "tensor", None)
    w32 = ops.fp8_dequant(w_t, rs.reshape(-1), K, N, mode_of("tensor"), None, out_dtype=torch.float32)
    assert np.array_equal(host(w32), F.kernel_w(codes, scale_inv).T.astype(np.float64))
    for act in ("fp16", "bf16"):
        got = ops.fp8_dequant(w_t, rs.reshape(-1), K, N, mode_of("tensor"), None, out_dtype=TDT[act])
        assert torch.equal(got, w32.to(TDT[act])), (act, int((got != w32.to(TDT[act])).sum()))
        assert torch.equal(torch.signbit(got), torch.signbit(w32))


# ---- dynamic range --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [3, 19])
@pytest.mark.parametrize("act", ["fp16", "bf16"])
@pytest.mark.parametrize("method,block", [("row", None), ("block", (16, 128))])
def test_scale_ladder_and_activation_range(method, block, act, M):
    """scale_inv climbs from 2^-20 to 2^40 across the rows (row scales) or the blocks (block scales); activation rows at 1e-4, 1 and 1e+3.
    The outputs span sixty binades, so a bar normalised by the largest output would see the loud columns only.  Held to ONE rounding
    element by element instead:  |got - y64| <= |y_once - y64| + 1e-4 * S,  S[m, n] = sum_k |x[m, k] * W[n, k]| -- the 1e-4 allowance of the
    bar above, scaled by what a column's fp32 partial sums are made of (K * 2^-24 = 4e-5 for K = 640).  Where one rounding overflows the dtype
    (fp16 beyond 65504) the kernel must overflow the same way."""
    from gptqmodel_amd import ops
    N, K = 64, 640
    rng = np.random.RandomState(11)
    codes = F.make_codes(12, N, K)
    shape = (N,) if method == "row" else (N // block[0], K // block[1])
    n = int(np.prod(shape))
    scale_inv = (2.0 ** np.round(np.linspace(-20, 40, n))).astype(np.float32).reshape(shape)
    scale_inv *= (1.0 + rng.rand(*shape) * 0.5).astype(np.float32)            # not powers of two
    amps = np.array([1e-4, 1.0, 1e3] * 7)[:M]
    x = F.round_to(rng.randn(M, K) * amps[:, None], act)
    w_t, rs = repacked(codes, scale_inv, method, block)
    got = host(ops.fp8_gemm(dev(x, act), w_t, rs.reshape(-1), None, N, mode_of(method), block))
    w64 = F.weights64(codes, scale_inv, block)
    ref = x @ w64.T
    once = F.round_to(ref, act)
    S = np.abs(x) @ np.abs(w64).T
    big = float(torch.finfo(TDT[act]).max)
    edge = (np.abs(ref) > 0.999 * big) & (np.abs(ref) < 1.001 * big)              # at the overflow threshold either side may round either way
    over = np.isinf(once) & ~edge
    assert np.array_equal(got[over], once[over])
    ok = ~np.isinf(once) & ~edge
    assert np.isfinite(got[ok]).all()
    excess = np.abs(got[ok] - ref[ok]) - np.abs(once[ok] - ref[ok]) - 1e-4 * S[ok]
    print(f"fp8 ladder {method} {act} M={M}: {int(over.sum())} overflowing, worst excess {float(excess.max()):.3e}, "
          f"worst |got - y64| / S {float((np.abs(got[ok] - ref[ok]) / np.maximum(S[ok], 1e-300)).max()):.3e}")
    assert (excess <= 0).all()


@pytest.mark.parametrize("M", [16, 17])
def test_a_block_of_zero_codes_contributes_exactly_zero(M):
    """Block scales (16, 128), K = 256: the second K block of columns 16 .. 31 holds only +-0 codes under a huge reciprocal scale (scale_inv
    2^-20).  Those columns must come out bit-identical to the K = 128 layer made of the first block alone."""
    from gptqmodel_amd import ops
    N, K, block = 48, 256, (16, 128)
    codes = np.array(F.make_codes(21, N, K))
    scale_inv = np.array(F.make_scale_inv(22, N, K, "block", block))
    codes[16:32, 128:] = np.where(np.random.RandomState(23).rand(16, 128) < 0.5, 0x00, 0x80).astype(np.uint8)
    scale_inv[1, 1] = 2.0 ** -20
    x = F.make_x(24, M, K, "fp16")
    w_t, rs = repacked(codes, scale_inv, "block", block)
    full = ops.fp8_gemm(dev(x, "fp16"), w_t, rs.reshape(-1), None, N, mode_of("block"), block)
    w_h, rs_h = repacked(codes[:, :128].copy(), scale_inv[:, :1].copy(), "block", block)
    half = ops.fp8_gemm(dev(x[:, :128].copy(), "fp16"), w_h, rs_h.reshape(-1), None, N, mode_of("block"), block)
    assert torch.equal(full[:, 16:32], half[:, 16:32])
    assert not torch.equal(full[:, :16], half[:, :16])          # (the other columns do have a second block)


# ---- invariance -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["row", "b16x128"])
@pytest.mark.parametrize("act", ["fp16", "bf16"])
def test_bits_do_not_depend_on_the_run_the_batch_or_the_capture(layout, act):
    K, N = 1152, 272
    method, block = LAYOUTS[layout]
    w_t, rs = device_layer(K, N, layout)
    c = F.case(16, K, N, method, block, act, True)
    x, bias = dev(c["x"], act), dev(c["bias"], act)
    y = gemm(x, w_t, rs, bias, N, layout)
    assert torch.equal(gemm(x, w_t, rs, bias, N, layout), y)                       # run to run
    for t in range(16):                                                            # row t alone, and as the last row of a shorter batch
        assert torch.equal(gemm(x[t:t + 1], w_t, rs, bias, N, layout)[0], y[t]), t
        assert torch.equal(gemm(x[:t + 1], w_t, rs, bias, N, layout), y[:t + 1]), t
    big = dev(F.make_x(99, 40, K, act), act)                                        # the general kernel: run to run
    assert torch.equal(gemm(big, w_t, rs, bias, N, layout), gemm(big, w_t, rs, bias, N, layout))
    # a captured decode call replays to the eager bits
    from gptqmodel_amd import ops
    xs = x[:3].clone()
    out = torch.zeros((3, N), dtype=TDT[act], device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.fp8_gemm(xs, w_t, rs.reshape(-1), bias, N, mode_of(method), block, out=out)     # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.fp8_gemm(xs, w_t, rs.reshape(-1), bias, N, mode_of(method), block, out=out)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, y[:3])
    xs.copy_(x[5:8])
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, y[5:8])


# ---- module -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method,block", [("row", None), ("tensor", None), ("block", (32, 128))])
@pytest.mark.parametrize("act", ["fp16", "bf16"])
def test_module_pack_post_init_forward_dequantize(method, block, act):
    from gptqmodel_amd.nn_modules.qlinear.hip_fp8 import HipFp8Linear
    from gptqmodel_amd.utils.const import DEVICE, FORMAT, METHOD
    from gptqmodel_amd.utils.importer import select_quant_linear
    K, N = 384, 96
    g = torch.Generator().manual_seed(3)
    lin = torch.nn.Linear(K, N, bias=True)
    with torch.no_grad():
        lin.weight.copy_(torch.randn(N, K, generator=g) * 0.05)
        lin.bias.copy_(torch.randn(N, generator=g) * 0.3)
    cls = select_quant_linear(8, -1, False, True, device=DEVICE.ROCM, format=FORMAT.FP8, quant_method=METHOD.FP8, pack=True)
    assert cls is HipFp8Linear
    m = cls(bits=8, group_size=-1, sym=True, desc_act=False, in_features=K, out_features=N, bias=True, weight_scale_method=method,
            weight_block_size=block)
    m.pack(lin, None, None)                                    # the CPU packer fills the checkpoint buffers
    codes, scale_inv = m.weight.view(torch.uint8).numpy().copy(), m.weight_scale_inv.numpy().copy()
    bias = m.bias.double().numpy()
    m = m.to(DEV).eval()
    m.post_init()
    m.post_init()                                              # idempotent
    assert m.weight.dtype == torch.uint8 and m.weight.numel() == K * N and tuple(m.rscale.shape) == tuple(scale_inv.shape)
    x = F.make_x(8, 6, K, act).reshape(2, 3, K)
    y = m(dev(x, act))
    assert tuple(y.shape) == (2, 3, N) and y.dtype == TDT[act]
    bias_act = F.round_to(bias, act)                           # the module casts the fp16 bias to the activation dtype
    ref = F.y64(x.reshape(6, K), codes, scale_inv, bias_act, block)
    e = F.rel64(host(y).reshape(6, N), ref)
    b = max(F.rel64(F.chain(x.reshape(6, K), codes, scale_inv, bias_act, act, block), ref), F.rel64(F.round_to(ref, act), ref)) + 1e-4
    print(f"fp8 module {method} {act}: rel64 {e:.3e} bar {b:.3e}")
    assert e <= b
    big = m(dev(F.make_x(9, 40, K, act), act))                  # 40 rows: the general kernel through the module
    assert tuple(big.shape) == (40, N)
    empty = m(torch.empty((0, K), dtype=TDT[act], device=DEV))
    assert tuple(empty.shape) == (0, N) and empty.dtype == TDT[act]
    assert tuple(m(torch.empty((2, 0, K), dtype=TDT[act], device=DEV)).shape) == (2, 0, N)
    want32 = F.kernel_w(codes, scale_inv, block)
    for dt in ("fp32", "fp16", "bf16"):
        w = m.dequantize_weight(dtype=TDT[dt])
        assert tuple(w.shape) == (K, N) and w.dtype == TDT[dt] and w.is_cuda
        assert np.array_equal(host(w), F.round_to(want32, dt).T), dt
    assert m.dequantize_weight(device="cpu").dtype == torch.float32
    with pytest.raises(RuntimeError, match="state_dict"):
        m.state_dict()
