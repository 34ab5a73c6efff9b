"""Oracle of the NVFP4 weight-only linear (numpy + torch on the CPU; a helper, not a test; shared by tests/test_fp4_cpu.py and
tests/test_gpu_fp4.py).  W[n, k] = code[n, k] * weight_scale[n, k / 16] * weight_scale_2: e2m1 codes two per byte (low nibble = even feature),
float8_e4m3fn block scales as bytes [N, K / 16], one fp32 global scale.  The reference cannot run its own FP4 forward without torchao
(gptqmodel/nn_modules/qlinear/fp4.py:45-55), so there are no reference-generated goldens: this restatement is the oracle.

  E2M1      the 16 decoded codes, +-{0, 0.5, 1, 1.5, 2, 3, 4, 6} (gptqmodel_ext/floatx_cpu.cpp:153-156)
  unpack    packed uint8 [N, K / 2] -> codes [N, K] (floatx_cpu.cpp:1998-2003);  pack is its inverse
  weights64 float64 [N, K]: code * block scale * global scale
  y64       float64 arithmetic: x . W^T + bias
  y_once    y64 rounded ONCE to the activation dtype -- the best any implementation can do
  chain     the reference's dequantise-then-matmul chain restated (quantization/dtype.py:303-340): the table value cast to the activation dtype,
            the effective scale fp32(weight_scale) * scale_2 cast to it, the product rounded to it, a dense matmul, the bias added in it
  kernel_w  the kernels' own weight arithmetic: fp32(code * s_blk) (exact) * s2, rounded to fp32
  rel64     max |a - y64| / max |y64|, as in tests/fp8_oracle.py
Arrays in an activation dtype travel as float64 numpy arrays holding exactly representable values (`round_to`)."""
import functools

import numpy as np
import torch

from fp8_oracle import E4M3, FINITE_CODES, TORCH_DT, make_x, rel64, round_to   # noqa: F401  (re-exported)

BLOCK = 16
E2M1 = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, -0.0, -0.5, -1.0, -1.5, -2.0, -3.0, -4.0, -6.0], np.float64)
E2M1.setflags(write=False)
S2 = np.float32(3.17e-4)    # a global scale of realistic size (amax / 2688 of a weight matrix with amax 0.85), not a power of two


def unpack(packed) -> np.ndarray:
    """uint8 [N, K / 2] -> codes uint8 [N, K]: feature 2 b is the low nibble of byte b, 2 b + 1 the high nibble."""
    p = np.asarray(packed, np.uint8)
    out = np.empty((p.shape[0], p.shape[1] * 2), np.uint8)
    out[:, 0::2] = p & 0xF
    out[:, 1::2] = p >> 4
    return out


def pack(codes) -> np.ndarray:
    c = np.asarray(codes, np.uint8)
    return (c[:, 0::2] | (c[:, 1::2] << 4)).astype(np.uint8)


def block_weights64(codes, scale) -> np.ndarray:
    """float64 [N, K]: code * block scale (exact)."""
    return E2M1[np.asarray(codes)] * np.repeat(E4M3[np.asarray(scale)], BLOCK, axis=1)


def weights64(codes, scale, s2=1.0) -> np.ndarray:
    return block_weights64(codes, scale) * np.float64(np.float32(s2))


def y64(x, codes, scale, s2=1.0, bias=None) -> np.ndarray:
    y = np.asarray(x, np.float64) @ weights64(codes, scale, s2).T
    return y if bias is None else y + np.asarray(bias, np.float64)[None, :]


def y_once(x, codes, scale, s2, bias, act: str) -> np.ndarray:
    return round_to(y64(x, codes, scale, s2, bias), act)


def chain(x, codes, scale, s2, bias, act: str) -> np.ndarray:
    """The reference's chain: dequantise to the dtype (table value and effective scale both cast to it first, the product rounded to it),
    matmul, bias add -- torch CPU ops in the dtype itself, so every rounding step is the reference's."""
    dt = TORCH_DT[act]
    w = torch.from_numpy(E2M1[np.asarray(codes)]).to(dt)                                              # exact
    eff = torch.from_numpy(E4M3[np.asarray(scale)].astype(np.float32) * np.float32(s2)).to(dt)         # fp32 product, then the cast
    wkn = (w * eff.repeat_interleave(BLOCK, dim=1)).transpose(0, 1).contiguous()
    out = torch.matmul(torch.from_numpy(np.asarray(x, np.float64)).to(dt), wkn)
    if bias is not None:
        out = out + torch.from_numpy(np.asarray(bias, np.float64)).to(dt)
    return out.to(torch.float64).numpy()


def kernel_w(codes, scale, s2=1.0) -> np.ndarray:
    """float32 [N, K]: the kernels' weight values, fp32(code * s_blk) * s2 with the second product rounded in fp32."""
    return (block_weights64(codes, scale).astype(np.float32) * np.float32(s2)).astype(np.float32)


def make_codes(seed: int, N: int, K: int) -> np.ndarray:
    return np.random.RandomState(seed).randint(0, 16, size=(N, K)).astype(np.uint8)


def make_scale(seed: int, N: int, K: int) -> np.ndarray:
    """Random finite scale bytes, uniform over the 254 finite e4m3 bytes: every exponent, subnormals, negative values and both zeros occur."""
    return FINITE_CODES[np.random.RandomState(seed).randint(0, FINITE_CODES.size, size=(N, K // BLOCK))]


@functools.lru_cache(maxsize=None)
def layer(K: int, N: int):
    """(codes uint8 [N, K], scale bytes uint8 [N, K / 16]) of one synthetic layer: a function of the shape alone."""
    seed = (K * 7 + N * 3 + 4000) % (2 ** 31)
    codes, scale = make_codes(seed, N, K), make_scale(seed + 1, N, K)
    codes.setflags(write=False)
    scale.setflags(write=False)
    return codes, scale


@functools.lru_cache(maxsize=None)
def case(M: int, K: int, N: int, act: str, with_bias: bool, s2: float = float(S2)):
    """Inputs and oracle outputs of one GPU test case, computed once per process and left unchanged."""
    codes, scale = layer(K, N)
    x = make_x(M * 131 + K, M, K, act)
    bias = round_to(np.random.RandomState(N + 5).randn(N), act) if with_bias else None
    ref = y64(x, codes, scale, s2, bias)
    out = {"codes": codes, "scale": scale, "x": x, "y64": ref, "y_once": round_to(ref, act), "chain": chain(x, codes, scale, s2, bias, act)}
    if bias is not None:
        out["bias"] = bias
    for v in out.values():
        v.setflags(write=False)
    return out
