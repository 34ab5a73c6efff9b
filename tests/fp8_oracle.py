"""Oracle of the FP8 (float8_e4m3fn) weight-only linear (numpy + torch on the CPU; a helper, not a test; shared by tests/test_fp8_cpu.py and
tests/test_gpu_fp8.py).  W[n, k] = code[n, k] / scale_inv[...] with scale_inv fp32 in the tensor [] / row [N] / block [N / br, K / bc] layout.

  E4M3      the 256 decoded bytes (float64; 0x7f / 0xff are NaN)
  y64       float64 arithmetic: x . (code / scale_inv)^T + bias
  y_once    y64 rounded ONCE to the activation dtype -- the best any implementation can do
  chain     the reference's forward restated (TorchFP8Linear, fp8.py:384-387, 423-461): codes and scale_inv cast to the activation dtype, the
            quotient rounded to it, a dense matmul, the bias added in it
  kernel_w  the kernels' own weight arithmetic: float32(code) * (float32(1) / scale_inv), an fp32 product of the fp32 reciprocal
  rel64     max |a - y64| / max |y64|, as in tests/moe_oracle.py
Arrays in an activation dtype travel as float32 numpy arrays holding exactly representable values (`round_to`)."""
import functools

import numpy as np
import torch

TORCH_DT = {"fp16": torch.float16, "bf16": torch.bfloat16, "fp32": torch.float32}
FINITE_CODES = np.array([b for b in range(256) if (b & 0x7f) != 0x7f], dtype=np.uint8)   # 254 bytes: everything but the two NaNs


def _decode_table():
    t = np.zeros(256, np.float64)
    for b in range(256):
        e, m = (b >> 3) & 0xF, b & 7
        if e == 15 and m == 7:
            v = np.nan
        elif e == 0:
            v = (m / 8.0) * 2.0 ** -6
        else:
            v = (1.0 + m / 8.0) * 2.0 ** (e - 7)
        t[b] = -v if b & 0x80 else v
    return t


E4M3 = _decode_table()
E4M3.setflags(write=False)


def round_to(a, act: str) -> np.ndarray:
    """One rounding (nearest even) of a float64 / float32 array to the dtype; returned as float64 (exact)."""
    t = torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64)))
    return t.to(TORCH_DT[act]).to(torch.float64).numpy()


def expand_scale(scale_inv, N: int, K: int, block=None) -> np.ndarray:
    """scale_inv in any of the three layouts -> float32 [N, K]."""
    s = np.asarray(scale_inv, np.float32)
    if s.ndim == 0:
        return np.full((N, K), s, np.float32)
    if s.ndim == 1:
        assert s.shape == (N,)
        return np.repeat(s[:, None], K, axis=1)
    br, bc = block
    assert s.shape == (N // br, K // bc)
    return np.repeat(np.repeat(s, br, axis=0), bc, axis=1)


def weights64(codes, scale_inv, block=None) -> np.ndarray:
    """float64 [N, K]: code / scale_inv."""
    N, K = codes.shape
    return E4M3[codes] / expand_scale(scale_inv, N, K, block).astype(np.float64)


def y64(x, codes, scale_inv, bias=None, block=None) -> np.ndarray:
    y = np.asarray(x, np.float64) @ weights64(codes, scale_inv, block).T
    return y if bias is None else y + np.asarray(bias, np.float64)[None, :]


def y_once(x, codes, scale_inv, bias, act: str, block=None) -> np.ndarray:
    return round_to(y64(x, codes, scale_inv, bias, block), act)


def chain(x, codes, scale_inv, bias, act: str, block=None) -> np.ndarray:
    """The reference's forward: dequantise to the dtype (codes / scale_inv, both cast to it first), matmul, bias add -- torch CPU ops in the
    dtype itself, so every rounding step is the reference's."""
    dt = TORCH_DT[act]
    N, K = codes.shape
    w = torch.from_numpy(E4M3[codes]).to(dt)                                   # exact: 4 significant bits
    s = torch.from_numpy(expand_scale(scale_inv, N, K, block)).to(dt)          # scale_inv.to(target dtype): overflows fp16 above 65504
    wkn = (w / s).transpose(0, 1).contiguous()
    out = torch.matmul(torch.from_numpy(np.asarray(x, np.float64)).to(dt), wkn)
    if bias is not None:
        out = out + torch.from_numpy(np.asarray(bias, np.float64)).to(dt)
    return out.to(torch.float64).numpy()


def kernel_w(codes, scale_inv, block=None) -> np.ndarray:
    """float32 [N, K]: the kernels' weight values, float32(code) * (1 / scale_inv) with the reciprocal and the product rounded in fp32."""
    N, K = codes.shape
    r = np.float32(1.0) / expand_scale(scale_inv, N, K, block)
    return (E4M3[codes].astype(np.float32) * r).astype(np.float32)


def rel64(a, ref64) -> float:
    """max |a - y64| / max |y64| in float64."""
    return float(np.abs(np.asarray(a, np.float64) - ref64).max() / max(float(np.abs(ref64).max()), 1e-12))


def make_x(seed: int, M: int, K: int, act: str, amp: float = 0.5) -> np.ndarray:
    return round_to(np.random.RandomState(seed).randn(M, K) * amp, act)


def make_codes(seed: int, N: int, K: int) -> np.ndarray:
    """Random finite codes, uniform over the 254 finite bytes: every exponent, subnormals and both zeros occur."""
    return FINITE_CODES[np.random.RandomState(seed).randint(0, FINITE_CODES.size, size=(N, K))]


def make_scale_inv(seed: int, N: int, K: int, method: str, block=None, lo: float = 200.0, hi: float = 6.0e4) -> np.ndarray:
    """scale_inv log-uniform in [lo, hi] (not powers of two); hi <= 6e4 keeps the reference's fp16 cast of scale_inv finite."""
    shape = () if method == "tensor" else (N,) if method == "row" else (N // block[0], K // block[1])
    u = np.random.RandomState(seed).rand(*shape)
    return np.exp(np.log(lo) + u * (np.log(hi) - np.log(lo))).astype(np.float32)


METHOD_ID = {"tensor": 0, "row": 1, "block": 2}


@functools.lru_cache(maxsize=None)
def layer(K: int, N: int, method: str, block=None):
    """(codes uint8 [N, K], scale_inv) of one synthetic layer: a function of the shape and the scale layout alone."""
    seed = (K * 7 + N * 3 + 1000 * METHOD_ID[method] + (block[0] * 13 + block[1] if block else 0)) % (2 ** 31)
    codes, scale_inv = make_codes(seed, N, K), make_scale_inv(seed + 1, N, K, method, block)
    codes.setflags(write=False)
    scale_inv.setflags(write=False)
    return codes, scale_inv


@functools.lru_cache(maxsize=None)
def case(M: int, K: int, N: int, method: str, block, act: str, with_bias: bool):
    """Inputs and oracle outputs of one GPU test case, computed once per process and left unchanged."""
    codes, scale_inv = layer(K, N, method, block)
    x = make_x(M * 131 + K, M, K, act)
    bias = round_to(np.random.RandomState(N + 5).randn(N), act) if with_bias else None
    ref = y64(x, codes, scale_inv, bias, block)
    out = {"codes": codes, "scale_inv": scale_inv, "x": x, "y64": ref, "y_once": round_to(ref, act),
           "chain": chain(x, codes, scale_inv, bias, act, block)}
    if bias is not None:
        out["bias"] = bias
    for v in out.values():
        v.setflags(write=False)
    return out
