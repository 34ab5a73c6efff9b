"""Oracle of an FP8 (float8_e4m3fn, weight-only) sparse-MoE experts call (numpy + torch on the CPU; a helper, not a test; shared by
tests/test_moe_fp8_cpu.py and tests/test_gpu_moe_fp8.py), built on tests/fp8_oracle.py in the shape of tests/moe_oracle.py.  For a case it returns

  act_model  the kernels' stated stage-one contract restated: float64 dot products with exact code / scale_inv weights, then round(gate),
             round(up), round(silu(gate)), round(product) in the activation dtype, per slot s = t * top_k + j: [T * top_k, I]
  y64        float64 arithmetic from act_model with exact weights and the routing weights: [T, H]
  y_once     y64 rounded once to the activation dtype
  chain      the reference path from act_model on: fp8_oracle.chain (TorchFP8Linear's forward) for each expert's down, each output rounded, its
             product with the routing weight rounded, and index_add_ accumulation in the activation dtype in ascending expert id

Inputs: fp8_oracle.make_codes (uniform over the 254 finite bytes), make_scale_inv with its defaults (which keep the reference's fp16 cast of
scale_inv finite), moe_oracle.make_routing / make_x."""
import functools

import numpy as np

import fp8_oracle as F
import moe_oracle as MO

# (H, I, E, top_k): the smallest shapes at which the kernels can go wrong -- one chunk on the down side; odd chunk counts and an odd expert count;
# ten chunks on the gate|up side (more than eight waves: uneven shares, a ragged second round of loads); two waves per slot on the down side
SHAPES = {"256x128e8k2": (256, 128, 8, 2), "384x640e5k3": (384, 640, 5, 3), "1280x128e3k2": (1280, 128, 3, 2), "256x256e8k8": (256, 256, 8, 8)}
TOKENS = (1, 2, 5, 16)
# name -> ((gate / up method, block), (down method, block))
LAYOUTS = {"tensor": (("tensor", None), ("tensor", None)), "row": (("row", None), ("row", None)),
           "b128x128": (("block", (128, 128)), ("block", (128, 128))),
           # K blocks spanning two chunks over the ten chunks of H = 1280, and a different block height per projection
           "gu64x256_d32x128": (("block", (64, 256)), ("block", (32, 128)))}
WIDE_LAYOUT_SHAPE = "1280x128e3k2"
CASES = [(s, l) for s in sorted(SHAPES) for l in LAYOUTS if l != "gu64x256_d32x128" or s == WIDE_LAYOUT_SHAPE]
# Deep shapes: the smallest at which a wave runs SEVERAL chunks of its contiguous range (tests/moe_wave_model.py derives, from the kernels'
# constants, what each reaches) -- ranges longer than the look-ahead with a ragged last round, K blocks of 2 and 3 chunks that a wave boundary
# cuts, top_k 7 / 8 / 16.  Seeds of their own (_seed0), so the inputs of the cases above keep their bits.
DEEP_SHAPES = {"4224x128e3k2": (4224, 128, 3, 2), "128x4224e3k2": (128, 4224, 3, 2), "128x768e16k16": (128, 768, 16, 16),
               "256x768e8k8": (256, 768, 8, 8), "256x384e7k7": (256, 384, 7, 7)}
DEEP_LAYOUTS = {"gu64x384_d32x128": (("block", (64, 384)), ("block", (32, 128))), "gu128x128_d32x256": (("block", (128, 128)), ("block", (32, 256))),
                "gu128x128_d32x384": (("block", (128, 128)), ("block", (32, 384)))}
DEEP_CASES = [("4224x128e3k2", "row"), ("4224x128e3k2", "b128x128"), ("4224x128e3k2", "gu64x384_d32x128"),
              ("128x4224e3k2", "tensor"), ("128x4224e3k2", "b128x128"), ("128x4224e3k2", "gu128x128_d32x384"),
              ("128x768e16k16", "row"), ("128x768e16k16", "gu128x128_d32x256"), ("256x768e8k8", "tensor"), ("256x768e8k8", "gu128x128_d32x256"),
              ("256x384e7k7", "row"), ("256x384e7k7", "b128x128")]
DEEP_TOKENS = (1, 16)
assert not set(DEEP_SHAPES) & set(SHAPES) and not set(DEEP_LAYOUTS) & set(LAYOUTS)
_ALL_SHAPES = dict(SHAPES, **DEEP_SHAPES)
_ALL_LAYOUTS = dict(LAYOUTS, **DEEP_LAYOUTS)
_DEEP_SEED_BASE = 40                # first seed index of the deep shapes / layouts: past anything sorted(SHAPES) / sorted(LAYOUTS) can grow to
PROJ = ("gate", "up", "down")


def _shape_index(shape: str) -> int:
    return _DEEP_SEED_BASE + sorted(DEEP_SHAPES).index(shape) if shape in DEEP_SHAPES else sorted(SHAPES).index(shape)


def _layout_index(layout: str) -> int:
    return _DEEP_SEED_BASE + sorted(DEEP_LAYOUTS).index(layout) if layout in DEEP_LAYOUTS else sorted(LAYOUTS).index(layout)


def _seed0(shape: str, layout: str) -> int:
    return 7000 + 977 * _shape_index(shape) + 101 * _layout_index(layout)


def proj_dims(shape: str, name: str):
    """(N, K) of a projection's [N, K] weight."""
    H, I = _ALL_SHAPES[shape][:2]
    return (H, I) if name == "down" else (I, H)


def proj_layout(layout: str, name: str):
    return _ALL_LAYOUTS[layout][1 if name == "down" else 0]


def make_experts(shape: str, layout: str, lo: float = 200.0, hi: float = 6.0e4):
    """-> list of E dicts {gate, up, down}, each (codes uint8 [N, K], scale_inv float32 in the projection's layout)."""
    E = _ALL_SHAPES[shape][2]
    seed0 = _seed0(shape, layout) + (0 if hi <= 6.0e4 else 50000)
    out = []
    for e in range(E):
        d = {}
        for i, name in enumerate(PROJ):
            N, K = proj_dims(shape, name)
            method, block = proj_layout(layout, name)
            seed = seed0 + 6 * e + 2 * i
            codes, scale_inv = F.make_codes(seed, N, K), F.make_scale_inv(seed + 1, N, K, method, block, lo=lo, hi=hi)
            codes.setflags(write=False)
            scale_inv.setflags(write=False)
            d[name] = (codes, scale_inv)
        out.append(d)
    return out


@functools.lru_cache(maxsize=None)
def experts_of(shape: str, layout: str, hi: float = 6.0e4):
    return make_experts(shape, layout, hi=hi)


@functools.lru_cache(maxsize=None)
def weights64_of(shape: str, layout: str, hi: float = 6.0e4):
    """Exact weights code / scale_inv, float64 [N, K], per expert and projection."""
    out = []
    for ex in experts_of(shape, layout, hi):
        out.append({name: F.weights64(c, s, proj_layout(layout, name)[1]) for name, (c, s) in ex.items()})
    return out


def silu64(y):
    return y / (1.0 + np.exp(-y))


def act_model(w64, x, ids, act: str) -> np.ndarray:
    """Stage one as the kernels state it: [T * top_k, I] in the activation dtype (float64 holding representable values)."""
    T, k = ids.shape
    I = w64[0]["gate"].shape[0]
    out = np.zeros((T * k, I), np.float64)
    for t in range(T):
        for j in range(k):
            w = w64[int(ids[t, j])]
            g = F.round_to(np.asarray(x[t], np.float64) @ w["gate"].T, act)
            u = F.round_to(np.asarray(x[t], np.float64) @ w["up"].T, act)
            out[t * k + j] = F.round_to(F.round_to(silu64(g), act) * u, act)
    return out


def evaluate(experts, w64, layout: str, x, ids, rw, act: str, with_chain: bool = True):
    """experts / w64: experts_of(..) / weights64_of(..); x [T, H], ids [T, k], rw [T, k] float32 -> dict."""
    T, H = x.shape
    k = ids.shape[1]
    a = act_model(w64, x, ids, act)
    y64 = np.zeros((T, H), np.float64)
    for t in range(T):
        for j in range(k):
            y64[t] += float(rw[t, j]) * (a[t * k + j] @ w64[int(ids[t, j])]["down"].T)
    out = {"act_model": a, "y64": y64, "y_once": F.round_to(y64, act)}
    if with_chain:
        chain = np.zeros((T, H), np.float64)
        block = proj_layout(layout, "down")[1]
        for e in sorted(set(int(v) for v in ids.reshape(-1))):
            pos, tok = np.nonzero((ids == e).T)            # torch.where(expert_mask[e]) of a [top_k, T] mask: by slot, then by token
            codes, scale_inv = experts[e]["down"]
            d = F.chain(a[tok * k + pos], codes, scale_inv, None, act, block)      # each expert's down: the reference's forward, rounded
            for r, (p_, t) in enumerate(zip(pos, tok)):
                dr = F.round_to(d[r] * float(rw[t, p_]), act)
                chain[t] = F.round_to(chain[t] + dr, act)   # index_add_: rows of one token accumulate in order, each add rounded
        out["chain"] = chain
    return out


@functools.lru_cache(maxsize=None)
def case(shape: str, layout: str, T: int, act: str):
    """The inputs and oracle outputs of one GPU test case, computed once per process and left unchanged."""
    H, I, E, k = _ALL_SHAPES[shape]
    seed = 100 * _shape_index(shape) + T
    x = MO.make_x(8000 + seed, T, H, act).astype(np.float64)
    ids, rw = MO.make_routing(9000 + seed, T, E, k, act)
    out = evaluate(experts_of(shape, layout), weights64_of(shape, layout), layout, x, ids, rw, act)
    out.update(x=x, ids=ids, rw=rw)
    for v in out.values():
        v.setflags(write=False)
    return out


def bar(c) -> float:
    """The stage-two bar of tests/test_gpu_moe.py / tests/test_gpu_fp8.py."""
    return max(F.rel64(c["chain"], c["y64"]), F.rel64(c["y_once"], c["y64"])) + 1e-4


def model_down_f32(shape: str, layout: str, c, act: str, reverse: bool = True) -> np.ndarray:
    """act_model -> down as an implementation of the stage-two contract may compute it: the kernels' fp32 weights (code * fp32 reciprocal),
    fp32 accumulation chunk by chunk (in reversed chunk order), ONE fp32 weighted sum in slot order, ONE rounding."""
    H, I, E, k = _ALL_SHAPES[shape]
    block = proj_layout(layout, "down")[1]
    kw = [F.kernel_w(*ex["down"], block) for ex in experts_of(shape, layout)]
    ids, rw, a = c["ids"], c["rw"], c["act_model"].astype(np.float32)
    T = ids.shape[0]
    chunks = list(range(I // 128))
    y = np.zeros((T, H), np.float32)
    for t in range(T):
        for j in range(k):
            w = kw[int(ids[t, j])]
            d = np.zeros(H, np.float32)
            for ck in (reversed(chunks) if reverse else chunks):
                sl = slice(128 * ck, 128 * ck + 128)
                d = (d + (w[:, sl] @ a[t * k + j, sl]).astype(np.float32)).astype(np.float32)
            y[t] = (y[t] + np.float32(rw[t, j]) * d).astype(np.float32)
    return F.round_to(y, act)


def fused_rows(gate: np.ndarray, up: np.ndarray) -> np.ndarray:
    """The stacked gate|up row order restated: fused rows 16 t .. 16 t + 7 = gate rows 8 t .. 8 t + 7, 16 t + 8 .. 16 t + 15 = up rows 8 t .. 8 t + 7."""
    n = gate.shape[0]
    out = np.empty((2 * n,) + gate.shape[1:], gate.dtype)
    for t in range(n // 8):
        out[16 * t:16 * t + 8] = gate[8 * t:8 * t + 8]
        out[16 * t + 8:16 * t + 16] = up[8 * t:8 * t + 8]
    return out
