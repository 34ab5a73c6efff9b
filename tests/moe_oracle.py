"""Oracle of a quantised sparse-MoE experts call (numpy only; shared by tests/test_moe_oracle_cpu.py and tests/test_gpu_moe.py), built on
oracle.gptq_oracle and helpers.synth_gptq.  For given experts, x, ids and routing weights `evaluate` returns

  chain     the reference chain: the HF experts loop (Qwen3MoeExperts.forward / MixtralExperts.forward) over per-expert oracle forwards --
            every linear = dequantise, matmul, ONE rounding; act_fn(gate) * up rounded like HF; each expert's output rounded, its product with
            the routing weight rounded, and index_add_ accumulation in the activation dtype in ascending expert id
  act_ref   the stage-one output of that chain per slot s = t * top_k + j: [T * top_k, I]
  y64       float64 arithmetic on the reference's ROUNDED weights, from act_ref, with the routing weights: [T, H]
  y_once    y64 rounded once to the activation dtype

Routing weights are float32 values exactly representable in the activation dtype (HF hands the experts `router_top_value.to(dtype)`)."""
import functools

import numpy as np

from helpers import synth_gptq
from oracle import gptq_oracle as O

# (H, I, E, top_k, group_size; -1 = one group for the whole K of each projection): the smallest shapes at which the kernels can go wrong --
# one chunk on the down side; odd chunk counts and an odd expert count; whole-K groups
SHAPES = {"256x128e8k2": (256, 128, 8, 2, 128), "384x640e5k3": (384, 640, 5, 3, 128), "512x256e4k4gK": (512, 256, 4, 4, -1)}
TOKENS = (1, 2, 5, 16)
GS64_SHAPE = "256x128e4k2g64"      # group_size 64: outside the fused ops, served by the module's host-routed loop
_SEEDED_SHAPES = dict(SHAPES, **{GS64_SHAPE: (256, 128, 4, 2, 64)})      # (their sorted order fixes the seeds of every case above: add nothing here)
# Deep shapes: the smallest at which a wave of the MoE kernels runs SEVERAL 128-row chunks (tests/moe_wave_model.py derives, from the kernels'
# constants, what each reaches) -- more chunks than the look-ahead with a ragged last round, chunks of one wave in different groups
# (group_size 256), top_k 7 / 8 / 16, and H wide enough for several column blocks of the grouped path's combine.  Seeds of their own
# (_seed_index), so the inputs of the shapes above keep their bits.
DEEP_SHAPES = {"4224x128e3k2": (4224, 128, 3, 2, 128), "128x4224e3k2": (128, 4224, 3, 2, 128), "2304x1536e4k4g256": (2304, 1536, 4, 4, 256),
               "256x1408e8k8": (256, 1408, 8, 8, 128), "128x640e16k16": (128, 640, 16, 16, 128), "256x384e7k7": (256, 384, 7, 7, 128)}
DEEP_TOKENS = (1, 16)
assert not set(DEEP_SHAPES) & set(_SEEDED_SHAPES)
_ALL_SHAPES = dict(_SEEDED_SHAPES, **DEEP_SHAPES)
_DEEP_SEED_BASE = 40                # first seed index of the deep shapes: past anything sorted(_SEEDED_SHAPES) can grow to


def _seed_index(shape: str) -> int:
    if shape in DEEP_SHAPES:
        return _DEEP_SEED_BASE + sorted(DEEP_SHAPES).index(shape)
    return sorted(_SEEDED_SHAPES).index(shape)


def make_experts(shape: str, scale_dtype: str):
    """-> list of E dicts {gate, up, down}, each (qweight, qzeros, scales, g_idx) as synth_gptq makes them (scales in [0.005, 0.015])."""
    H, I, E, _, gs = _ALL_SHAPES[shape]
    seed0 = 3000 + 17 * _seed_index(shape)
    out = []
    for e in range(E):
        out.append({"gate": synth_gptq(seed0 + 3 * e, 4, H, I, H if gs < 0 else gs, scale_dtype=scale_dtype),
                    "up": synth_gptq(seed0 + 3 * e + 1, 4, H, I, H if gs < 0 else gs, scale_dtype=scale_dtype),
                    "down": synth_gptq(seed0 + 3 * e + 2, 4, I, H, I if gs < 0 else gs, scale_dtype=scale_dtype)})
    return out


@functools.lru_cache(maxsize=None)
def experts_of(shape: str, scale_dtype: str):
    return make_experts(shape, scale_dtype)


@functools.lru_cache(maxsize=None)
def rounded_weights(shape: str, act: str, scale_dtype: str):
    """The reference's weights as the matmul sees them: round_scaledtype(scale * (code - zero)), then cast to the activation dtype."""
    out = []
    for ex in experts_of(shape, scale_dtype):
        d = {}
        for name, (qw, qz, sc, gi) in ex.items():
            w = O.dequant_gptq(qw, qz, sc, gi, 4, scale_dtype)
            d[name] = O.round_to(w, act) if act != scale_dtype else w
        out.append(d)
    return out


def make_routing(seed: int, T: int, E: int, top_k: int, act: str):
    """ids int32 [T, top_k] (distinct experts per token while top_k <= E) and normalised routing weights, float32 exactly representable in act."""
    rng = np.random.RandomState(seed)
    ids = np.stack([rng.permutation(E)[:top_k] if top_k <= E else rng.randint(0, E, size=top_k) for _ in range(T)]).astype(np.int32)
    p = rng.rand(T, top_k).astype(np.float32) + 0.1
    return ids, O.round_to(p / p.sum(axis=1, keepdims=True), act)


def make_x(seed: int, T: int, H: int, act: str):
    return O.round_to(np.random.RandomState(seed).randn(T, H).astype(np.float32) * 0.5, act)


def expert_mlp(w, x, act):
    """One expert's MLP through the oracle's rounding steps: (stage-one output, output)."""
    h = O.silu_mul_ref(O.matmul_round(x, w["gate"], None, act), O.matmul_round(x, w["up"], None, act), act)
    return h, O.matmul_round(h, w["down"], None, act)


def evaluate(weights, x, ids, rw, act):
    """weights: rounded_weights(..) (list of {gate, up, down} float32 [K, N]); x [T, H], ids [T, k], rw [T, k] float32 -> dict."""
    T, H = x.shape
    k = ids.shape[1]
    I = weights[0]["gate"].shape[1]
    chain = np.zeros((T, H), np.float32)
    act_ref = np.zeros((T * k, I), np.float32)
    for e in sorted(set(int(v) for v in ids.reshape(-1))):
        pos, tok = np.nonzero((ids == e).T)            # torch.where(expert_mask[e]) of a [top_k, T] mask: by slot, then by token
        for p_, t in zip(pos, tok):                    # one row at a time: the same fp32 sums whatever else is routed to the expert
            h, d = expert_mlp(weights[e], x[t:t + 1], act)
            act_ref[t * k + p_] = h[0]
            d = O.round_to(d[0] * rw[t, p_], act)
            chain[t] = O.round_to(chain[t] + d, act)   # index_add_: rows of one token accumulate in order, each add rounded
    y64 = np.zeros((T, H), np.float64)
    for t in range(T):
        for j in range(k):
            y64[t] += float(rw[t, j]) * (act_ref[t * k + j].astype(np.float64) @ weights[int(ids[t, j])]["down"].astype(np.float64))
    return {"chain": chain, "act_ref": act_ref, "y64": y64, "y_once": O.round_to(y64.astype(np.float32), act)}


@functools.lru_cache(maxsize=None)
def case(shape: str, T: int, act: str, scale_dtype: str):
    """The inputs and oracle outputs of one GPU test case, computed once per process and left unchanged."""
    H, I, E, k, _ = _ALL_SHAPES[shape]
    seed = 100 * _seed_index(shape) + T
    x = make_x(5000 + seed, T, H, act)
    ids, rw = make_routing(6000 + seed, T, E, k, act)
    out = evaluate(rounded_weights(shape, act, scale_dtype), x, ids, rw, act)
    out.update(x=x, ids=ids, rw=rw)
    for v in out.values():
        v.setflags(write=False)
    return out


def rel64(a, y64) -> float:
    """max |a - y64| / max |y64| in float64."""
    return float(np.abs(np.asarray(a, np.float64) - y64).max() / max(float(np.abs(y64).max()), 1e-12))
