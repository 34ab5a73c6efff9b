"""The small kernels around the prefill GEMM, restated in plain Python (a helper, not a test; used by tests/test_prefill_helper_model_cpu.py
and tests/test_gpu_prefill_helpers.py):

  * the launch geometry of launch_rmsnorm_gather / launch_gather_cols (gptqmodel_amd/csrc/gptqhip_aux.hip): which (R, IT) instantiation a
    (M, K) call runs, how many R-row passes and blocks it has, how many trips the grid-stride loop takes -- the constants are READ from the
    kernel source, so a changed threshold changes what this model says the test shapes reach;
  * a float32 model of rmsnorm_gather_kernel's statistics: the per-thread fma chain over its 16-byte pieces in order, the xor-shuffle tree
    over the 64 lanes of a wave, the four waves summed 0 + 1 + 2 + 3, `/ (float)K + eps`, the reciprocal square root; then the two
    documented roundings (the normalised value, its product with the weight);
  * the inputs of the GPU tests (shapes, seeds, row families), so that the CPU test vouches for exactly the cases the GPU test runs."""
import os
import re
from collections import namedtuple

import numpy as np

from conftest import ROOT
from oracle import gptq_oracle as O

f32, f64 = np.float32, np.float64
AUX = os.path.join(ROOT, "gptqmodel_amd", "csrc", "gptqhip_aux.hip")
THREADS = 256           # __launch_bounds__(256); `threadIdx.x + it * 256`
PIECE = 8               # 16-bit elements per 16-byte piece
WAVE = 64


# ---- constants of the two launchers, read from the source text --------------------------------------------------------------------------------
def _body(text: str, name: str) -> str:
    """The text of `int <name>(...) { ... }` (up to the first closing brace in column 0)."""
    start = text.index("int " + name + "(")
    return text[start:text.index("\n}\n", start)]


def _int(pattern: str, text: str, what: str) -> tuple:
    m = re.search(pattern, text)
    assert m, f"{what} not found in gptqhip_aux.hip"
    return tuple(int(g) for g in m.groups())


_TEXT = open(AUX).read()
_NORM, _GATHER = _body(_TEXT, "launch_rmsnorm_gather"), _body(_TEXT, "launch_gather_cols")
kGatherMaxK, = _int(r"constexpr\s+int\s+kGatherMaxK\s*=\s*(\d+)\s*;", _TEXT, "kGatherMaxK")
Launcher = namedtuple("Launcher", "rows_k r_short r_long grid_cap instantiations")


def _launcher(body: str, macro: str) -> Launcher:
    rows_k, r_short, r_long = _int(r"const int r = K <= (\d+) \? (\d+) : (\d+);", body, "rows per pass")
    cap, cap2 = _int(r"passes < (\d+) \? passes : (\d+)", body, "grid cap")
    assert cap == cap2
    inst = tuple((int(a), int(b)) for a, b in re.findall(macro + r"\((\d+), (\d+)\);", body))
    assert inst, macro
    return Launcher(rows_k, r_short, r_long, cap, inst)


NORM = _launcher(_NORM, "GPTQHIP_RMSG_A")
GATHER = _launcher(_GATHER, "GPTQHIP_GATHER")
GATHER_MIN_ROWS, = _int(r"K <= kGatherMaxK && M >= (\d+)", _GATHER, "the LDS gather's least row count")
SIMPLE_ROWS_CAP, _cap2 = _int(r"M < (\d+) \? M : (\d+)", _GATHER, "the simple gather's grid.y cap")
assert SIMPLE_ROWS_CAP == _cap2
NORM_MAX_K = kGatherMaxK     # gptqhip_rmsnorm_gather refuses K > 16384 (gptqhip_abi.hip), the LDS budget both kernels share

# kernel "lds": R rows per pass, IT pieces per thread (the instantiation), `pieces` of them needed; "simple": grid = (column blocks, rows)
Geometry = namedtuple("Geometry", "kernel R IT pieces passes grid trips")


def _ceil_div(a, b):
    return -(-a // b)


def _lds_geometry(L: Launcher, M: int, K: int) -> Geometry:
    pieces = _ceil_div(K // PIECE, THREADS)
    r = L.r_short if K <= L.rows_k else L.r_long
    mine = [it for rr, it in L.instantiations if rr == r]
    it = next((i for i in mine if pieces <= i), mine[-1])     # `if (it <= 1) .. else if (it <= 2) .. else ..`
    assert pieces <= it, (K, pieces, it)
    passes = _ceil_div(M, r)
    grid = min(passes, L.grid_cap)
    return Geometry("lds", r, it, pieces, passes, grid, _ceil_div(passes, grid))


def norm_geometry(M: int, K: int) -> Geometry:
    assert K % PIECE == 0 and 0 < K <= NORM_MAX_K and M > 0
    return _lds_geometry(NORM, M, K)


def gather_geometry(M: int, K: int) -> Geometry:
    if K % PIECE == 0 and K <= kGatherMaxK and M >= GATHER_MIN_ROWS:
        return _lds_geometry(GATHER, M, K)
    gy = min(M, SIMPLE_ROWS_CAP)
    return Geometry("simple", 1, 1, 1, M, (_ceil_div(K, THREADS), gy), _ceil_div(M, gy))


def simple_gather_reason(M: int, K: int):
    """Which condition sends a call to gather_cols_kernel: "long" (K beyond the staged row) or "few" (fewer rows than a pass is worth)."""
    if gather_geometry(M, K).kernel != "simple":
        return None
    return "long" if K > kGatherMaxK else ("few" if M < GATHER_MIN_ROWS else "ragged")


def live_threads(K: int, it: int) -> int:
    """Threads for which `threadIdx.x + it * 256 < k8` holds."""
    return min(max(K // PIECE - it * THREADS, 0), THREADS)


def has_partial_wave_piece(g: Geometry, K: int) -> bool:
    """Some piece is live in only part of a wave: the mask is false in the middle of the instantiation."""
    return any(live_threads(K, it) % WAVE for it in range(g.IT))


def has_dead_last_piece(g: Geometry, K: int) -> bool:
    return live_threads(K, g.IT - 1) == 0


def short_pass_in_later_trip(g: Geometry, M: int) -> bool:
    """A pass of a second or later trip with fewer than R live rows (the clamp `m0 + r < M ? .. : M - 1` in a later trip)."""
    for b in range(g.grid):
        for t in range(1, g.trips):
            m0 = (b + t * g.grid) * g.R
            if m0 < M < m0 + g.R:
                return True
    return False


def trip_of_row(g: Geometry, m: int) -> int:
    return (m // g.R) // g.grid


# ---- the float32 model of the statistics -------------------------------------------------------------------------------------------------------
def thread_sums(h: np.ndarray, pieces: int) -> np.ndarray:
    """[M, 256] fp32: every thread's `a = fmaf(x, x, a)` chain over its pieces in order, eight elements of a piece in address order.  A dead piece
    adds nothing (here: zeros, fmaf(0, 0, a) == a for a >= +0).  x * x is exact in float64 (x has at most 11 significant bits) and the float64
    sum with the fp32 accumulator rounds to fp32 like the fused operation does."""
    M, K = h.shape
    pad = np.zeros((M, pieces * THREADS * PIECE), f32)
    pad[:, :K] = h
    v = pad.reshape(M, pieces, THREADS, PIECE)
    a = np.zeros((M, THREADS), f32)
    for it in range(pieces):
        for e in range(PIECE):
            x = v[:, it, :, e].astype(f64)
            a = (x * x + a.astype(f64)).astype(f32)
    return a


def block_sum(a: np.ndarray) -> np.ndarray:
    """[M] fp32: `a += __shfl_xor(a, mk, 64)` for mk = 32 .. 1 inside each wave, then red[0] + red[1] + red[2] + red[3]."""
    w = a.reshape(a.shape[0], THREADS // WAVE, WAVE).astype(f32)
    lane = np.arange(WAVE)
    mk = WAVE // 2
    while mk >= 1:
        w = w + w[:, :, lane ^ mk]
        mk >>= 1
    red = w[:, :, 0]
    return ((red[:, 0] + red[:, 1]) + red[:, 2]) + red[:, 3]


def sum_of_squares(h: np.ndarray, chunk: int = 512) -> np.ndarray:
    """[M] fp32, the kernel's order of summation."""
    pieces = _ceil_div(h.shape[1] // PIECE, THREADS)
    return np.concatenate([block_sum(thread_sums(h[i:i + chunk], pieces)) for i in range(0, h.shape[0], chunk)])


def rsqrt32(v: np.ndarray, ulps: int = 0) -> np.ndarray:
    """The correctly rounded fp32 reciprocal square root, moved `ulps` fp32 steps (the device's rsqrtf is within one)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = (1.0 / np.sqrt(v.astype(f64))).astype(f32)
    for _ in range(abs(ulps)):
        inv = np.nextafter(inv, f32(np.inf if ulps > 0 else 0.0))
    return inv


def model_inv(h: np.ndarray, eps: float, ulps: int = 0, wrong: str = None, s: np.ndarray = None) -> np.ndarray:
    """[M] fp32: 1 / rms as the kernel computes it.  wrong = "eps_inside": rsqrt((sum + eps) / K); "no_eps": rsqrt(sum / K) -- two slips the
    eps cases must be able to tell from the kernel."""
    s, k, e = sum_of_squares(h) if s is None else s, f32(h.shape[1]), f32(eps)
    with np.errstate(divide="ignore", invalid="ignore"):
        stat = {None: lambda: s / k + e, "eps_inside": lambda: (s + e) / k, "no_eps": lambda: s / k}[wrong]()
    return rsqrt32(stat.astype(f32), ulps)


def oracle_inv(h: np.ndarray, eps: float) -> np.ndarray:
    """[M] fp32: 1 / rms as O.rmsnorm_ref computes it (float64 mean rounded to fp32; eps added and the root taken in float64)."""
    var = np.mean(h.astype(f64) ** 2, axis=-1).astype(f32)
    return (1.0 / np.sqrt(var.astype(f64) + eps)).astype(f32)


def normalise(h: np.ndarray, w: np.ndarray, inv: np.ndarray, act: str) -> np.ndarray:
    """The two roundings both sides share: act(h32 * inv) in fp32, its fp32 product with the weight rounded once."""
    with np.errstate(invalid="ignore", over="ignore"):
        return O.round_to(np.asarray(w, f32) * O.round_to(np.asarray(h, f32) * inv.astype(f32)[:, None], act), act)


def bits16(x: np.ndarray, act: str) -> np.ndarray:
    return np.asarray(x, f32).astype(np.float16).view(np.uint16) if act == "fp16" else O.bf16_bits(x)


def ulps16(got_bits: np.ndarray, ref_bits: np.ndarray) -> np.ndarray:
    """Distance in representable 16-bit floats (sign-magnitude -> ordered integers)."""
    def order(b):
        b = b.astype(np.int32)
        return np.where(b & 0x8000, -(b & 0x7FFF), b & 0x7FFF)
    return np.abs(order(got_bits) - order(ref_bits))


# the project's bar for this kernel (tests/test_gpu_round3.py::test_rmsnorm_gather_vs_hf_formula)
BAR_ULPS, BAR_FRACTION = 2, 1e-3


def distance(got_bits: np.ndarray, ref_bits: np.ndarray):
    """(largest distance in 16-bit ulps, fraction of the elements that differ)."""
    d = ulps16(got_bits, ref_bits)
    return int(d.max()), float((d > 0).mean())


def meets_bar(worst: int, fraction: float) -> bool:
    return worst <= BAR_ULPS and fraction <= BAR_FRACTION


def model_vs_oracle(h: np.ndarray, w: np.ndarray, eps: float, act: str, ulps: int = 0, wrong: str = None, s: np.ndarray = None):
    """distance() of the model's output from O.rmsnorm_ref's, per row: (worst [M], differing elements [M]).  Both sides apply normalise() to
    their own 1 / rms, so a row whose two values are the same fp32 number is bit-equal without being evaluated (pinned by
    test_prefill_helper_model_cpu.py::test_normalise_with_the_oracles_statistics_is_the_oracle)."""
    mi, oi = model_inv(h, eps, ulps, wrong, s), oracle_inv(h, eps)
    worst, differing = np.zeros(h.shape[0], np.int64), np.zeros(h.shape[0], np.int64)
    rows = np.flatnonzero(mi.view(np.uint32) != oi.view(np.uint32))
    for i in range(0, rows.size, 256):
        r = rows[i:i + 256]
        d = ulps16(bits16(normalise(h[r], w, mi[r], act), act), bits16(normalise(h[r], w, oi[r], act), act))
        worst[r], differing[r] = d.max(axis=1), (d > 0).sum(axis=1)
    return worst, differing


# ---- the cases of tests/test_gpu_prefill_helpers.py ---------------------------------------------------------------------------------------------
ACTS = ("fp16", "bf16")
# the smallest K that reaches each case -- (R, IT): K
K_CASES = {
    (4, 1): (8, 264, 2048),         # one live thread; 33 pieces: part of wave 0; every thread
    (4, 2): (2056, 3584),           # the second piece live in one thread; Qwen2.5-7B's hidden size
    (4, 4): (4104, 5120),           # three pieces, the fourth dead; Llama-2-13B / Qwen2.5-14B
    (2, 6): (8200, 11008, 12288),   # five pieces, the sixth dead; Llama-2-7B's intermediate size; six full pieces
    (2, 8): (12296, 16384),         # seven pieces, the eighth dead; the largest K, byte offsets up to 32766
}
K_LIST = tuple(k for ks in K_CASES.values() for k in ks)
VARIANT_ROWS = 9


def variant_rows_of(K: int):
    """M of the variants test: one row, three, one more than a pass holds, nine."""
    return tuple(sorted({1, 3, norm_geometry(1, K).R + 1, VARIANT_ROWS}))


TRIP_SHAPES = ((8197, 264), (16389, 8), (4099, 8200))      # second / third trips of the grid-stride loop, a short last pass in them
GATHER_LDS_ROWS = (8, 9, 13)
GATHER_SIMPLE_SHAPES = ((1, 264), (7, 264), (9, 16392), (9, 28672), (1030, 16392))
EPS_K = (264, 5120, 12288)
EPS_LIST = (1e-6, 1e-5, 1e-3)
EPS_RATIOS = (1e-2, 1e-1, 1.0, 10.0, 100.0)
FAMILIES = tuple(f"eps/ms={r:g}" for r in EPS_RATIOS) + ("massive", "+0", "-0", "one-hot", "span", "top", "tiny", "randn")
FAMILY_ROWS = len(FAMILIES)      # 13: the families fall at different positions of the 4- and 2-row passes


def plain_case(M: int, K: int, act: str):
    """(h [M, K], w [K]) float32 holding values of `act`: rows of different scale, weights around 1 (the inputs of the geometry tests)."""
    rng = np.random.RandomState(100003 * (ACTS.index(act) + 1) + 7 * K + M)
    h = O.round_to(rng.randn(M, K).astype(f32) * (0.5 + np.arange(M)[:, None] % 7), act)
    return h, range_weights(rng, K, act)


def range_weights(rng, K: int, act: str) -> np.ndarray:
    """randn with a tenth of the weights scaled by 8: negative, large and near-zero weights."""
    w = rng.randn(K).astype(f32)
    w[rng.rand(K) < 0.1] *= f32(8.0)
    return O.round_to(w, act)


def _family_row(name: str, rng, K: int, act: str, eps: float) -> np.ndarray:
    if name.startswith("eps/ms="):
        return rng.randn(K) * np.sqrt(eps / float(name[7:]))
    if name == "massive":
        row = rng.randn(K) * 0.05
        row[rng.choice(K, 3, replace=False)] = np.array([2000.0, -1900.0, 2100.0])
        return row
    if name in ("+0", "-0"):
        return np.zeros(K) if name == "+0" else -np.zeros(K)
    if name == "one-hot":
        row = np.zeros(K)
        row[rng.randint(K)] = -1.0 - rng.randint(1, 64) / 64.0
        return row
    if name == "span":
        return rng.choice([-1.0, 1.0], K) * 2.0 ** rng.uniform(-14.0, 10.0, K)
    if name == "top":
        return rng.uniform(-1.0, 1.0, K) * (6.0e4 if act == "fp16" else 1.0e15)
    if name == "tiny":
        if act == "fp16":
            return rng.randint(-8, 9, K) * 2.0 ** -24
        row = O.round_to((rng.choice([-1.0, 1.0], K) * rng.uniform(0.5, 1.5, K) * 1e-30).astype(f32), act)
        # The squares vanish, so 1 / rms is rsqrt(eps) whatever the row holds: exactly 1000 = 125 * 2^3 for eps = 1e-6, and the product of 125 with an
        # 8-bit significand is an exact rounding tie for one significand in 128.  A tie goes with the last bit of the device's rsqrtf, which nothing
        # specifies: elements whose product lies within an fp32 step of a bf16 rounding boundary move on to the next bf16 value.
        inv = rsqrt32(np.array([eps], f32))[0]
        for _ in range(4):
            p = row * inv
            near = O.round_bf16(np.nextafter(p, f32(0.0))) != O.round_bf16(np.nextafter(p, np.copysign(f32(np.inf), p)))
            if not near.any():
                break
            row = np.where(near, O.round_bf16(row * f32(1.0 + 2.0 ** -7)), row)
        assert not near.any()
        return row
    assert name == "randn"
    return rng.randn(K)


FAMILY_MAX_DRAWS = 12
_family_cache = {}


def family_case(K: int, act: str, eps: float):
    """(h [13, K], w [K]): one row per family of FAMILIES.
      eps/ms=<r>  randn scaled so that eps / mean(h^2) is about r: from eps as a rounding detail to eps deciding the result
      massive     randn * 0.05 with three entries near +-2000 (a massive-activation row)
      +0, -0      padding rows;  one-hot: a single non-zero entry
      span        entries of magnitude 2^-14 .. 2^10
      top         the top of the range: fp16 |h| up to 6e4, bf16 up to 1e15 (the fp32 SUM of squares stays finite)
      tiny        fp16: n * 2^-24 with |n| <= 8, around the smallest subnormal; bf16: (0.5 .. 1.5) * 1e-30, whose squares are zero in fp32 for the
                  kernel and for the oracle alike
      randn       a plain row
    Left out on purpose: bf16 subnormal inputs and rows whose squares or partial sums are fp32 denormals (the device's denormal mode would decide
    the result), and bf16 rows whose sum of squares exceeds FLT_MAX while the mean does not (the kernel, like HF's fp32 mean, gives inf -> 0; the
    oracle's float64 mean does not).

    The bar is applied to each row on its own, and one row cannot average: all elements of a row share one 1 / rms, so all elements with the same
    significand (128 classes in bf16, 1024 in fp16) sit at the same distance from a rounding boundary and flip TOGETHER when 1 / rms moves by an
    fp32 ulp -- a class is about 1e-2 (bf16) / 1e-3 (fp16) of a row, and for roughly one row in ten some class lies that close.  Whether the model
    (this file) meets the bar with rsqrt exact and one ulp off either way is therefore decided per row, and a row that does not is drawn again
    (seeded by its draw number; family_draws() tells how often): the case changes, the bar does not, and nothing here looks at the kernel."""
    key = (K, act, float(eps))
    if key not in _family_cache:
        base = [7919, ACTS.index(act), K, int(round(-np.log10(eps)))]
        w = range_weights(np.random.RandomState(base), K, act)
        rows, draws = [], []
        for f, name in enumerate(FAMILIES):
            for draw in range(FAMILY_MAX_DRAWS):
                row = O.round_to(np.asarray(_family_row(name, np.random.RandomState(base + [f + 1, draw]), K, act, eps), f64).astype(f32)[None], act)
                if row_meets_bar_whatever_rsqrt_rounds_to(row, w, eps, act):
                    break
            else:
                raise AssertionError(("no draw of this family meets the bar in the model", K, act, eps, name))
            rows.append(row[0])
            draws.append(draw)
        _family_cache[key] = (np.stack(rows), w, tuple(draws))
    h, w, _ = _family_cache[key]
    return h.copy(), w.copy()


def family_draws(K: int, act: str, eps: float):
    family_case(K, act, eps)
    return _family_cache[(K, act, float(eps))][2]


def row_meets_bar_whatever_rsqrt_rounds_to(row: np.ndarray, w: np.ndarray, eps: float, act: str) -> bool:
    s = sum_of_squares(row)
    for ulps in (0, -1, 1):
        worst, differing = model_vs_oracle(row, w, eps, act, ulps, s=s)
        if not meets_bar(worst[0], differing[0] / row.shape[1]):
            return False
    return True


def poisoned_rows(K: int, act: str) -> np.ndarray:
    """[2, K]: a randn row with one NaN, another with one inf."""
    rng = np.random.RandomState(K + 5)
    p = O.round_to(rng.randn(2, K).astype(f32), act)
    p[0, rng.randint(K)] = np.nan
    p[1, rng.randint(K)] = np.inf
    return p


SPLITK_SPLITS = (7, 9, 12, 16, 17, 25)      # SP = 7; the generic body: remainders 0, 3 and 7, a second batch of eight, a third
SPLITK_SHAPE = (70, 264, 128)               # M, N, group size; K = 128 * split: one chunk per slab


def generic_reduce_trips(splits: int):
    """(batches of eight, remainder slabs) of splitk_reduce_kernel<ACT, 0>: slab 0 starts the sum, `for (; sp + 8 <= splits; sp += 8)`."""
    return (splits - 1) // 8, (splits - 1) % 8
