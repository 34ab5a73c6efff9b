"""How the decode kernels of the two weight-only linears (gptqhip_fp8.hip: fp8_decode_kernel; gptqhip_fp4.hip: fp4_decode_kernel) deal the
128-row chunks of K to the waves of a block, which 16-column tiles straddle two scale rows, and a float32 model of the decode summation built
on that deal (a helper, not a test; used by tests/test_linear_wave_model_cpu.py, tests/test_gpu_fp8_geometry.py and
tests/test_gpu_fp4_geometry.py).

Both kernels give wave w of W = min(k*DecodeWaves, chunks) the CONTIGUOUS range [w chunks / W, (w + 1) chunks / W) and run it in trips of
`ahead` chunks -- the rule moe_wave_model.contiguous_deal restates -- so a wave of more than `ahead` chunks carries acc / tot across trips,
addresses `base + u` with base > c0, and clamps the surplus loads of a ragged last trip to c1 - 1.  The constants are READ from the kernel
sources by name, so a changed constant changes what this model says the test shapes reach."""
import numpy as np

import fp4_oracle as F4
import fp8_oracle as F
from moe_wave_model import CHUNK_K, contiguous_deal, kernel_constant

TILE_N = 16              # columns per tile (gptqhip_device.h: kTileN)

kFp8DecodeWaves = kernel_constant("gptqhip_fp8.hip", "kFp8DecodeWaves")
kFp8Ahead = kernel_constant("gptqhip_fp8.hip", "kFp8Ahead")
kFp8GemmCT = kernel_constant("gptqhip_fp8.hip", "kFp8GemmCT")
kFp8GemmWaves = kernel_constant("gptqhip_fp8.hip", "kFp8GemmWaves")
kFp4DecodeWaves = kernel_constant("gptqhip_fp4.hip", "kFp4DecodeWaves")
kFp4Ahead = kernel_constant("gptqhip_fp4.hip", "kFp4Ahead")
kFp4WideAhead = kernel_constant("gptqhip_fp4.hip", "kFp4WideAhead")
kFp4WideNT = kernel_constant("gptqhip_fp4.hip", "kFp4WideNT")
kFp4WideTiles = kernel_constant("gptqhip_fp4.hip", "kFp4WideTiles")

# ---- the shapes of the geometry tests ---------------------------------------------------------------------------------------------------------
LAYOUTS = {"tensor": ("tensor", None), "row": ("row", None)}
for _br, _bc in ((16, 128), (24, 1408), (8, 4224), (24, 640), (1, 640), (3, 1664), (1, 128), (3, 128), (8, 384), (24, 128), (24, 384), (34, 384),
                 (136, 1152)):
    LAYOUTS[f"b{_br}x{_bc}"] = ("block", (_br, _bc))
N_NARROW = 48
FP8_TABLE = {4224: ("row", "tensor", "b16x128", "b24x1408", "b8x4224"),      # K -> scale layouts, N = 48
             7040: ("row", "b16x128", "b24x640", "b1x640"),
             8320: ("row", "b3x1664"),
             384: ("b1x128", "b3x128", "b8x384", "b24x128", "b24x384")}
FP8_TABLE_CASES = [(K, N_NARROW, l) for K, ls in FP8_TABLE.items() for l in ls]
FP8_GENERAL_EXTRA = [(1152, 272, "b34x384"), (1152, 272, "b136x1152")]      # the general kernel: several K blocks of three chunks, split tiles
FP8_SCALE_ROW_CASES = [(384, N_NARROW, l) for l in FP8_TABLE[384]] + FP8_GENERAL_EXTRA
FP4_DEEP_K = (4224, 7040, 8320)
FP4_WIDE = (4224, 16384)
# test_nibble_and_block_placement's deep case, K = 4224, N = 48: (column, 16-wide scale block); a chunk holds eight blocks
FP4_DEEP_PLACEMENT = [(17, 8 * 32 + 5),      # chunk 32: wave 7's second trip, and the chunk its surplus loads repeat
                      (0, 8 * 31 + 2),       # chunk 31: wave 7's first trip, u = 3
                      (47, 8 * 3 + 7),       # chunk 3: wave 0, u = 3
                      (32, 8 * 13 + 0)]      # chunk 13: wave 3, u = 1


def block_of(layout):
    return LAYOUTS[layout][1]


# ---- deals ---------------------------------------------------------------------------------------------------------------------------------------
def fp8_decode(K: int, block=None):
    chunks = K // CHUNK_K
    return contiguous_deal(chunks, min(kFp8DecodeWaves, chunks), kFp8Ahead, block[1] // CHUNK_K if block else None)


def fp4_is_wide(N: int) -> bool:
    return N // TILE_N >= kFp4WideTiles


def fp4_ahead(N: int) -> int:
    return kFp4WideAhead if fp4_is_wide(N) else kFp4Ahead


def fp4_decode(K: int, N: int):
    chunks = K // CHUNK_K
    return contiguous_deal(chunks, min(kFp4DecodeWaves, chunks), fp4_ahead(N))


def trips(deal):
    """Chunks consumed per trip of the `for (base ..)` loop, per wave."""
    return [[len(r) for r in w.rounds] for w in deal]


def slot_of(deal, ck: int):
    """(wave, trip, u) of the look-ahead slot that consumes chunk ck."""
    for i, w in enumerate(deal):
        for t, r in enumerate(w.rounds):
            if ck in r:
                return i, t, r.index(ck)
    raise KeyError(ck)


def flush_slots(deal, kind: str):
    """{(wave, trip, u)} of every flush of this kind ("block": a K block ends; "share": the wave's share of one ends)."""
    return {slot_of(deal, ck) for w in deal for ck, k in w.flushes if k == kind}


def clamped_loads(deal, ahead: int):
    """[(wave, trip, chunk the surplus loads repeat, how many)] of every ragged trip."""
    return [(i, t, w.chunks[-1], ahead - len(r)) for i, w in enumerate(deal) for t, r in enumerate(w.rounds) if len(r) < ahead]


# ---- scale rows ----------------------------------------------------------------------------------------------------------------------------------
def scale_rows_of_tile(tile: int, br: int):
    return sorted({(tile * TILE_N + c) // br for c in range(TILE_N)})


def straddling_tiles(N: int, br: int):
    """Tiles whose 16 columns lie in more than one scale row."""
    return [t for t in range(N // TILE_N) if len(scale_rows_of_tile(t, br)) > 1]


def gemm_waves(N: int):
    """fp8_gemm_kernel: [(first tile, tiles)] of the waves that own columns; wave g takes tiles kFp8GemmCT g .."""
    tiles = N // TILE_N
    return [(t0, min(kFp8GemmCT, tiles - t0)) for t0 in range(0, tiles, kFp8GemmCT)]


def gemm_waves_with_tiles_in_different_scale_rows(N: int, br: int):
    """Waves (by first tile) whose column tiles do not read the same scale rows."""
    return [t0 for t0, n in gemm_waves(N) if len({tuple(scale_rows_of_tile(t0 + i, br)) for i in range(n)}) > 1]


def scale_row_ladder(N: int, K: int, block) -> np.ndarray:
    """scale_inv [N / br, K / bc] whose neighbouring scale rows differ by a factor of at least 8 in every K block, none a power of two: row i
    is 3.1 x 9^((2 i) % 5) x a jitter of 1 .. 1.37 that no two rows share (exponents of neighbours differ by 2 or 3: 81 / 1.37 > 8), K blocks
    cycle through 1, 1.7, 2.89."""
    br, bc = block
    i = np.arange(N // br)
    rows = 3.1 * 9.0 ** ((2 * i) % 5) * (1.0 + 0.37 * ((i * 0.6180339887) % 1.0))
    cols = 1.7 ** (np.arange(K // bc) % 3)
    s = (rows[:, None] * cols[None, :]).astype(np.float32)
    if s.shape[0] > 1:
        assert np.maximum(s[1:] / s[:-1], s[:-1] / s[1:]).min() >= 8.0
    return s


# ---- one-hot rows --------------------------------------------------------------------------------------------------------------------------------
def one_hot_ks(chunks: int):
    """One k per activation row: row i sits in chunk i % chunks at position 32 j + 8 rq + e with (j, rq, e in {0, 7}) cycling through all 32
    combinations -- every K-step, every row quarter, the first and the last byte of a lane's eight.  max(chunks, 32) rows."""
    ks = []
    for i in range(max(chunks, 32)):
        j, rq, e = i & 3, (i >> 2) & 3, 7 * ((i >> 4) & 1)
        ks.append(CHUNK_K * (i % chunks) + 32 * j + 8 * rq + e)
    return ks


def one_hot_x(K: int) -> np.ndarray:
    ks = one_hot_ks(K // CHUNK_K)
    x = np.zeros((len(ks), K))
    x[np.arange(len(ks)), ks] = 1.0
    return x


# ---- float32 model of the decode summation ---------------------------------------------------------------------------------------------------------
f32 = np.float32
MUTATIONS = ("acc_reset", "first_trip_loads", "flush_from_c0", "tile_scale_row", "drop_later_trips")


def _chunk(acc, x, w, ck):
    for k in range(CHUNK_K * ck, CHUNK_K * ck + CHUNK_K):      # sequential within a chunk
        acc = acc + x[:, k, None] * w[None, :, k]
    return acc


def _waves(deal, ahead, x, w, rs, cpb, mutation):
    """The partial sums of every wave, added in wave order.  rs: [N, K blocks] reciprocal scales per column, or None (no flushes)."""
    M, N = x.shape[0], w.shape[0]
    s = np.zeros((M, N), f32)
    for wave in deal:
        c0, c1 = wave.chunks[0], wave.chunks[-1] + 1
        acc, tot = np.zeros((M, N), f32), np.zeros((M, N), f32)
        for base in range(c0, c1, ahead):
            if mutation == "acc_reset":
                acc = np.zeros((M, N), f32)
            if mutation == "drop_later_trips" and base - c0 >= 2 * ahead:
                continue
            for u in range(ahead):
                ck = base + u
                if ck >= c1:
                    break
                src = min(c0 + u, c1 - 1) if mutation == "first_trip_loads" else ck      # the chunk the slot's loads took
                acc = _chunk(acc, x, w, src)
                if rs is not None:
                    ends = (ck + 1 - c0) % cpb == 0 if mutation == "flush_from_c0" else (ck + 1) % cpb == 0
                    if ends or ck + 1 == c1:
                        tot = tot + acc * rs[None, :, src // cpb]
                        acc = np.zeros((M, N), f32)
        s = s + (acc if rs is None else tot)
    return s


def fp8_decode_model(x, codes, scale_inv, method, block, bias, act, mutation=None) -> np.ndarray:
    """fp8_decode_kernel in float32 numpy: sequential within a chunk, chunks in wave order, tot += acc * r at the modelled flushes, waves added
    in wave order, scale (tensor / row) and bias in fp32, one rounding.  `mutation`: one of MUTATIONS, a deliberately wrong kernel."""
    N, K = codes.shape
    x32, w32 = np.asarray(x, np.float64).astype(f32), F.E4M3[codes].astype(f32)
    r = f32(1.0) / np.asarray(scale_inv, f32)
    rs = cpb = None
    if method == "block":
        cols = np.arange(N)
        first = cols // TILE_N * TILE_N if mutation == "tile_scale_row" else cols
        rs, cpb = r[first // block[0]], block[1] // CHUNK_K
    s = _waves(fp8_decode(K, block if method == "block" else None), kFp8Ahead, x32, w32, rs, cpb, mutation)
    if method != "block":
        s = s * (r[None, :] if method == "row" else r)
    if bias is not None:
        s = s + np.asarray(bias, np.float64).astype(f32)[None, :]
    return F.round_to(s, act)


def fp4_decode_model(x, codes, scale, s2, bias, act, mutation=None) -> np.ndarray:
    """fp4_decode_kernel (one tile per block, kFp4Ahead chunks per trip) in float32 numpy: exact block-scaled weights, no flushes, s2 and the
    bias in fp32, one rounding."""
    N, K = codes.shape
    x32, w32 = np.asarray(x, np.float64).astype(f32), F4.block_weights64(codes, scale).astype(f32)
    s = _waves(fp4_decode(K, N), fp4_ahead(N), x32, w32, None, None, mutation) * f32(s2)
    if bias is not None:
        s = s + np.asarray(bias, np.float64).astype(f32)[None, :]
    return F.round_to(s, act)


def elementwise_excess(got, x, w64, act) -> np.ndarray:
    """|got - y64| - |y_once - y64| - 1e-4 S, S = |x| . |W|^T: the scale-ladder bar of tests/test_gpu_fp8.py; <= 0 passes."""
    x = np.asarray(x, np.float64)
    ref = x @ w64.T
    S = np.abs(x) @ np.abs(w64).T
    return np.abs(got - ref) - np.abs(F.round_to(ref, act) - ref) - 1e-4 * S
