"""What the deep shapes of tests/test_gpu_fp8_geometry.py and tests/test_gpu_fp4_geometry.py reach, derived from the kernels' constants
(tests/linear_wave_model.py), and a float32 model of the decode summation against the bars those tests hold the kernels to.  No GPU.

If a kernel constant changes (kFp8DecodeWaves, kFp8Ahead, kFp4DecodeWaves, kFp4Ahead, kFp4WideAhead, kFp4WideNT, kFp4WideTiles, kFp8GemmCT,
kFp8GemmWaves), the first group of tests says which shape no longer reaches the code it is there for.  The second group shows that the bars
are attainable by the documented arithmetic for the seeds used, and that five deliberately wrong kernels, modelled in Python, miss them."""
import numpy as np
import pytest

import fp4_oracle as F4
import fp8_oracle as F
import linear_wave_model as LM
import test_gpu_fp8 as T8
from moe_wave_model import CHUNK_K, blocks_cut_by_a_wave_boundary


def test_constants_are_the_kernels():
    assert (LM.kFp8DecodeWaves, LM.kFp8Ahead, LM.kFp8GemmCT, LM.kFp8GemmWaves) == (8, 4, 2, 4)
    assert (LM.kFp4DecodeWaves, LM.kFp4Ahead, LM.kFp4WideAhead, LM.kFp4WideNT, LM.kFp4WideTiles) == (8, 4, 2, 4, 1024)


def test_the_decode_shapes_from_before_run_one_trip_per_wave():
    """The gap: no decode shape of tests/test_gpu_fp8.py or tests/test_gpu_fp4.py carries acc / tot into a second trip of the one-tile
    instantiations; the wide FP4 variant stops at two."""
    for K, N, layout in T8.DECODE_SHAPES:
        assert all(len(t) == 1 for t in LM.trips(LM.fp8_decode(K, T8.LAYOUTS[layout][1]))), (K, layout)
    for K in (128, 256, 384, 640, 1152, 4096):       # every K of both files: parametrised shapes, ladders, placement, invariance, modules
        assert all(len(t) == 1 for t in LM.trips(LM.fp8_decode(K))), K
        assert all(len(t) == 1 for t in LM.trips(LM.fp4_decode(K, 272))), K
    for K, N in ((384, 16384), (2176, 16400)):
        assert LM.fp4_is_wide(N) and max(len(t) for t in LM.trips(LM.fp4_decode(K, N))) <= 2
    assert LM.trips(LM.fp4_decode(2176, 16400))[7] == [2, 1]
    # scale rows: br = 16 and 128 never split a tile; 48 at N = 48 is one scale row
    for name, (method, block) in T8.LAYOUTS.items():
        if block:
            assert not LM.straddling_tiles(48 if block[0] == 48 else 256, block[0]), name
    # the general kernel's K blocks of two chunks: K = 256 only, a single block
    assert [K for K, N, l in T8.GENERAL_SHAPES if l == "b48x256"] == [256]


def test_k4224_one_ragged_second_trip_and_blocks_longer_than_a_round():
    K = 4224
    deal = LM.fp8_decode(K)
    assert K // CHUNK_K == 33 and LM.trips(deal) == [[4]] * 7 + [[4, 1]]
    assert LM.clamped_loads(deal, LM.kFp8Ahead) == [(7, 1, 32, 3)]                      # chunk 32 loaded four times, consumed once
    assert LM.trips(LM.fp4_decode(K, 48)) == LM.trips(deal)
    d = LM.fp8_decode(K, LM.block_of("b24x1408"))                                       # 11 chunks per K block
    assert LM.flush_slots(d, "block") == {(2, 0, 2), (5, 0, 1), (7, 1, 0)}              # mid-round at u = 2, u = 1; u = 0 of a second trip
    assert LM.flush_slots(d, "share") == {(w, 0, 3) for w in range(7) if w not in (2, 5)} | {(2, 0, 3), (5, 0, 3)}
    assert blocks_cut_by_a_wave_boundary(d, 11) == [0, 1, 2]
    d = LM.fp8_decode(K, LM.block_of("b8x4224"))                                        # one K block of 33 chunks
    assert LM.flush_slots(d, "block") == {(7, 1, 0)} and LM.flush_slots(d, "share") == {(w, 0, 3) for w in range(7)}
    d = LM.fp8_decode(K, LM.block_of("b16x128"))
    assert all(len(w.flushes) == len(w.chunks) for w in d)
    assert LM.straddling_tiles(48, 24) == [1] and LM.straddling_tiles(48, 8) == [0, 1, 2] and not LM.straddling_tiles(48, 16)
    # the FP4 placement blocks of tests/test_gpu_fp4.py
    d4 = LM.fp4_decode(K, 48)
    assert [LM.slot_of(d4, blk // 8) for n, blk in LM.FP4_DEEP_PLACEMENT] == [(7, 1, 0), (7, 0, 3), (0, 0, 3), (3, 0, 1)]
    assert LM.clamped_loads(d4, LM.kFp4Ahead)[0][2] == LM.FP4_DEEP_PLACEMENT[0][1] // 8
    assert len({n // 16 for n, blk in LM.FP4_DEEP_PLACEMENT}) == 3 and all(blk >= 16 for n, blk in LM.FP4_DEEP_PLACEMENT)


def test_k7040_every_wave_runs_a_ragged_second_trip_and_blocks_end_at_every_u():
    K = 7040
    deal = LM.fp8_decode(K)
    assert K // CHUNK_K == 55 and LM.trips(deal) == [[4, 2]] + [[4, 3]] * 7
    assert [(w, t, n) for w, t, ck, n in LM.clamped_loads(deal, LM.kFp8Ahead)] == [(0, 1, 2)] + [(w, 1, 1) for w in range(1, 8)]
    assert LM.trips(LM.fp4_decode(K, 48)) == LM.trips(deal)
    d = LM.fp8_decode(K, LM.block_of("b24x640"))                                        # five chunks per K block
    ends = LM.flush_slots(d, "block")
    assert {u for w, t, u in ends if t == 0} == {0, 1, 2, 3} and {u for w, t, u in ends if t == 1} >= {0, 1, 2}
    # wave boundaries at chunks 6, 13, 20, .., 48 against K blocks of five: all but 20 cut a block, each shared by two waves
    assert len(ends) == 11 and len(blocks_cut_by_a_wave_boundary(d, 5)) == 6 and all(len(w.flushes) >= 2 for w in d)
    share = LM.flush_slots(d, "share")
    assert len(share) == 6 and {t for w, t, u in share} == {1}                          # every share ends in a second trip
    assert LM.straddling_tiles(48, 1) == [0, 1, 2]


def test_k8320_two_full_trips_and_a_third():
    K = 8320
    deal = LM.fp8_decode(K)
    assert K // CHUNK_K == 65 and LM.trips(deal) == [[4, 4]] * 7 + [[4, 4, 1]]
    assert LM.clamped_loads(deal, LM.kFp8Ahead) == [(7, 2, 64, 3)]
    assert LM.trips(LM.fp4_decode(K, 48)) == LM.trips(deal)
    d = LM.fp8_decode(K, LM.block_of("b3x1664"))                                        # 13 chunks per K block
    assert blocks_cut_by_a_wave_boundary(d, 13) == [0, 1, 2, 3, 4]                      # every block spans waves and trips
    assert LM.flush_slots(d, "block") == {(1, 1, 0), (3, 0, 1), (4, 1, 2), (6, 0, 3), (7, 2, 0)}
    assert LM.straddling_tiles(48, 3) == [0, 1, 2]


def test_k384_one_chunk_per_wave_and_tiles_that_straddle_scale_rows():
    assert LM.trips(LM.fp8_decode(384)) == [[1]] * 3
    for layout, rows_in_tile_1 in (("b1x128", 16), ("b3x128", 6), ("b8x384", 2), ("b24x128", 2), ("b24x384", 2)):
        br = LM.block_of(layout)[0]
        assert len(LM.scale_rows_of_tile(1, br)) == rows_in_tile_1 and 1 in LM.straddling_tiles(48, br), layout
    assert LM.straddling_tiles(48, 24) == [1]                                           # tiles 0 and 2 lie in one scale row each


def test_the_272_column_cases_split_tiles_and_waves_of_the_general_kernel():
    K, N = 1152, 272
    waves = LM.gemm_waves(N)
    assert len(waves) == 9 and waves[-1] == (16, 1)                                     # a ragged last wave: one tile of its two
    assert -(-len(waves) // LM.kFp8GemmWaves) == 3                                      # three blocks, the last with one live wave
    br, bc = LM.block_of("b34x384")
    assert bc // CHUNK_K == 3 and K // bc == 3                                          # three K blocks of three chunks
    assert LM.straddling_tiles(N, br) == [2, 4, 6, 8, 10, 12, 14]                       # the boundaries 34, 68, .., 238
    assert LM.gemm_waves_with_tiles_in_different_scale_rows(N, br) == [2, 4, 6, 8, 10, 12, 14]   # every full wave but the first
    br, bc = LM.block_of("b136x1152")
    assert LM.straddling_tiles(N, br) == [8] and LM.gemm_waves_with_tiles_in_different_scale_rows(N, br) == [8]
    assert LM.scale_rows_of_tile(8, br) == [0, 1] and LM.scale_rows_of_tile(9, br) == [1]


def test_fp4_wide_k4224_runs_a_third_trip():
    K, N = LM.FP4_WIDE
    assert LM.fp4_is_wide(N) and N // LM.TILE_N % LM.kFp4WideNT == 0
    assert LM.trips(LM.fp4_decode(K, N)) == [[2, 2]] * 7 + [[2, 2, 1]]
    assert LM.trips(LM.fp4_decode(K, 32)) == [[4]] * 7 + [[4, 1]]                       # the 32-column layer it is compared with


def test_one_hot_rows_cover_every_chunk_k_step_quarter_and_both_end_bytes():
    for K in list(LM.FP8_TABLE) + [1152]:
        chunks = K // CHUNK_K
        ks = LM.one_hot_ks(chunks)
        assert {k // CHUNK_K for k in ks} == set(range(chunks))
        assert {((k % 128) >> 5, ((k % 128) >> 3) & 3, k & 7) for k in ks} == {(j, rq, e) for j in range(4) for rq in range(4) for e in (0, 7)}
        assert len(ks) >= 17 and len(ks) == max(chunks, 32)


# ---- the bars are attainable by the documented arithmetic; the wrong kernels miss them ---------------------------------------------------------
def bar(c):
    return max(F.rel64(c["chain"], c["y64"]), F.rel64(c["y_once"], c["y64"])) + 1e-4


@pytest.mark.parametrize("act", ["fp16", "bf16"])
@pytest.mark.parametrize("K,N,layout", LM.FP8_TABLE_CASES)
def test_fp8_decode_summation_fits_the_dense_bar(K, N, layout, act):
    method, block = LM.LAYOUTS[layout]
    c = F.case(16, K, N, method, block, act, True)
    e = F.rel64(LM.fp8_decode_model(c["x"], c["codes"], c["scale_inv"], method, block, c["bias"], act), c["y64"])
    print(f"fp8 decode order model K={K} {layout} M=16 {act}: rel64 {e:.3e} bar {bar(c):.3e}")
    assert e <= bar(c)


# (mutation, K, layout): a shape of the table that reaches the edited line
FP8_MUTANTS = [("acc_reset", 7040, "row"), ("acc_reset", 8320, "b3x1664"), ("first_trip_loads", 7040, "row"), ("first_trip_loads", 4224, "b24x1408"),
               ("flush_from_c0", 7040, "b24x640"), ("flush_from_c0", 4224, "b24x1408"), ("flush_from_c0", 8320, "b3x1664")]


@pytest.mark.parametrize("act", ["fp16", "bf16"])
@pytest.mark.parametrize("mutation,K,layout", FP8_MUTANTS)
def test_a_wrong_fp8_decode_loop_misses_the_dense_bar(mutation, K, layout, act):
    method, block = LM.LAYOUTS[layout]
    c = F.case(16, K, LM.N_NARROW, method, block, act, True)
    e = F.rel64(LM.fp8_decode_model(c["x"], c["codes"], c["scale_inv"], method, block, c["bias"], act, mutation), c["y64"])
    print(f"fp8 decode order model, {mutation}, K={K} {layout} M=16 {act}: rel64 {e:.3e} bar {bar(c):.3e}")
    assert e > 2 * bar(c)


def test_the_mutations_leave_the_shapes_from_before_alone():
    """At K = 4096 (one full trip per wave, K blocks in step with the rounds) the three loop mutations compute what the kernel computes."""
    for layout in ("row", "b16x128"):
        method, block = T8.LAYOUTS[layout]
        c = F.case(3, 4096, 16, method, block, "fp16", True)
        good = LM.fp8_decode_model(c["x"], c["codes"], c["scale_inv"], method, block, c["bias"], "fp16")
        for mutation in ("acc_reset", "first_trip_loads", "flush_from_c0", "tile_scale_row"):
            assert np.array_equal(good, LM.fp8_decode_model(c["x"], c["codes"], c["scale_inv"], method, block, c["bias"], "fp16", mutation)), mutation


@pytest.mark.parametrize("act", ["fp16", "bf16"])
@pytest.mark.parametrize("K,N,layout", LM.FP8_SCALE_ROW_CASES)
def test_scale_rows_element_by_element_model_fits_and_the_tiles_first_row_does_not(K, N, layout, act):
    """The scale-row cases with neighbouring scale rows a factor >= 8 apart: y_once and the float32 model stay inside
    |got - y64| <= |y_once - y64| + 1e-4 S; a model that takes the scale row of the tile's first column for all sixteen does not."""
    block = LM.block_of(layout)
    codes, scale_inv = F.layer(K, N, "block", block)[0], LM.scale_row_ladder(N, K, block)
    x = F.make_x(31, 16, K, act)
    w64 = F.weights64(codes, scale_inv, block)
    assert (LM.elementwise_excess(F.round_to(x @ w64.T, act), x, w64, act) <= 0).all()
    good = LM.elementwise_excess(LM.fp8_decode_model(x, codes, scale_inv, "block", block, None, act), x, w64, act)
    wrong = LM.elementwise_excess(LM.fp8_decode_model(x, codes, scale_inv, "block", block, None, act, "tile_scale_row"), x, w64, act)
    S = np.abs(x) @ np.abs(w64).T
    print(f"fp8 scale rows K={K} N={N} {layout} {act}: model excess / S {float((good / S).max()):.3e}, "
          f"first-row model: {int((wrong > 0).sum())} of {wrong.size} outside, worst excess / S {float((wrong / S).max()):.3e}")
    assert (good <= 0).all()
    cols = np.arange(N)
    moved = (cols // LM.TILE_N * LM.TILE_N) // block[0] != cols // block[0]              # columns whose scale row the mutation changes
    assert moved.any() and (wrong[:, ~moved] <= 0).all()
    assert (wrong[:, moved] > 0).mean() > 0.9 and (wrong[:, moved] > 0).any(axis=0).all()
    assert float((wrong / S).max()) > 100 * 1e-4                                          # a wide margin


@pytest.mark.parametrize("act", ["fp16", "bf16"])
@pytest.mark.parametrize("K", LM.FP4_DEEP_K)
def test_fp4_decode_summation_fits_the_dense_bar_and_a_dropped_third_trip_does_not(K, act):
    N = LM.N_NARROW
    c = F4.case(16, K, N, act, True)
    b = max(F4.rel64(c["chain"], c["y64"]), F4.rel64(c["y_once"], c["y64"])) + 1e-4
    e = F4.rel64(LM.fp4_decode_model(c["x"], c["codes"], c["scale"], F4.S2, c["bias"], act), c["y64"])
    wrong = LM.fp4_decode_model(c["x"], c["codes"], c["scale"], F4.S2, c["bias"], act, "drop_later_trips")
    ew = F4.rel64(wrong, c["y64"])
    print(f"fp4 decode order model K={K} M=16 {act}: rel64 {e:.3e} bar {b:.3e}; without the trips after the second: {ew:.3e}")
    assert e <= b
    if K == 8320:
        assert ew > 2 * b
    else:                                                                                # (no third trip there: the wide variant's case)
        assert ew == e
