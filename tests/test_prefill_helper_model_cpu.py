"""CPU side of tests/test_gpu_prefill_helpers.py: the shapes of that file reach every instantiation, mask state and loop trip of the three
helper kernels of the prefill path (geometry restated from the launchers' source text), and the project's bar for rmsnorm_gather -- at most
2 ulps of the 16-bit dtype from O.rmsnorm_ref, at most 1e-3 of the elements differing -- is attainable on every new case: a float32 model of
the kernel's own order of summation meets it, also with the reciprocal square root one fp32 ulp off either way (the device's rsqrtf is not
correctly rounded), while two wrong treatments of eps miss it by far."""
import numpy as np
import pytest

import prefill_helper_model as P
from oracle import gptq_oracle as O


def test_constants_are_the_ones_the_cases_were_chosen_for():
    """The K list names 'the smallest K that reaches its case' for these thresholds; a changed launcher must come back here."""
    assert P.NORM == P.GATHER == P.Launcher(8192, 4, 2, 2048, ((4, 1), (4, 2), (4, 4), (2, 6), (2, 8)))
    assert (P.kGatherMaxK, P.GATHER_MIN_ROWS, P.SIMPLE_ROWS_CAP) == (16384, 8, 1024)


def test_k_list_reaches_every_instantiation_and_mask_state():
    for (R, IT), ks in P.K_CASES.items():
        for K in ks:
            for M in P.variant_rows_of(K) + P.GATHER_LDS_ROWS:
                g = P.norm_geometry(M, K)
                assert (g.R, g.IT) == (R, IT) and g.trips == 1, (M, K, g)
                if M >= P.GATHER_MIN_ROWS:
                    assert P.gather_geometry(M, K) == g
    seen = {(P.norm_geometry(1, K).R, P.norm_geometry(1, K).IT) for K in P.K_LIST}
    assert seen == set(P.NORM.instantiations) == set(P.GATHER.instantiations)
    geo = {K: P.norm_geometry(1, K) for K in P.K_LIST}
    # a piece that is live in only part of a wave: one thread (8), 33 threads (264), thread 0 of a second / third / .. piece, a wave and a half (11008)
    assert [K for K in P.K_LIST if P.has_partial_wave_piece(geo[K], K)] == [8, 264, 2056, 4104, 8200, 11008, 12296]
    assert (P.live_threads(8, 0), P.live_threads(264, 0), P.live_threads(2056, 1), P.live_threads(4104, 2)) == (1, 33, 1, 1)
    assert (P.live_threads(8200, 4), P.live_threads(11008, 5), P.live_threads(12296, 6)) == (1, 96, 1)
    # ... and whole waves of a piece dead while others live (3584: three of four, 5120: two)
    assert (P.live_threads(3584, 1), P.live_threads(5120, 2)) == (192, 128)
    # a wholly dead last piece, in every instantiation that has more than one
    assert [K for K in P.K_LIST if P.has_dead_last_piece(geo[K], K)] == [4104, 5120, 8200, 12296]
    assert [geo[K].pieces for K in (4104, 5120, 8200, 12296)] == [3, 3, 5, 7]
    # ... and every piece of every thread live: the largest K of each instantiation's range that the list holds
    assert all(P.live_threads(K, geo[K].IT - 1) == P.THREADS for K in (2048, 12288, 16384))
    # M: a single row, a partly filled pass, one row more than a pass, several passes
    for K in P.K_LIST:
        R = geo[K].R
        assert P.variant_rows_of(K) == ((1, 3, 5, 9) if R == 4 else (1, 3, 9))
        assert {M % R for M in P.variant_rows_of(K)} >= {1, R - 1}
    assert max(P.K_LIST) == P.NORM_MAX_K and 2 * (max(P.K_LIST) - 1) == 32766


def test_trip_shapes_reach_later_trips_and_short_passes():
    """(M, K) of the loop-trip tests: a second trip with R = 4 and with R = 2, a third with R = 4, and in each shape a last pass with fewer than
    R live rows inside the last trip.  (A third trip with R = 2 would need M > 8192 rows of K > 8192: 134 MB per tensor, twice the size the
    suite allows itself; the loop is the same code in every instantiation.)"""
    g = {s: P.norm_geometry(*s) for s in P.TRIP_SHAPES}
    assert [(x.R, x.IT, x.trips) for x in g.values()] == [(4, 1, 2), (4, 1, 3), (2, 6, 2)]
    for (M, K), x in g.items():
        assert x.grid == P.NORM.grid_cap and P.short_pass_in_later_trip(x, M), (M, K, x)
        assert P.gather_geometry(M, K) == x
        assert P.trip_of_row(x, M - 1) == x.trips - 1 and M % x.R == 1      # the last row sits alone in a pass of the last trip
    assert not any(P.short_pass_in_later_trip(P.norm_geometry(M, K), M) for K in P.K_LIST for M in P.variant_rows_of(K))


def test_gather_shapes_reach_the_simple_kernel_both_ways_and_its_second_trip():
    reasons = {s: P.simple_gather_reason(*s) for s in P.GATHER_SIMPLE_SHAPES}
    assert reasons == {(1, 264): "few", (7, 264): "few", (9, 16392): "long", (9, 28672): "long", (1030, 16392): "long"}
    assert [P.gather_geometry(*s).trips for s in P.GATHER_SIMPLE_SHAPES] == [1, 1, 1, 1, 2]
    assert P.gather_geometry(1030, 16392).grid == (65, 1024)
    assert all(P.gather_geometry(M, K).kernel == "lds" for K in P.K_LIST for M in P.GATHER_LDS_ROWS)
    assert P.gather_geometry(8, 16384).kernel == "lds" and P.gather_geometry(8, 16392).kernel == "simple"      # either side of the limit


def test_split_k_list_reaches_sp7_and_the_generic_body():
    """Forced splits up to 8 are compile-time instantiations; from 9 slabs the generic body runs batches of eight plus a remainder."""
    assert P.SPLITK_SPLITS[0] == 7 and all(s > 8 for s in P.SPLITK_SPLITS[1:])
    assert [P.generic_reduce_trips(s) for s in P.SPLITK_SPLITS[1:]] == [(1, 0), (1, 3), (1, 7), (2, 0), (3, 0)]


# ---- the model --------------------------------------------------------------------------------------------------------------------------------
def test_model_order_of_summation_on_exact_integers():
    """On small integers every partial sum is exact, so any order gives the exact sum; on a row whose order matters the model differs from a
    plain left-to-right fp32 sum (it is a model of an order, not of a value)."""
    rng = np.random.RandomState(1)
    h = rng.randint(-8, 9, size=(5, 4104)).astype(np.float32)
    assert np.array_equal(P.sum_of_squares(h), (h.astype(np.float64) ** 2).sum(axis=1).astype(np.float32))
    x = O.round_to(rng.randn(64, 5120).astype(np.float32), "fp16")
    serial = np.zeros(64, np.float32)
    for k in range(x.shape[1]):
        serial = serial + x[:, k] * x[:, k]
    s = P.sum_of_squares(x)
    exact = (x.astype(np.float64) ** 2).sum(axis=1)
    assert (s != serial).any() and np.abs(s / exact - 1.0).max() < 4e-7 and np.abs(s / exact - 1.0).max() <= np.abs(serial / exact - 1.0).max()
    # thread t owns elements 8 (t + 256 it) .. + 7: a single large element lands in that thread's chain
    one = np.zeros((1, 4104), np.float32)
    one[0, 8 * (300 % 256 + 256) + 3] = 3.0
    assert P.thread_sums(one, 3)[0, 300 % 256] == 9.0 and P.thread_sums(one, 3).sum() == 9.0


@pytest.mark.parametrize("act", P.ACTS)
def test_normalise_with_the_oracles_statistics_is_the_oracle(act):
    """model_vs_oracle() evaluates only the rows whose 1 / rms differs between model and oracle; that rests on this identity."""
    for K, eps in ((264, 1e-6), (5120, 1e-3)):
        h, w = P.family_case(K, act, eps)
        assert np.array_equal(P.bits16(P.normalise(h, w, P.oracle_inv(h, eps), act), act), P.bits16(O.rmsnorm_ref(h, w, eps, act), act))
    h, w = P.plain_case(5, 2056, act)
    assert np.array_equal(P.bits16(P.normalise(h, w, P.oracle_inv(h, 1e-5), act), act), P.bits16(O.rmsnorm_ref(h, w, 1e-5, act), act))


def _report(tag, worst, differing, K):
    return f"{tag}: worst {int(worst.max())} ulps, {int(differing.sum())} of {worst.size * K} elements differ"


@pytest.mark.parametrize("act", P.ACTS)
@pytest.mark.parametrize("ulps", [0, -1, 1])
def test_model_meets_the_bar_on_the_geometry_cases(act, ulps):
    """Every (M, K) of the variants and loop-trip tests, whole-case bar (what the GPU test asserts)."""
    for K in P.K_LIST:
        h, w = P.plain_case(P.VARIANT_ROWS, K, act)
        for M in P.variant_rows_of(K):
            worst, differing = P.model_vs_oracle(h[:M], w, 1e-5, act, ulps)
            assert P.meets_bar(worst.max(), differing.sum() / (M * K)), _report((act, ulps, M, K), worst, differing, K)
    for M, K in P.TRIP_SHAPES:
        h, w = P.plain_case(M, K, act)
        worst, differing = P.model_vs_oracle(h, w, 1e-5, act, ulps)
        assert P.meets_bar(worst.max(), differing.sum() / (M * K)), _report((act, ulps, M, K), worst, differing, K)


@pytest.mark.parametrize("act", P.ACTS)
@pytest.mark.parametrize("K", P.EPS_K)
def test_model_meets_the_bar_on_every_row_family(act, K):
    """The eps and range cases, the bar applied to every family (row) on its own, with rsqrt exact and one fp32 ulp off either way."""
    for eps in P.EPS_LIST:
        h, w = P.family_case(K, act, eps)
        assert np.isfinite(h).all() and np.isfinite(P.sum_of_squares(h)).all()
        for ulps in (0, -1, 1):
            worst, differing = P.model_vs_oracle(h, w, eps, act, ulps)
            for f, name in enumerate(P.FAMILIES):
                assert P.meets_bar(worst[f], differing[f] / K), (act, K, eps, ulps, name, int(worst[f]), int(differing[f]))


def test_family_rows_are_rarely_drawn_again():
    """family_case draws a row again when the model says that it cannot meet the per-row bar whatever rsqrtf rounds to: that must stay the exception
    (a case list that needs many draws would be a list tuned to pass)."""
    draws = [d for act in P.ACTS for K in P.EPS_K for eps in P.EPS_LIST for d in P.family_draws(K, act, eps)]
    assert len(draws) == 2 * 3 * 3 * P.FAMILY_ROWS and max(draws) <= 2 and sum(d > 0 for d in draws) <= len(draws) // 20, draws


@pytest.mark.parametrize("act", P.ACTS)
@pytest.mark.parametrize("wrong", ["eps_inside", "no_eps"])
def test_wrong_treatments_of_eps_miss_the_bar(act, wrong):
    """rsqrt((sum + eps) / K) and rsqrt(sum / K): in every eps case some family misses the bar, and over the rows where eps matters (eps at
    least 1e-2 of the mean square, the tiny row, the padding rows with eps dropped) nearly every element differs -- the eps cases can fail."""
    for K in P.EPS_K:
        for eps in P.EPS_LIST:
            h, w = P.family_case(K, act, eps)
            worst, differing = P.model_vs_oracle(h, w, eps, act, 0, wrong)
            missed = [name for f, name in enumerate(P.FAMILIES) if not P.meets_bar(worst[f], differing[f] / K)]
            assert {f"eps/ms={r:g}" for r in P.EPS_RATIOS} | {"tiny"} <= set(missed), (act, K, eps, wrong, missed)
            rows = [f for f, name in enumerate(P.FAMILIES) if name.startswith("eps/ms") or name == "tiny"]
            live = (P.normalise(h[rows], w, P.oracle_inv(h[rows], eps), act) != 0.0).sum()      # (a zero stays a zero whatever 1 / rms is)
            assert differing[rows].sum() > 0.9 * live, (act, K, eps, wrong, int(differing[rows].sum()), int(live))


def test_poisoned_rows_hold_one_nan_and_one_inf():
    for act in P.ACTS:
        p = P.poisoned_rows(264, act)
        assert np.isnan(p[0]).sum() == 1 and np.isinf(p[1]).sum() == 1 and np.isfinite(p).sum() == p.size - 2
