"""What the deep MoE test shapes reach, derived from the kernels' constants (tests/moe_wave_model.py: the chunk-to-wave deal of the five inner
loops restated), and float32 models of the two few-token gate_up kernels' summation order against the stage-one bar.  No GPU.

If a kernel constant changes (kMoeAhead, kMoeGateUpWaves, kMoeDownWaves, kGroupedAhead, kGroupedGateUpWaves, kGroupedDownWaves), the first
group of tests says which shape of moe_oracle.DEEP_SHAPES / moe_fp8_oracle.DEEP_CASES no longer reaches the code it is there for."""
import numpy as np
import pytest

import fp8_oracle as F
import moe_fp8_oracle as MF
import moe_oracle as MO
import moe_wave_model as WM
from helpers import NORM_TOL, WEIGHT_RANGE_DTYPES, rel_err
from oracle import gptq_oracle as O


def lens(deal):
    return [len(w.chunks) for w in deal]


def round_lens(wave):
    return [len(r) for r in wave.rounds]


def test_constants_are_the_kernels():
    # quoted with their names; the look-ahead arrays of every shape of the suite BEFORE the deep shapes consumed slot u = 0 only
    assert (WM.kMoeGateUpWaves, WM.kMoeDownWaves, WM.kMoeAhead) == (8, 16, 4)
    assert (WM.kGroupedGateUpWaves, WM.kGroupedDownWaves, WM.kGroupedAhead) == (8, 16, 2)
    for H, I, E, k, gs in MO.SHAPES.values():
        for deal in (WM.int4_gate_up(H), WM.int4_down(I, k), WM.grouped_gate_up(H), WM.grouped_down(I)):
            assert WM.most_chunks(deal) == 1
        assert WM.combine_grid(H)[0] == 1


def test_the_deal_covers_every_chunk_exactly_once():
    for chunks in range(1, 40):
        for W in range(1, min(chunks, 16) + 1):
            for deal in (WM.strided_deal(chunks, W, 4), WM.strided_deal(chunks, W, 2), WM.contiguous_deal(chunks, W, 4, 3)):
                assert sorted(ck for w in deal for ck in w.chunks) == list(range(chunks))
                assert all(w.chunks for w in deal)
                for w in deal:      # block scales: nothing is left in acc at the end of a wave, and a flush only after a chunk the wave ran
                    assert not w.flushes or w.flushes[-1][0] == w.chunks[-1]


def test_int4_4224x128_reaches_a_ragged_second_round_and_five_combine_blocks():
    H, I, E, k, gs = MO.DEEP_SHAPES["4224x128e3k2"]
    few = WM.int4_gate_up(H)
    assert lens(few) == [5, 4, 4, 4, 4, 4, 4, 4] and round_lens(few[0]) == [4, 1]
    assert WM.has_ragged_last_round(few, WM.kMoeAhead) and WM.runs_a_second_trip(few)
    assert few[0].chunks == [0, 8, 16, 24, 32]                       # u * step addressing: u = 1 .. 3 consumed
    grp = WM.grouped_gate_up(H)
    assert lens(grp)[0] == 5 and round_lens(grp[0]) == [2, 2, 1] and WM.has_ragged_last_round(grp, WM.kGroupedAhead)
    assert WM.combine_grid(H) == (5, 32)                             # `blockIdx.y * 256` up to 4, a partial last block (`col >= p.H` exit)
    assert WM.most_chunks(WM.int4_down(I, k)) == 1                   # (the down side of this shape is the shallow one)


def test_int4_128x4224_reaches_the_same_on_the_down_side():
    H, I, E, k, gs = MO.DEEP_SHAPES["128x4224e3k2"]
    assert WM.few_down_wps(I, k) == 8
    few = WM.int4_down(I, k)
    assert lens(few) == [5, 4, 4, 4, 4, 4, 4, 4] and round_lens(few[0]) == [4, 1] and WM.has_ragged_last_round(few, WM.kMoeAhead)
    grp = WM.grouped_down(I)
    assert len(grp) == 16 and lens(grp) == [3] + [2] * 15 and round_lens(grp[0]) == [2, 1]
    assert WM.has_ragged_last_round(grp, WM.kGroupedAhead)


def test_int4_2304x1536_g256_puts_one_waves_chunks_in_three_groups():
    H, I, E, k, gs = MO.DEEP_SHAPES["2304x1536e4k4g256"]
    cpg = gs // WM.CHUNK_K
    assert cpg == 2
    few = WM.int4_gate_up(H)
    assert lens(few) == [3, 3, 2, 2, 2, 2, 2, 2] and few[0].chunks == [0, 8, 16] and few[1].chunks == [1, 9, 17]
    assert WM.most_groups(few, cpg) >= 3 and {ck // cpg for ck in few[1].chunks} == {0, 4, 8}
    assert WM.has_ragged_round(few, WM.kMoeAhead)                    # 3 of 4 look-ahead slots: the clamp runs
    assert WM.most_groups(WM.grouped_gate_up(H), cpg) >= 3 and WM.runs_a_second_trip(WM.grouped_gate_up(H))
    assert WM.few_down_wps(I, k) == 4
    down = WM.int4_down(I, k)
    assert lens(down) == [3, 3, 3, 3] and WM.most_groups(down, cpg) == 3
    blocks, last = WM.combine_grid(H)
    assert blocks == 3 and 0 < last < WM.COMBINE_THREADS


def test_int4_wide_top_k_shapes():
    H, I, E, k, gs = MO.DEEP_SHAPES["256x1408e8k8"]
    assert WM.few_down_wps(I, k) == 2 and WM.few_down_wps(I, k) * k == 16
    d = WM.int4_down(I, k)
    assert lens(d) == [6, 5] and round_lens(d[0]) == [4, 2] and round_lens(d[1]) == [4, 1] and WM.has_ragged_last_round(d, WM.kMoeAhead)
    H, I, E, k, gs = MO.DEEP_SHAPES["128x640e16k16"]
    assert WM.few_down_wps(I, k) == 1 and k == 16 and 16 * k == 256           # sixteen slots in red[]; T = 16: a 256-slot grid.y of gate_up
    d = WM.int4_down(I, k)
    assert lens(d) == [5] and round_lens(d[0]) == [4, 1]
    H, I, E, k, gs = MO.DEEP_SHAPES["256x384e7k7"]
    assert WM.kMoeDownWaves // k == 2 and WM.few_down_wps(I, k) * k == 14     # a top_k that does not divide 16: a 14-wave block
    assert lens(WM.int4_down(I, k)) == [2, 1]


def test_fp8_deep_cases_cut_k_blocks_at_wave_boundaries():
    H, I, E, k = MF.DEEP_SHAPES["4224x128e3k2"]
    block = MF.proj_layout("gu64x384_d32x128", "gate")[1]
    g = WM.fp8_gate_up(H, block)
    assert lens(g) == [4, 4, 4, 4, 4, 4, 4, 5] and round_lens(g[7]) == [4, 1] and WM.has_ragged_last_round(g, WM.kMoeAhead)
    cpb = block[1] // WM.CHUNK_K
    # wave boundaries at chunks 4, 8, .., 28 against K blocks of 3 chunks: five of the seven cut a block (12 and 24 are block ends), and the
    # waves left of those five flush "the wave's share of it ends here"
    assert cpb == 3 and len(WM.blocks_cut_by_a_wave_boundary(g, cpb)) == 5
    assert [w for w, _ in WM.share_end_flushes(g)] == [0, 1, 3, 4, 6]
    assert all(len(w.flushes) >= 2 for w in g)                                  # tot accumulates over more than one flush
    assert lens(WM.fp8_gate_up(H)) == lens(g) and not WM.fp8_gate_up(H)[0].flushes

    H, I, E, k = MF.DEEP_SHAPES["128x4224e3k2"]
    block = MF.proj_layout("gu128x128_d32x384", "down")[1]
    assert WM.few_down_wps(I, k) == 8
    d = WM.fp8_down(I, k, block)
    assert lens(d) == [4, 4, 4, 4, 4, 4, 4, 5] and len(WM.share_end_flushes(d)) == 5 and WM.has_ragged_last_round(d, WM.kMoeAhead)

    H, I, E, k = MF.DEEP_SHAPES["128x768e16k16"]
    block = MF.proj_layout("gu128x128_d32x256", "down")[1]
    d = WM.fp8_down(I, k, block)
    assert lens(d) == [6] and round_lens(d[0]) == [4, 2] and [ck for ck, _ in d[0].flushes] == [1, 3, 5] and block[1] // WM.CHUNK_K == 2

    H, I, E, k = MF.DEEP_SHAPES["256x768e8k8"]
    d = WM.fp8_down(I, k, block)
    assert [(w.chunks[0], w.chunks[-1] + 1) for w in d] == [(0, 3), (3, 6)]
    assert WM.share_end_flushes(d) == [(0, 2)] and WM.blocks_cut_by_a_wave_boundary(d, 2) == [1]     # a share ends mid-block

    H, I, E, k = MF.DEEP_SHAPES["256x384e7k7"]
    d = WM.fp8_down(I, k, (128, 128))
    assert WM.few_down_wps(I, k) * k == 14 and [(w.chunks[0], w.chunks[-1] + 1) for w in d] == [(0, 1), (1, 3)]


# ---- the stage-one bar is attainable by the kernels' own summation order ---------------------------------------------------------------------
@pytest.mark.parametrize("act,scale_dtype", WEIGHT_RANGE_DTYPES)
@pytest.mark.parametrize("shape", ["4224x128e3k2", "2304x1536e4k4g256"])
def test_int4_gate_up_summation_order_fits_the_stage_one_bar(shape, act, scale_dtype):
    T = 16
    k = MO.DEEP_SHAPES[shape][3]
    c, w = MO.case(shape, T, act, scale_dtype), MO.rounded_weights(shape, act, scale_dtype)
    got = np.zeros_like(c["act_ref"])
    for t in range(T):
        for j in range(k):
            e = int(c["ids"][t, j])
            g = O.round_to(WM.int4_gate_up_sums(c["x"][t], w[e]["gate"])[None], act)
            u = O.round_to(WM.int4_gate_up_sums(c["x"][t], w[e]["up"])[None], act)
            got[t * k + j] = O.silu_mul_ref(g, u, act)[0]
    err = rel_err(got, c["act_ref"])
    print(f"int4 gate_up order model {shape} T={T} {act}x{scale_dtype}: stage1 {err:.3e} (bar {NORM_TOL[act]:.0e})")
    assert err <= NORM_TOL[act], err


@pytest.mark.parametrize("act", ["fp16", "bf16"])
@pytest.mark.parametrize("layout", ["row", "b128x128", "gu64x384_d32x128"])
def test_fp8_gate_up_summation_order_fits_the_stage_one_bar(layout, act):
    shape, T = "4224x128e3k2", 16
    H, I, E, k = MF.DEEP_SHAPES[shape]
    block = MF.proj_layout(layout, "gate")[1]
    c, ex = MF.case(shape, layout, T, act), MF.experts_of(shape, layout)

    def sums(x, codes, scale_inv):
        r = np.float32(1.0) / np.asarray(scale_inv, np.float32)
        return WM.fp8_gate_up_sums(x, F.E4M3[codes].astype(np.float32), np.repeat(r, block[0], axis=0) if block else r, block)

    got = np.zeros_like(c["act_model"])
    for t in range(T):
        for j in range(k):
            e = int(c["ids"][t, j])
            g, u = F.round_to(sums(c["x"][t], *ex[e]["gate"]), act), F.round_to(sums(c["x"][t], *ex[e]["up"]), act)
            got[t * k + j] = F.round_to(F.round_to(MF.silu64(g), act) * u, act)
    err = rel_err(got, c["act_model"])
    print(f"fp8 gate_up order model {shape} {layout} T={T} {act}: stage1 {err:.3e} (bar {NORM_TOL[act]:.0e})")
    assert err <= NORM_TOL[act], err
