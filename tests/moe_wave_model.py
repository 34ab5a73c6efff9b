"""How the MoE kernels deal the 128-row chunks of K to the waves of a block, restated in plain Python (a helper, not a test; used by
tests/test_moe_wave_model_cpu.py), and float32 models of the two few-token gate_up kernels' summation order built on that deal.

The five loops (gptqmodel_amd/csrc):
  gptqhip_moe.hip          wave_partial: wave w of W takes chunks w, w + W, .. and issues the loads of kMoeAhead of them per round; gate_up runs
                           W = min(kMoeGateUpWaves, chunks) waves, down wps = min(kMoeDownWaves / top_k, chunks) waves for each of the top_k slots
  gptqhip_moe_fp8.hip      fp8_wave_partial: wave w of W takes the contiguous range [w chunks / W, (w + 1) chunks / W), kMoeAhead per round; with
                           K-block scales the accumulator is flushed where a K block ends and where the wave's share of one ends
  gptqhip_moe_grouped.hip  moe_grouped_kernel: wave w of W = min(kGroupedGateUpWaves | kGroupedDownWaves, chunks) takes w, w + W, ..,
                           kGroupedAhead per round; moe_combine_kernel: 256 threads of 4 columns, grid.y = ceil(H / 4 / 256)
The constants are READ from the kernel sources by name, so a changed constant changes what this model says the test shapes reach."""
import os
import re
from collections import namedtuple

import numpy as np

from conftest import ROOT

CSRC = os.path.join(ROOT, "gptqmodel_amd", "csrc")
CHUNK_K = 128            # rows of K per chunk (gptqhip_device.h: kChunkK)
COMBINE_THREADS = 256    # moe_combine_kernel: __launch_bounds__(256), `blockIdx.y * 256`
COMBINE_VEC = 4          # columns per thread


def kernel_constant(filename: str, name: str) -> int:
    """`constexpr int <name> = <value>;` of a kernel source."""
    text = open(os.path.join(CSRC, filename)).read()
    m = re.search(r"constexpr\s+int\s+" + name + r"\s*=\s*(\d+)\s*;", text)
    assert m, f"{name} not found in {filename}"
    return int(m.group(1))


kMoeGateUpWaves = kernel_constant("gptqhip_moe_common.h", "kMoeGateUpWaves")
kMoeDownWaves = kernel_constant("gptqhip_moe_common.h", "kMoeDownWaves")
kMoeAhead = kernel_constant("gptqhip_moe_common.h", "kMoeAhead")
kGroupedGateUpWaves = kernel_constant("gptqhip_moe_grouped.hip", "kGroupedGateUpWaves")
kGroupedDownWaves = kernel_constant("gptqhip_moe_grouped.hip", "kGroupedDownWaves")
kGroupedAhead = kernel_constant("gptqhip_moe_grouped.hip", "kGroupedAhead")

# one wave's work: the chunks it consumes, in order; rounds = the chunks consumed per trip of its `for (base ..)` loop (`ahead` loads are issued in
# every trip: a round shorter than that is ragged, its surplus loads repeat an in-range chunk that a wave-uniform `if` skips);
# flushes (FP8 with K-block scales) = [(chunk after which acc is flushed, "block" | "share")]
Wave = namedtuple("Wave", "chunks rounds flushes")


def _rounds(chunks, ahead):
    return [chunks[i:i + ahead] for i in range(0, len(chunks), ahead)]


def strided_deal(chunks: int, W: int, ahead: int):
    """wave_partial / moe_grouped_kernel: for (base = w; base < chunks; base += W * ahead) for (u < ahead) if (base + u * W < chunks)."""
    out = []
    for w in range(W):
        mine, rounds = [], []
        for base in range(w, chunks, W * ahead):
            r = [base + u * W for u in range(ahead) if base + u * W < chunks]
            rounds.append(r)
            mine += r
        assert mine == list(range(w, chunks, W)) and rounds == _rounds(mine, ahead)
        out.append(Wave(mine, rounds, []))
    return out


def contiguous_deal(chunks: int, W: int, ahead: int, cpb=None):
    """fp8_wave_partial: c0 = w chunks / W, c1 = (w + 1) chunks / W; for (base = c0; base < c1; base += ahead); cpb: chunks per K block."""
    out = []
    for w in range(W):
        c0, c1 = w * chunks // W, (w + 1) * chunks // W
        mine = list(range(c0, c1))
        flushes = []
        if cpb is not None:
            for ck in mine:
                if (ck + 1) % cpb == 0:
                    flushes.append((ck, "block"))
                elif ck + 1 == c1:
                    flushes.append((ck, "share"))
        out.append(Wave(mine, _rounds(mine, ahead), flushes))
    return out


def few_gate_up_waves(H: int) -> int:
    return min(kMoeGateUpWaves, H // CHUNK_K)


def few_down_wps(I: int, top_k: int) -> int:
    return min(kMoeDownWaves // top_k, I // CHUNK_K)


def int4_gate_up(H):
    return strided_deal(H // CHUNK_K, few_gate_up_waves(H), kMoeAhead)


def int4_down(I, top_k):
    """The waves of ONE slot (the block has top_k times as many)."""
    return strided_deal(I // CHUNK_K, few_down_wps(I, top_k), kMoeAhead)


def fp8_gate_up(H, block=None):
    return contiguous_deal(H // CHUNK_K, few_gate_up_waves(H), kMoeAhead, block[1] // CHUNK_K if block else None)


def fp8_down(I, top_k, block=None):
    return contiguous_deal(I // CHUNK_K, few_down_wps(I, top_k), kMoeAhead, block[1] // CHUNK_K if block else None)


def grouped_gate_up(H):
    return strided_deal(H // CHUNK_K, min(kGroupedGateUpWaves, H // CHUNK_K), kGroupedAhead)


def grouped_down(I):
    return strided_deal(I // CHUNK_K, min(kGroupedDownWaves, I // CHUNK_K), kGroupedAhead)


def combine_grid(H: int):
    """(column blocks = grid.y, live threads of the last one)."""
    vecs = H // COMBINE_VEC
    blocks = (vecs + COMBINE_THREADS - 1) // COMBINE_THREADS
    return blocks, vecs - COMBINE_THREADS * (blocks - 1)


# ---- what a deal reaches --------------------------------------------------------------------------------------------------------------------
def most_chunks(deal) -> int:
    return max(len(w.chunks) for w in deal)


def runs_a_second_trip(deal) -> bool:
    return any(len(w.rounds) >= 2 for w in deal)


def has_ragged_last_round(deal, ahead: int) -> bool:
    """Some wave runs more than `ahead` chunks and its last round is shorter than `ahead`."""
    return any(len(w.chunks) > ahead and len(w.rounds[-1]) < ahead for w in deal)


def has_ragged_round(deal, ahead: int) -> bool:
    return any(len(r) < ahead for w in deal for r in w.rounds)


def most_groups(deal, cpg: int) -> int:
    """The most group-constant rows (ck / cpg) one wave reads."""
    return max(len({ck // cpg for ck in w.chunks}) for w in deal)


def share_end_flushes(deal):
    """Flushes at the end of a wave's share of a K block that is not the block's end."""
    return [(i, ck) for i, w in enumerate(deal) for ck, kind in w.flushes if kind == "share"]


def blocks_cut_by_a_wave_boundary(deal, cpb: int):
    """K blocks whose chunks lie in more than one wave."""
    owner = {}
    for i, w in enumerate(deal):
        for ck in w.chunks:
            owner.setdefault(ck // cpb, set()).add(i)
    return sorted(b for b, ws in owner.items() if len(ws) > 1)


# ---- float32 models of the gate_up kernels' summation order ----------------------------------------------------------------------------------
f32 = np.float32


def _lane_sum(s):
    return (s[0] + s[1]) + (s[2] + s[3])        # moe_lane_sum


def int4_gate_up_sums(x, w):
    """moe_gate_up_kernel's fp32 sums of one projection.  x [K] and w [K, N]: float32 values representable in the activation dtype (w: the
    reference's rounded weights, which dequant_word4 reproduces).  One fp32 accumulator per K-step (32 rows) of a chunk, carried across the
    wave's chunks; the four are added as (0 + 1) + (2 + 3); the waves' sums are added in wave order."""
    K, N = w.shape
    x = x.astype(f32)
    v = np.zeros(N, f32)
    for wave in int4_gate_up(K):
        acc = np.zeros((4, N), f32)
        for ck in wave.chunks:
            for j in range(4):
                sl = slice(CHUNK_K * ck + 32 * j, CHUNK_K * ck + 32 * j + 32)
                acc[j] = acc[j] + (x[sl] @ w[sl]).astype(f32)
        v = v + _lane_sum(acc)
    return v


def fp8_gate_up_sums(x, codes_f32, rscale, block):
    """moe_fp8_gate_up_kernel's fp32 sums of one projection.  x [K]; codes_f32 [N, K]: the e4m3 values; rscale: fp32 reciprocal scales [N] (row)
    or [N, K / bc] per weight row (block = (br, bc)).  Block scales: acc * rscale is added to tot at every flush and acc restarts; row scales
    multiply the reduced sum once."""
    N, K = codes_f32.shape
    x = x.astype(f32)
    v = np.zeros(N, f32)
    cpb = block[1] // CHUNK_K if block else None
    for wave in fp8_gate_up(K, block):
        acc, tot = np.zeros((4, N), f32), np.zeros((4, N), f32)
        flush_at = {ck for ck, _ in wave.flushes}
        for ck in wave.chunks:
            for j in range(4):
                sl = slice(CHUNK_K * ck + 32 * j, CHUNK_K * ck + 32 * j + 32)
                acc[j] = acc[j] + (codes_f32[:, sl] @ x[sl]).astype(f32)
            if ck in flush_at:
                tot = tot + acc * rscale[:, ck // cpb][None, :]
                acc = np.zeros((4, N), f32)
        v = v + _lane_sum(tot if block else acc)
    return v if block else v * rscale
