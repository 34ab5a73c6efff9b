"""Expert-grouped FP8 MoE ops without a GPU: the C ABI's three entries (bindings, the host predicate, GPTQHIP_EINVAL before any device access),
HipFp8MoeExperts' grouped_path against the predicate, what the two experts modules inherit from StackedMoeExperts, the float32 model of the
stage-two contract against its bar on every case of tests/test_gpu_moe_fp8_grouped.py, and what the deep shapes reach in the chunk deal of
moe_fp8_grouped_kernel (tests/moe_wave_model.py: contiguous_deal, with the constants READ from gptqhip_moe_fp8_grouped.hip).  Nothing here
launches a kernel."""
import ctypes
import os
import re

import pytest
import torch

import fp8_oracle as F
import moe_fp8_oracle as MF
import moe_wave_model as WM
from gptqmodel_amd import _lib, ops
from gptqmodel_amd.nn_modules import moe, moe_fp8
from gptqmodel_amd.nn_modules.moe_base import StackedMoeExperts

EINVAL = -22
TENSOR, ROW, BLOCK = ops.FP8_SCALE_TENSOR, ops.FP8_SCALE_ROW, ops.FP8_SCALE_BLOCK
_i, _vp = ctypes.c_int, ctypes.c_void_p
NEW_SYMBOLS = {"gptqhip_moe_fp8_grouped_supported": (_i, [_i] * 10),
               "gptqhip_moe_fp8_gate_up_grouped": (_i, [_vp] * 7 + [_i] * 7 + [_vp]),
               "gptqhip_moe_fp8_down_grouped": (_i, [_vp] * 7 + [_i] * 9 + [_vp])}
# the cases of tests/test_gpu_moe_fp8_grouped.py
TOKENS = (1, 5, 16, 17, 33, 70)
DEEP_CASES = [("4224x128e3k2", "row"), ("4224x128e3k2", "b128x128"), ("4224x128e3k2", "gu64x384_d32x128"),
              ("128x4224e3k2", "tensor"), ("128x4224e3k2", "b128x128"), ("128x4224e3k2", "gu128x128_d32x384")]
DEEP_TOKENS = (5, 33)
ACTS = ("fp16", "bf16")
SRC = "gptqhip_moe_fp8_grouped.hip"


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


# ---- C ABI -------------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_bound(lib):
    from conftest import ROOT
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gptqhip.h")).read(), flags=re.S)
    for s, sig in NEW_SYMBOLS.items():
        assert re.search(r"\b" + s + r"\s*\(", text) and hasattr(lib, s), s
        assert _lib.SIGNATURES[s] == sig, s
    assert lib.gptqhip_abi_version() == 21 and _lib.ABI_VERSION == 21
    assert callable(ops.moe_fp8_grouped_supported) and callable(ops.moe_fp8_gate_up_grouped) and callable(ops.moe_fp8_down_grouped)


def test_supported_predicate_table(lib):
    sup = lib.gptqhip_moe_fp8_grouped_supported
    #      H     I      gu_bc mode   br   bc   T     k  E
    qwen = (2048, 768, 128, BLOCK, 128, 128, 2048, 8, 128)
    mixtral = (4096, 14336, 0, ROW, 0, 0, 8192, 2, 8)
    for act in (0, 1):
        assert sup(*qwen, act) == 1 and sup(*mixtral, act) == 1
    assert sup(2048, 768, 128, BLOCK, 128, 128, 2048, 8, 512, 0) == 1 and sup(2048, 768, 128, BLOCK, 128, 128, 2048, 8, 513, 0) == 0      # E
    assert sup(2048, 768, 128, BLOCK, 128, 128, 65536, 1, 128, 0) == 1 and sup(2048, 768, 128, BLOCK, 128, 128, 65537, 1, 128, 0) == 0   # T * k
    assert sup(2048, 768, 128, BLOCK, 128, 128, 4096, 16, 128, 0) == 1 and sup(2048, 768, 128, BLOCK, 128, 128, 4, 17, 128, 0) == 0      # top_k
    assert sup(2000, 768, 0, ROW, 0, 0, 64, 8, 128, 0) == 0                                                                               # H = 2000
    assert sup(2048, 768, 64, BLOCK, 128, 128, 64, 8, 128, 0) == 0 and sup(2048, 768, 128, BLOCK, 128, 64, 64, 8, 128, 0) == 0            # bc = 64
    assert sup(*qwen, 2) == 0 and sup(*qwen, -1) == 0                                                                                     # fp32
    for T, k, E in ((0, 8, 128), (64, 0, 128), (64, 8, 0)):
        assert sup(2048, 768, 128, BLOCK, 128, 128, T, k, E, 0) == 0
    # every scale rule of the few-token predicate, at a T it refuses
    for H, I, gbc, mode, br, bc in ((256, 128, 0, TENSOR, 0, 0), (1280, 128, 256, BLOCK, 32, 128), (384, 640, 384, BLOCK, 3, 640)):
        assert sup(H, I, gbc, mode, br, bc, 70, 3, 5, 0) == 1 and lib.gptqhip_moe_fp8_supported(H, I, gbc, mode, br, bc, 16, 3, 0) == 1
    for H, I, gbc, mode, br, bc in ((256, 192, 0, ROW, 0, 0), (384, 128, 256, ROW, 0, 0), (256, 384, 0, BLOCK, 128, 256), (256, 128, 0, BLOCK, 96, 128),
                                    (256, 128, 0, 3, 0, 0)):
        assert sup(H, I, gbc, mode, br, bc, 70, 3, 5, 0) == 0 and lib.gptqhip_moe_fp8_supported(H, I, gbc, mode, br, bc, 16, 3, 0) == 0
    # the ops-level wrappers
    assert ops.moe_fp8_grouped_supported(2048, 768, 128, BLOCK, (128, 128), 2048, 8, 128, torch.bfloat16)
    assert ops.moe_fp8_grouped_supported(4096, 14336, 0, ROW, None, 8192, 2, 8)
    assert not ops.moe_fp8_grouped_supported(2048, 768, 128, BLOCK, (128, 128), 64, 8, 513)
    assert not ops.moe_fp8_grouped_supported(2048, 768, 128, BLOCK, (128, 128), 65537, 1, 128)
    assert not ops.moe_fp8_grouped_supported(2048, 768, 128, BLOCK, (128, 128), 64, 8, 128, torch.float32)
    # the few-token predicate keeps its limit
    assert not ops.moe_fp8_supported(2048, 768, 128, BLOCK, (128, 128), 17, 8) and ops.moe_fp8_supported(2048, 768, 128, BLOCK, (128, 128), 16, 8)


def test_every_entry_validates_before_touching_a_device(lib):
    one, odd16, odd4 = ctypes.c_void_p(256), ctypes.c_void_p(264), ctypes.c_void_p(258)
    err = lib.gptqhip_last_error
    gu, dn = lib.gptqhip_moe_fp8_gate_up_grouped, lib.gptqhip_moe_fp8_down_grouped

    def gate_up(x=one, w=one, rs=one, ss=one, ue=one, nu=one, act=one, T=20, k=2, E=8, H=256, I=128, bc=0, dt=0):
        return gu(x, w, rs, ss, ue, nu, act, T, k, E, H, I, bc, dt, None)

    def down(a=one, w=one, rs=one, ss=one, ue=one, nu=one, part=one, T=20, k=2, E=8, H=256, I=128, mode=ROW, br=0, bc=0, dt=0):
        return dn(a, w, rs, ss, ue, nu, part, T, k, E, H, I, mode, br, bc, dt, None)

    for fn, big in ((gate_up, ("x", "w", "act")), (down, ("a", "w", "part"))):
        for name in big + ("rs", "ss", "ue", "nu"):
            assert fn(**{name: None}) == EINVAL and b"null" in err(), name
        for name in big:
            assert fn(**{name: odd16}) == EINVAL and b"16-byte aligned" in err(), name
        for name in ("rs", "ss", "ue", "nu"):
            assert fn(**{name: odd4}) == EINVAL and b"4-byte aligned" in err(), name
        for kw in (dict(T=0), dict(k=0), dict(k=17), dict(E=0), dict(E=513), dict(T=40000), dict(T=65536, k=2)):      # routing limits
            assert fn(**kw) == EINVAL and b"top_k" in err(), kw
        for kw in (dict(H=200), dict(I=192), dict(H=0), dict(I=-128)):
            assert fn(**kw) == EINVAL and b"multiples of 128" in err(), kw
        for dt in (2, -1):
            assert fn(dt=dt) == EINVAL and b"dtype" in err()
    for kw in (dict(bc=64), dict(bc=192), dict(H=384, bc=256), dict(bc=-128)):
        assert gate_up(**kw) == EINVAL and b"block columns" in err() and b"gptqhip_moe_fp8_gate_up_grouped" in err(), kw
    assert down(mode=3) == EINVAL and b"scale layout" in err() and b"gptqhip_moe_fp8_down_grouped" in err()
    for kw in (dict(mode=BLOCK, br=128, bc=64), dict(mode=BLOCK, br=128, bc=256), dict(mode=BLOCK, br=128, bc=0)):
        assert down(**kw) == EINVAL and b"block columns" in err(), kw
    for kw in (dict(mode=BLOCK, br=96, bc=128), dict(mode=BLOCK, br=0, bc=128)):
        assert down(**kw) == EINVAL and b"block rows" in err(), kw


def test_ops_refuse_cpu_tensors(lib):
    H, I, E, T, k = 256, 128, 2, 20, 2
    units = ops.moe_grouped_units(T * k, E)
    x, act = torch.zeros((T, H), dtype=torch.float16), torch.zeros((T * k, I), dtype=torch.float16)
    ss, ue, nu = (torch.zeros(n, dtype=torch.int32) for n in (16 * units, units, 1))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.moe_fp8_gate_up_grouped(x, torch.zeros((E, 2 * I * H), dtype=torch.uint8), torch.ones((E, 2 * I)), ss, ue, nu, act, k, E, I)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.moe_fp8_down_grouped(act, torch.zeros((E, I * H), dtype=torch.uint8), torch.ones((E, H)), ss, ue, nu, torch.zeros((T * k, H)), k, E, H, ROW)


# ---- module ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gu,down", [(("block", (128, 128)), ("block", (128, 128))), (("row", None), ("tensor", None)),
                                     (("block", (64, 256)), ("block", (32, 128)))], ids=["b128x128", "row-tensor", "gu64x256_d32x128"])
def test_grouped_path_is_the_c_predicate(lib, gu, down):
    E, H, I = 8, 1280, 128
    m = moe_fp8.HipFp8MoeExperts(E, H, I, gu[0], gu[1], down[0], down[1])
    gbc = gu[1][1] if gu[0] == "block" else 0
    mode = ops.FP8_SCALE_MODES[down[0]]
    br, bc = down[1] if down[1] else (0, 0)
    for T, k in ((1, 1), (5, 3), (16, 16), (17, 2), (1, 17), (70, 8), (4097, 16)):
        for dtype, tag in ((torch.float16, 0), (torch.bfloat16, 1), (torch.float32, 2)):
            want = bool(lib.gptqhip_moe_fp8_grouped_supported(H, I, gbc, mode, br, bc, T, k, E, tag))
            assert m.grouped_path(T, k, dtype) is want, (T, k, dtype)
    # the table is not vacuous
    assert m.grouped_path(17, 2, torch.float16) and m.grouped_path(70, 8, torch.bfloat16) and m.grouped_path(1, 1, torch.float16)
    assert not m.grouped_path(1, 17, torch.float16) and not m.grouped_path(4097, 16, torch.float16) and not m.grouped_path(17, 2, torch.float32)
    assert not m.fast_path(17, 2, torch.float16)
    assert not moe_fp8.HipFp8MoeExperts(513, H, I, gu[0], gu[1], down[0], down[1]).grouped_path(17, 2, torch.float16)


def test_module_defaults_leave_the_grouped_path_off(monkeypatch):
    monkeypatch.delenv("GPTQHIP_MOE_GROUPED", raising=False)
    m = moe_fp8.HipFp8MoeExperts(8, 256, 128, "row", None, "row", None)
    assert m.grouped_routing is False
    assert (m.grouped_min_tokens, m.grouped_max_tokens) == (moe_fp8.GROUPED_MIN_TOKENS, moe_fp8.GROUPED_MAX_TOKENS)
    assert 1 <= m.grouped_min_tokens <= m.grouped_max_tokens <= 65536 and m._grouped_eager == {} and m._grouped_captured == {}
    monkeypatch.setenv("GPTQHIP_MOE_GROUPED", "1")
    assert moe_fp8.HipFp8MoeExperts(8, 256, 128, "row", None, "row", None).grouped_routing is True
    # the int4 module keeps its attributes and constants
    monkeypatch.delenv("GPTQHIP_MOE_GROUPED", raising=False)
    q = moe.HipMoeExperts(8, 256, 128, 128, 128, torch.float16)
    assert q.grouped_routing is False and (q.grouped_min_tokens, q.grouped_max_tokens) == (moe.GROUPED_MIN_TOKENS, moe.GROUPED_MAX_TOKENS)
    assert q._grouped_eager == {} and q._grouped_captured == {}


@pytest.mark.parametrize("cls", [moe.HipMoeExperts, moe_fp8.HipFp8MoeExperts], ids=["int4", "fp8"])
def test_grouped_scaffolding_is_inherited_and_the_stages_are_the_subclass(cls):
    for name in ("_grouped_alloc", "_grouped_scratch", "_forward_grouped", "_forward_routed", "forward", "_forward_loop", "_scratch_for",
                 "_device_routing"):
        assert name not in vars(cls) and name in vars(StackedMoeExperts), name
    for name in ("grouped_path", "_grouped_gate_up", "_grouped_down", "fast_path", "_fused_gate_up", "_fused_down"):
        assert name in vars(cls), name


def test_fuse_moe_experts_passes_the_flag_to_the_fp8_stand_in(monkeypatch):
    """The stacking itself needs a device; with from_linears stubbed, what fuse_moe_experts does with `grouped_routing` is host logic."""
    import torch.nn as nn
    from gptqmodel_amd.utils.moe import auto_fuse_moe, fuse_moe_experts
    monkeypatch.delenv("GPTQHIP_MOE_GROUPED", raising=False)
    monkeypatch.setattr(moe_fp8.HipFp8MoeExperts, "from_linears",
                        classmethod(lambda cls, g, u, d: cls(len(g), 256, 128, "row", None, "row", None)))

    class Proj(nn.Module):
        QUANT_TYPE = "hip_fp8"

    class Expert(nn.Module):
        def __init__(self):
            super().__init__()
            self.gate_proj, self.up_proj, self.down_proj, self.act_fn = Proj(), Proj(), Proj(), nn.SiLU()

    class Experts(nn.ModuleList):
        def forward(self, hidden_states, top_k_index, top_k_weights):
            raise AssertionError("not called here")

    class Block(nn.Module):
        def __init__(self):
            super().__init__()
            self.experts = Experts([Expert(), Expert()])

    for flag, want in ((True, True), (False, False), (None, False)):
        blk = Block()
        assert fuse_moe_experts(blk, grouped_routing=flag) is True and isinstance(blk.experts, moe_fp8.HipFp8MoeExperts)
        assert blk.experts.grouped_routing is want, flag
    model = nn.Sequential(Block(), Block())
    assert auto_fuse_moe(model, grouped_routing=True) == 2 and all(b.experts.grouped_routing is True for b in model)


# ---- the stage-two bar is reachable on every GPU case ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("shape,layout", MF.CASES + DEEP_CASES)
def test_the_model_of_the_contract_fits_its_own_bars(shape, layout, act):
    """act_model -> down with the kernels' fp32 weights, fp32 accumulation chunk by chunk in BOTH chunk orders, one fp32 weighted sum in slot
    order, one rounding: inside the stage-two bar on every case of tests/test_gpu_moe_fp8_grouped.py (so the bar leaves room for the grouped
    kernel's summation order)."""
    worst = 0.0
    for T in (DEEP_TOKENS if (shape, layout) in DEEP_CASES else TOKENS):
        c = MF.case(shape, layout, T, act)
        b = MF.bar(c)
        for reverse in (True, False):
            e = F.rel64(MF.model_down_f32(shape, layout, c, act, reverse=reverse), c["y64"])
            worst = max(worst, e / b)
            assert e <= b, (T, reverse, e, b)
    print(f"{shape} {layout} {act}: model at {worst:.2f} of its bar")


def test_routing_of_seventy_tokens_fills_partial_full_and_several_units():
    import numpy as np
    c = MF.case("256x128e8k2", "row", 70, "fp16")
    counts = np.bincount(c["ids"].reshape(-1), minlength=8)
    assert counts.sum() == 140 and counts.min() >= 1 and counts.max() > 16       # several units per expert, and partial last ones
    assert any(n % 16 for n in counts)
    one = MF.case("256x128e8k2", "row", 1, "fp16")["ids"]
    assert np.bincount(one.reshape(-1), minlength=8).tolist().count(0) == 6      # empty experts take no unit


# ---- what the deep shapes reach in moe_fp8_grouped_kernel's chunk deal -----------------------------------------------------------------------
kGateUpWaves = WM.kernel_constant(SRC, "kFp8GroupedGateUpWaves")
kDownWaves = WM.kernel_constant(SRC, "kFp8GroupedDownWaves")
kAhead = WM.kernel_constant(SRC, "kFp8GroupedAhead")


def gate_up_deal(H, block=None):
    chunks = H // WM.CHUNK_K
    return WM.contiguous_deal(chunks, min(kGateUpWaves, chunks), kAhead, block[1] // WM.CHUNK_K if block else None)


def down_deal(I, block=None):
    chunks = I // WM.CHUNK_K
    return WM.contiguous_deal(chunks, min(kDownWaves, chunks), kAhead, block[1] // WM.CHUNK_K if block else None)


def lens(deal):
    return [len(w.chunks) for w in deal]


def test_constants_are_the_kernels():
    assert (kGateUpWaves, kDownWaves, kAhead) == (8, 16, 2)
    # the shallow shapes: at most two chunks per wave, so no wave runs a second round of loads
    for H, I, E, k in MF.SHAPES.values():
        assert WM.most_chunks(gate_up_deal(H)) <= kAhead and WM.most_chunks(down_deal(I)) <= kAhead
    assert lens(gate_up_deal(1280)) == [1, 1, 1, 2, 1, 1, 1, 2]                  # ten chunks over eight waves: uneven shares
    assert lens(down_deal(128)) == [1] and lens(down_deal(640)) == [1] * 5       # one chunk; an odd chunk count


def test_deep_gate_up_runs_ragged_rounds_and_cuts_k_blocks():
    H, I, E, k = MF.DEEP_SHAPES["4224x128e3k2"]
    g = gate_up_deal(H)
    assert lens(g) == [4, 4, 4, 4, 4, 4, 4, 5] and [len(r) for r in g[7].rounds] == [2, 2, 1]
    assert WM.has_ragged_last_round(g, kAhead) and WM.runs_a_second_trip(g)
    block = MF.proj_layout("gu64x384_d32x128", "gate")[1]
    gb = gate_up_deal(H, block)
    cpb = block[1] // WM.CHUNK_K
    # wave boundaries at chunks 4, 8, .., 28 against K blocks of 3 chunks: five of the seven cut a block (12 and 24 are block ends)
    assert cpb == 3 and len(WM.blocks_cut_by_a_wave_boundary(gb, cpb)) == 5
    assert [w for w, _ in WM.share_end_flushes(gb)] == [0, 1, 3, 4, 6]
    assert all(len(w.flushes) >= 2 for w in gb)                                  # tot accumulates over more than one flush
    b1 = gate_up_deal(H, (128, 128))
    assert all([ck for ck, _ in w.flushes] == w.chunks for w in b1) and not WM.share_end_flushes(b1)      # bc = 128: a flush after every chunk
    assert not g[0].flushes                                                      # row scales: the epilogue alone
    assert WM.combine_grid(H) == (5, 32)                                         # five column blocks of the combine, the last one partial
    assert lens(down_deal(I)) == [1]                                             # (the down side of this shape is the shallow one)


def test_deep_down_runs_sixteen_waves_with_a_ragged_last_round():
    H, I, E, k = MF.DEEP_SHAPES["128x4224e3k2"]
    d = down_deal(I)
    assert len(d) == 16 and lens(d) == [2] * 15 + [3] and [len(r) for r in d[15].rounds] == [2, 1]
    assert WM.has_ragged_last_round(d, kAhead)
    block = MF.proj_layout("gu128x128_d32x384", "down")[1]
    db = down_deal(I, block)
    cpb = block[1] // WM.CHUNK_K
    # wave boundaries at the even chunks 2 .. 30 against K blocks of 3 chunks: the ten that are no multiple of 3 cut a block
    assert cpb == 3 and len(WM.blocks_cut_by_a_wave_boundary(db, cpb)) == 10 and len(WM.share_end_flushes(db)) == 10
    assert max(len(w.flushes) for w in db) == 2 and lens(gate_up_deal(H)) == [1]


def test_the_deal_covers_every_chunk_exactly_once():
    for chunks in range(1, 40):
        for W in {min(kGateUpWaves, chunks), min(kDownWaves, chunks)}:
            for cpb in (None, 1, 2, 3):
                deal = WM.contiguous_deal(chunks, W, kAhead, cpb)
                assert sorted(ck for w in deal for ck in w.chunks) == list(range(chunks)) and all(w.chunks for w in deal)
                for w in deal:      # block scales: nothing is left in acc at the end of a wave
                    assert cpb is None or w.flushes[-1][0] == w.chunks[-1]
