"""Expert-grouped MoE ops without a GPU: the numpy model of gptqhip_moe_align (tests/moe_grouped_model.py), the host-side size helper and shape
predicate, and argument validation (GPTQHIP_EINVAL before any device access)."""
import ctypes
import os

import numpy as np
import pytest

import moe_grouped_model as GM
import moe_oracle as MO

EINVAL = -22


@pytest.fixture(scope="module")
def lib():
    from gptqmodel_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def check_invariants(ids, E):
    flat = ids.reshape(-1)
    S = flat.size
    ss, ue, nu, status = GM.align(ids, E)
    mu = GM.max_units(S, E)
    assert ss.shape == (16 * mu,) and ue.shape == (mu,) and 0 <= nu <= mu
    assert (ss[16 * nu:] == -1).all() and (ue[nu:] == -1).all()
    valid = (flat >= 0) & (flat < E)
    assert status == int(not valid.all())
    placed = ss[ss >= 0]
    assert sorted(placed.tolist()) == np.nonzero(valid)[0].tolist()           # every valid slot exactly once, no other
    assert (np.diff(ue[:nu]) >= 0).all()                                       # experts ascending
    for u in range(nu):
        rows = ss[16 * u:16 * u + 16]
        real = rows[rows >= 0]
        assert real.size >= 1 and rows[0] >= 0 and (rows[:real.size] >= 0).all()      # padding only at the end of a unit; row 0 is real
        assert (flat[real] == ue[u]).all() and (np.diff(real) > 0).all()      # one expert per unit, slots ascending
        if real.size < 16:
            assert u + 1 == nu or ue[u + 1] != ue[u]                           # only an expert's last unit is partial
    for e in set(ue[:nu].tolist()):
        mine = ss[np.repeat(ue == e, 16)]
        assert (np.diff(mine[mine >= 0]) > 0).all()                            # ascending across the units of an expert: stable
    return ss, ue, nu, status


def test_model_invariants_on_the_routing_cases():
    for E, k in ((8, 2), (5, 3), (4, 4), (128, 8)):
        for name, ids in GM.routing_cases(E, k).items():
            ss, ue, nu, status = check_invariants(ids, E)
            assert status == (1 if name == "out_of_range" else 0), name
    # all 40 slots on one expert: three units, the last one partial
    ss, ue, nu, _ = GM.align(np.full((40, 1), 3, np.int32), 8)
    assert nu == 3 and ue.tolist()[:3] == [3, 3, 3] and ss[:40].tolist() == list(range(40)) and (ss[40:48] == -1).all()
    # exactly 16 / 17 per expert: one full unit / one full and one single-row unit each
    for per, units in ((16, 1), (17, 2)):
        ss, ue, nu, _ = GM.align(GM.routing_cases(8, 2)[f"every_expert_{per}"], 8)
        assert nu == 8 * units and ue[:nu].tolist() == sorted(list(range(8)) * units)
    # E > S, and a dropped id takes no unit
    ss, ue, nu, st = GM.align(np.array([[200, 3], [-1, 200]], np.int32), 256)
    assert nu == 2 and ue[:2].tolist() == [3, 200] and ss[:2].tolist() == [1, -1] and ss[16:19].tolist() == [0, 3, -1] and st == 1


def test_units_helper_matches_the_model_and_covers_the_worst_cases(lib):
    for S in (1, 2, 15, 16, 17, 31, 32, 40, 255, 256, 257, 1000, 16384, 65536):
        for E in (1, 2, 5, 8, 60, 128, 256, 512):
            mu = lib.gptqhip_moe_grouped_units(S, E)
            assert mu == GM.max_units(S, E), (S, E)
            # every slot on its own expert (as far as E goes, the rest spread evenly), all slots on one expert
            spread = np.arange(S) % E
            assert GM.align(spread.reshape(-1, 1), E)[2] <= mu
            assert GM.align(np.zeros((S, 1), np.int32), E)[2] == -(-S // 16) <= mu
            # the worst case: one slot on each of min(S, E) - 1 experts, the rest on one -- the bound is met
            ne = min(S, E)
            worst = np.concatenate([np.arange(ne - 1), np.full(S - (ne - 1), ne - 1)])
            got = GM.align(worst.reshape(-1, 1), E)[2]
            assert got == mu, (S, E, got, mu)
    assert lib.gptqhip_moe_grouped_units(3, 256) == 3 and GM.align(np.array([[7, 99, 255]], np.int32), 256)[2] == 3        # E > S
    assert lib.gptqhip_moe_grouped_units(0, 8) == 0 and lib.gptqhip_moe_grouped_units(8, 0) == 0 and lib.gptqhip_moe_grouped_units(-1, 8) == 0


def test_shape_predicate(lib):
    from gptqmodel_amd import ops
    for name, (H, I, E, k, gs) in MO._ALL_SHAPES.items():
        for T in (1, 5, 16, 17, 33, 70, 2048):
            assert ops.moe_grouped_supported(H, I, gs, 4, False, T, k, E) == (name != MO.GS64_SHAPE), (name, T)
        assert not ops.moe_grouped_supported(H, I, gs, 4, True, 17, k, E)            # act-order
        assert not ops.moe_grouped_supported(H, I, gs, 8, False, 17, k, E)           # 8-bit codes
        assert not ops.moe_grouped_supported(H, I, gs, 4, False, 0, k, E)
    # the model shapes, and the stated limits: E <= 512, S <= 65536, top_k <= 16
    assert ops.moe_grouped_supported(2048, 768, 128, 4, False, 2048, 8, 128) and ops.moe_grouped_supported(4096, 14336, 128, 4, False, 8192, 2, 8)
    assert ops.moe_grouped_supported(2048, 768, 128, 4, False, 64, 8, 256) and ops.moe_grouped_supported(2048, 768, 128, 4, False, 64, 8, 512)
    assert not ops.moe_grouped_supported(2048, 768, 128, 4, False, 64, 8, 513)
    assert ops.moe_grouped_supported(2048, 768, 128, 4, False, 8192, 8, 128) and not ops.moe_grouped_supported(2048, 768, 128, 4, False, 8193, 8, 128)
    assert not ops.moe_grouped_supported(2048, 768, 128, 4, False, 4, 17, 128) and not ops.moe_grouped_supported(2000, 768, 128, 4, False, 4, 8, 128)


def test_argument_validation_without_a_device(lib):
    one, odd2, odd8 = ctypes.c_void_p(256), ctypes.c_void_p(258), ctypes.c_void_p(264)
    err = lib.gptqhip_last_error
    # align
    assert lib.gptqhip_moe_align(None, one, one, one, one, 4, 2, 8, None) == EINVAL and b"null" in err()
    assert lib.gptqhip_moe_align(one, one, one, None, one, 4, 2, 8, None) == EINVAL and b"null" in err()
    assert lib.gptqhip_moe_align(one, odd2, one, one, one, 4, 2, 8, None) == EINVAL and b"aligned" in err()
    for T, k, E in ((0, 2, 8), (4, 0, 8), (4, 17, 8), (4, 2, 0), (4, 2, 513), (65536, 2, 8)):
        assert lib.gptqhip_moe_align(one, one, one, one, one, T, k, E, None) == EINVAL and b"top_k" in err(), (T, k, E)
    # the two grouped stages
    for fn in (lib.gptqhip_moe_gate_up_grouped, lib.gptqhip_moe_down_grouped):
        def call(x=one, qw=one, meta=one, ss=one, ue=one, nu=one, out=one, T=20, k=2, E=8, H=256, I=128, gs=128, bits=4, adt=0, sdt=0):
            return fn(x, qw, meta, ss, ue, nu, out, T, k, E, H, I, gs, bits, adt, sdt, None)
        assert call(x=None) == EINVAL and b"null" in err()
        assert call(nu=None) == EINVAL and b"null" in err()
        assert call(out=odd8) == EINVAL and b"16-byte" in err()
        assert call(qw=odd8) == EINVAL and b"16-byte" in err()
        assert call(ss=odd2) == EINVAL and b"4-byte" in err()
        assert call(T=0) == EINVAL and call(k=17) == EINVAL and call(E=513) == EINVAL and call(T=40000) == EINVAL
        assert call(gs=64) == EINVAL and b"group_size" in err()
        assert call(bits=8) == EINVAL and call(H=200) == EINVAL and call(I=100) == EINVAL
        assert call(adt=1, sdt=0) == EINVAL and b"dtypes" in err()
        assert call(adt=2) == EINVAL
    # combine
    def comb(part=one, ids=one, w=one, out=one, st=one, T=20, k=2, E=8, H=256, adt=0):
        return lib.gptqhip_moe_combine(part, ids, w, out, st, T, k, E, H, adt, None)
    assert comb(part=None) == EINVAL and b"null" in err()
    assert comb(st=None) == EINVAL and b"null" in err()
    assert comb(out=odd8) == EINVAL and b"16-byte" in err()
    assert comb(w=odd2) == EINVAL and b"4-byte" in err()
    assert comb(T=0) == EINVAL and comb(E=0) == EINVAL and comb(H=100) == EINVAL and comb(adt=3) == EINVAL


def test_abi_version_and_bindings():
    from gptqmodel_amd import _lib
    assert _lib.ABI_VERSION == 21
    for name in ("gptqhip_moe_grouped_supported", "gptqhip_moe_grouped_units", "gptqhip_moe_align", "gptqhip_moe_gate_up_grouped",
                 "gptqhip_moe_down_grouped", "gptqhip_moe_combine"):
        assert name in _lib.SIGNATURES


def test_module_defaults_leave_the_grouped_path_off(monkeypatch):
    import torch
    from gptqmodel_amd.nn_modules.moe import HipMoeExperts
    monkeypatch.delenv("GPTQHIP_MOE_GROUPED", raising=False)
    m = HipMoeExperts(8, 256, 128, 128, 128, torch.float16)
    assert m.grouped_routing is False and isinstance(m.grouped_min_tokens, int) and isinstance(m.grouped_max_tokens, int)
    assert m.grouped_path(17, 2, torch.float16) and m.grouped_path(1, 2, torch.float16) and not m.grouped_path(17, 2, torch.float32)
    monkeypatch.setenv("GPTQHIP_MOE_GROUPED", "1")
    assert HipMoeExperts(8, 256, 128, 128, 128, torch.float16).grouped_routing is True
    assert not HipMoeExperts(4, 256, 128, 64, 64, torch.float16).grouped_path(17, 2, torch.float16)
