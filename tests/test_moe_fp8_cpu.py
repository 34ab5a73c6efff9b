"""Fused FP8 MoE experts without a GPU: the oracle's self-checks, the model of the kernels' contract against its own bars on every GPU case,
the interleave rule, the C ABI's predicate and argument validation, and what fuse_moe_experts / from_linears decline.  Nothing here launches a
kernel."""
import ctypes
import zlib

import numpy as np
import pytest
import torch
import torch.nn as nn

import fp8_oracle as F
import moe_fp8_oracle as MF
import moe_oracle as MO
from gptqmodel_amd import _lib, ops
from gptqmodel_amd.nn_modules.moe_fp8 import HipFp8MoeExperts, _interleave_tiled, interleave_rows8
from gptqmodel_amd.nn_modules.qlinear.hip_fp8 import HipFp8Linear

EINVAL = -22
TENSOR, ROW, BLOCK = ops.FP8_SCALE_TENSOR, ops.FP8_SCALE_ROW, ops.FP8_SCALE_BLOCK
NEW_SYMBOLS = ("gptqhip_moe_fp8_supported", "gptqhip_moe_fp8_gate_up", "gptqhip_moe_fp8_down")
ACTS = ("fp16", "bf16")


@pytest.fixture(scope="module")
def lib():
    import os
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


@pytest.fixture
def kernels_available(monkeypatch):
    """Pretend the native library + a gfx950 device are usable (nothing here launches a kernel)."""
    monkeypatch.setattr(HipFp8Linear, "validate_once", classmethod(lambda c: (True, None)))
    HipFp8Linear.cached_validate_once.cache_clear()
    yield
    HipFp8Linear.cached_validate_once.cache_clear()


# ---- oracle ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", ACTS)
def test_oracle_reduces_to_the_linear_oracle_on_one_slot(act):
    """One token, one slot, routing weight 1: stage two is one FP8 linear on act_model, so y64 / y_once / chain are fp8_oracle's."""
    shape, layout = "256x128e8k2", "b128x128"
    H, I, E, _ = MF.SHAPES[shape]
    ex, w64 = MF.experts_of(shape, layout), MF.weights64_of(shape, layout)
    x = MO.make_x(3, 1, H, act).astype(np.float64)
    for e in (0, E - 1):
        ids, rw = np.array([[e]], np.int32), np.ones((1, 1), np.float32)
        r = MF.evaluate(ex, w64, layout, x, ids, rw, act)
        a = r["act_model"]
        assert np.array_equal(a, F.round_to(a, act)) and np.isfinite(a).all() and np.abs(a).max() > 0
        codes, scale_inv = ex[e]["down"]
        assert np.array_equal(r["y64"], F.y64(a, codes, scale_inv, None, (128, 128)))
        assert np.array_equal(r["y_once"], F.y_once(a, codes, scale_inv, None, act, (128, 128)))
        assert np.array_equal(r["chain"], F.chain(a, codes, scale_inv, None, act, (128, 128)))
        # stage one by hand on one neuron
        g = F.round_to(x[0] @ w64[e]["gate"][5], act)
        u = F.round_to(x[0] @ w64[e]["up"][5], act)
        assert a[0, 5] == F.round_to(F.round_to(g / (1.0 + np.exp(-g)), act) * u, act)


def test_oracle_routing_and_inputs():
    shape, layout, act = "384x640e5k3", "row", "fp16"
    H, I, E, k = MF.SHAPES[shape]
    c = MF.case(shape, layout, 5, act)
    assert c["ids"].shape == (5, k) and c["ids"].min() >= 0 and c["ids"].max() < E and c["act_model"].shape == (5 * k, I)
    assert np.allclose(c["rw"].sum(axis=1), 1.0, atol=2e-3)
    for ex in MF.experts_of(shape, layout):
        for name, (codes, scale_inv) in ex.items():
            assert codes.shape == MF.proj_dims(shape, name) and not np.isin(codes, (0x7f, 0xff)).any()
            assert scale_inv.min() >= 200.0 and scale_inv.max() <= 6.0e4
    # experts differ from each other, a token's result depends on its own slots only
    assert not np.array_equal(MF.experts_of(shape, layout)[0]["gate"][0], MF.experts_of(shape, layout)[1]["gate"][0])
    solo = MF.evaluate(MF.experts_of(shape, layout), MF.weights64_of(shape, layout), layout, c["x"][2:3], c["ids"][2:3], c["rw"][2:3], act)
    assert np.array_equal(solo["y64"][0], c["y64"][2]) and np.array_equal(solo["chain"][0], c["chain"][2])
    # the wide-block layout only fits the shape it was made for
    assert ("1280x128e3k2", "gu64x256_d32x128") in MF.CASES and len(MF.CASES) == 13


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("shape,layout", MF.CASES)
def test_the_model_of_the_contract_fits_its_own_bars(shape, layout, act):
    """On every GPU case: act_model -> down with the kernels' fp32 weights and float32 accumulation in REVERSED chunk order stays within the
    stage-two bar (so the bar leaves room for any fp32 summation order), outputs are finite and the chain term is a real number."""
    for T in MF.TOKENS:
        c = MF.case(shape, layout, T, act)
        assert all(np.isfinite(c[k]).all() for k in ("act_model", "y64", "y_once", "chain"))
        e = F.rel64(MF.model_down_f32(shape, layout, c, act), c["y64"])
        assert e <= MF.bar(c), (T, e, MF.bar(c))
        assert F.rel64(c["y_once"], c["y64"]) <= F.rel64(c["chain"], c["y64"]) + 1e-4      # one rounding is never the worse of the two


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("shape,layout", MF.DEEP_CASES)
def test_the_model_of_the_contract_fits_its_own_bars_on_the_deep_cases(shape, layout, act):
    """The conditions of test_the_model_of_the_contract_fits_its_own_bars on every case of test_deep_k_and_wide_top_k_against_the_oracle."""
    for T in MF.DEEP_TOKENS:
        c = MF.case(shape, layout, T, act)
        assert all(np.isfinite(c[k]).all() for k in ("act_model", "y64", "y_once", "chain"))
        e = F.rel64(MF.model_down_f32(shape, layout, c, act), c["y64"])
        print(f"{shape} {layout} T={T} {act}: model {e:.3e} (bar {MF.bar(c):.3e}: chain {F.rel64(c['chain'], c['y64']):.3e}, "
              f"one rounding {F.rel64(c['y_once'], c['y64']):.3e}) max|act_model|={float(np.abs(c['act_model']).max()):.3g}")
        assert e <= MF.bar(c), (T, e, MF.bar(c))
        assert F.rel64(c["y_once"], c["y64"]) <= F.rel64(c["chain"], c["y64"]) + 1e-4


def test_deep_cases_are_apart_from_the_existing_ones():
    assert len(MF.CASES) == 13 and len(MF.DEEP_CASES) == 12 and not set(MF.DEEP_CASES) & set(MF.CASES)
    assert {s for s, _ in MF.DEEP_CASES} == set(MF.DEEP_SHAPES) and set(MF.DEEP_LAYOUTS) <= {l for _, l in MF.DEEP_CASES}
    for shape, layout in MF.DEEP_CASES:      # every block divides its projection
        for name in MF.PROJ:
            (N, K), (method, block) = MF.proj_dims(shape, name), MF.proj_layout(layout, name)
            assert block is None or (N % block[0] == 0 and K % block[1] == 0), (shape, layout, name)
    old = {MF._seed0(s, l) for s, l in MF.CASES}
    new = {MF._seed0(s, l) for s, l in MF.DEEP_CASES}
    assert len(new) == 12 and min(new) > max(old) + 6 * 16


def crc(a) -> int:
    return zlib.crc32(np.ascontiguousarray(a).tobytes())


# (shape, layout, T, act) -> crc32 of x, ids, rw, expert 0's gate codes, the last expert's down scale_inv and chain, recorded on the commit before
# DEEP_SHAPES / DEEP_LAYOUTS existed: adding them must not move the seeds, and with them the inputs, of any case that was there before
PINNED_INPUTS = {
    ("1280x128e3k2", "gu64x256_d32x128", 5, "fp16"): (3169201390, 3732383910, 556380046, 4281994224, 3155888974, 325525882),
    ("256x256e8k8", "row", 16, "bf16"): (93289943, 3617835931, 979495653, 346879391, 1686543588, 3152011844),
    ("384x640e5k3", "b128x128", 2, "fp16"): (1750784163, 1499497953, 2054021073, 2023461098, 3013506786, 2373060410),
    ("256x128e8k2", "tensor", 1, "bf16"): (2579204185, 4091379325, 2815860233, 394158350, 1378013163, 3359235249),
}


@pytest.mark.parametrize("key", sorted(PINNED_INPUTS))
def test_inputs_of_the_existing_cases_keep_their_bits(key):
    shape, layout, T, act = key
    c, ex = MF.case(*key), MF.experts_of(shape, layout)
    assert c["x"].dtype == np.float64 and c["ids"].dtype == np.int32 and ex[0]["gate"][0].dtype == np.uint8
    got = (crc(c["x"]), crc(c["ids"]), crc(c["rw"]), crc(ex[0]["gate"][0]), crc(ex[-1]["down"][1]), crc(c["chain"]))
    assert got == PINNED_INPUTS[key], got


# ---- layout ------------------------------------------------------------------------------------------------------------------------------
def np_tiled(w: np.ndarray) -> np.ndarray:
    """uint8 [N, K] -> the FP8 kernel layout (gptqhip_fp8.hip), restated."""
    N, K = w.shape
    chunks = K // 128
    out = np.zeros(N * K, np.uint8)
    n, k = np.meshgrid(np.arange(N), np.arange(K), indexing="ij")
    kk = k & 127
    lane = (((kk & 31) >> 3) << 4) | (n & 15)
    off = ((((n >> 4) * chunks + (k >> 7)) * 2 + (kk >> 6)) * 64 + lane) * 16 + 8 * ((kk >> 5) & 1) + (kk & 7)
    out[off.reshape(-1)] = w.reshape(-1)
    return out


def test_interleave_rule_is_fuse_gate_up_interleaved_column_order():
    from gptqmodel_amd.utils.model import _interleave_cols, deinterleave_gate_up
    I, K = 32, 256
    g = torch.arange(I * K, dtype=torch.int32).reshape(I, K)
    u = g + 100000
    fused = interleave_rows8(g, u)
    assert np.array_equal(fused.numpy(), MF.fused_rows(g.numpy(), u.numpy()))
    # the fused module's output columns are the fused weight's rows: the [K, N] orientation of fuse_gate_up_interleaved
    assert torch.equal(fused.t(), _interleave_cols(g.t().contiguous(), u.t().contiguous(), 8))
    dg, du = deinterleave_gate_up(fused.t())
    assert torch.equal(dg, g.t()) and torch.equal(du, u.t())
    # scale rows: 1-D and 2-D
    assert interleave_rows8(torch.arange(16.), torch.arange(16.) + 50).tolist() == [*range(8), *range(50, 58), *range(8, 16), *range(58, 66)]
    # the same interleave on arrays already in the kernel layout
    rng = np.random.RandomState(0)
    gb, ub = rng.randint(0, 256, (I, K)).astype(np.uint8), rng.randint(0, 256, (I, K)).astype(np.uint8)
    want = np_tiled(MF.fused_rows(gb, ub))
    got = _interleave_tiled(torch.from_numpy(np_tiled(gb)), torch.from_numpy(np_tiled(ub)), I // 16, (K // 128) * 2)
    assert np.array_equal(got.numpy(), want)


# ---- C ABI -------------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_bound(lib):
    import os
    import re
    from conftest import ROOT
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gptqhip.h")).read(), flags=re.S)
    for s in NEW_SYMBOLS:
        assert re.search(r"\b" + s + r"\s*\(", text) and s in _lib.SIGNATURES and hasattr(lib, s), s
    assert lib.gptqhip_abi_version() == 21 and _lib.ABI_VERSION == 21
    assert callable(ops.moe_fp8_supported) and callable(ops.moe_fp8_gate_up) and callable(ops.moe_fp8_down)


def test_supported_predicate_table(lib):
    sup = lib.gptqhip_moe_fp8_supported
    #      H     I     gu_bc mode    br   bc   T   k
    yes = [(256, 128, 0, TENSOR, 0, 0, 1, 1), (256, 128, 0, ROW, 0, 0, 16, 16), (2048, 768, 128, BLOCK, 128, 128, 1, 8),
           (4096, 14336, 128, BLOCK, 128, 128, 16, 2), (1280, 128, 256, BLOCK, 32, 128, 5, 2), (384, 640, 128, BLOCK, 128, 128, 2, 3),
           (256, 256, 256, ROW, 0, 0, 1, 8), (256, 256, 0, BLOCK, 1, 256, 1, 8), (384, 640, 384, BLOCK, 3, 640, 1, 1)]
    for H, I, gbc, mode, br, bc, T, k in yes:
        for act in (0, 1):
            assert sup(H, I, gbc, mode, br, bc, T, k, act) == 1, (H, I, gbc, mode, br, bc, T, k)
    no = [(200, 128, 0, ROW, 0, 0, 1, 1),              # H % 128
          (256, 192, 0, ROW, 0, 0, 1, 1),              # I % 128
          (0, 128, 0, ROW, 0, 0, 1, 1), (256, 0, 0, ROW, 0, 0, 1, 1),
          (256, 128, 0, ROW, 0, 0, 0, 1), (256, 128, 0, ROW, 0, 0, 17, 1),      # T
          (256, 128, 0, ROW, 0, 0, 1, 0), (256, 128, 0, ROW, 0, 0, 1, 17),      # top_k
          (256, 128, 64, ROW, 0, 0, 1, 1),             # gate/up bc = 64
          (256, 128, 192, ROW, 0, 0, 1, 1),            # gate/up bc % 128
          (384, 128, 256, ROW, 0, 0, 1, 1),            # gate/up bc does not divide H
          (256, 128, -128, ROW, 0, 0, 1, 1),
          (256, 256, 0, BLOCK, 128, 64, 1, 1),         # down bc = 64
          (256, 384, 0, BLOCK, 128, 256, 1, 1),        # down bc does not divide I
          (256, 128, 0, BLOCK, 96, 128, 1, 1),         # down br does not divide H
          (256, 128, 0, BLOCK, 0, 128, 1, 1),          # down br < 1
          (256, 128, 0, 3, 0, 0, 1, 1)]                # no such scale layout
    for H, I, gbc, mode, br, bc, T, k in no:
        assert sup(H, I, gbc, mode, br, bc, T, k, 0) == 0, (H, I, gbc, mode, br, bc, T, k)
    assert sup(256, 128, 0, ROW, 0, 0, 1, 1, 2) == 0 and sup(256, 128, 0, ROW, 0, 0, 1, 1, -1) == 0      # fp32 / unknown activations
    assert ops.moe_fp8_supported(2048, 768, 128, BLOCK, (128, 128), 16, 8, torch.bfloat16)
    assert not ops.moe_fp8_supported(2048, 768, 128, BLOCK, (128, 128), 17, 8) and not ops.moe_fp8_supported(256, 128, dtype=torch.float32)


def test_every_entry_validates_before_touching_a_device(lib):
    one, odd16, odd4 = ctypes.c_void_p(256), ctypes.c_void_p(264), ctypes.c_void_p(258)
    err = lib.gptqhip_last_error
    gu, dn = lib.gptqhip_moe_fp8_gate_up, lib.gptqhip_moe_fp8_down

    def gate_up(x=one, w=one, rs=one, ids=one, act=one, st=one, T=1, k=2, E=4, H=256, I=128, bc=0, dt=0):
        return gu(x, w, rs, ids, act, st, T, k, E, H, I, bc, dt, None)

    def down(a=one, w=one, rs=one, ids=one, wt=one, out=one, st=one, T=1, k=2, E=4, H=256, I=128, mode=ROW, br=0, bc=0, dt=0):
        return dn(a, w, rs, ids, wt, out, st, T, k, E, H, I, mode, br, bc, dt, None)

    for name in ("x", "w", "rs", "ids", "act", "st"):
        assert gate_up(**{name: None}) == EINVAL and b"null" in err(), name
    for name in ("x", "w", "act"):
        assert gate_up(**{name: odd16}) == EINVAL and b"16-byte aligned" in err(), name
    for name in ("rs", "ids", "st"):
        assert gate_up(**{name: odd4}) == EINVAL and b"4-byte aligned" in err(), name
    for kw in (dict(T=0), dict(T=17), dict(k=0), dict(k=17)):
        assert gate_up(**kw) == EINVAL and b"must be 1..16" in err(), kw
    assert gate_up(E=0) == EINVAL and b"experts" in err()
    for kw in (dict(H=200), dict(I=192), dict(H=0), dict(I=-128)):
        assert gate_up(**kw) == EINVAL and b"multiples of 128" in err(), kw
    for kw in (dict(bc=64), dict(bc=192), dict(H=384, bc=256), dict(bc=-128)):
        assert gate_up(**kw) == EINVAL and b"block columns" in err(), kw
    for dt in (2, -1):
        assert gate_up(dt=dt) == EINVAL and b"dtype" in err()

    for name in ("a", "w", "rs", "ids", "wt", "out", "st"):
        assert down(**{name: None}) == EINVAL and b"null" in err(), name
    for name in ("a", "w", "out"):
        assert down(**{name: odd16}) == EINVAL and b"16-byte aligned" in err(), name
    for name in ("rs", "ids", "wt", "st"):
        assert down(**{name: odd4}) == EINVAL and b"4-byte aligned" in err(), name
    for kw in (dict(T=0), dict(T=17), dict(k=0), dict(k=17)):
        assert down(**kw) == EINVAL and b"must be 1..16" in err(), kw
    assert down(E=-1) == EINVAL and b"experts" in err()
    for kw in (dict(H=200), dict(I=192)):
        assert down(**kw) == EINVAL and b"multiples of 128" in err(), kw
    assert down(mode=3) == EINVAL and b"scale layout" in err()
    for kw in (dict(mode=BLOCK, br=128, bc=64), dict(mode=BLOCK, br=128, bc=256), dict(mode=BLOCK, br=128, bc=0)):
        assert down(**kw) == EINVAL and b"block columns" in err(), kw
    for kw in (dict(mode=BLOCK, br=96, bc=128), dict(mode=BLOCK, br=0, bc=128)):
        assert down(**kw) == EINVAL and b"block rows" in err(), kw
    assert down(dt=2) == EINVAL and b"dtype" in err()


def test_ops_refuse_cpu_tensors_and_wrong_tensors(lib):
    H, I, E, T, k = 256, 128, 2, 1, 2
    x = torch.zeros((T, H), dtype=torch.float16)
    w, rs = torch.zeros((E, 2 * I * H), dtype=torch.uint8), torch.ones((E, 2 * I))
    ids, st = torch.zeros((T, k), dtype=torch.int32), torch.zeros(1, dtype=torch.int32)
    act, out = torch.zeros((T * k, I), dtype=torch.float16), torch.zeros((T, H), dtype=torch.float16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.moe_fp8_gate_up(x, w, rs, ids, act, st, E, I)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.moe_fp8_down(act, torch.zeros((E, I * H), dtype=torch.uint8), torch.ones((E, H)), ids, torch.ones((T, k)), out, st, E, ROW)


# ---- module and fusion -------------------------------------------------------------------------------------------------------------------
def fp8_linear(K, N, method="block", block=(128, 128), bias=False, seed=0):
    kw = dict(weight_scale_method=method, weight_block_size=block) if method == "block" else dict(weight_scale_method=method)
    m = HipFp8Linear(bits=8, group_size=-1, sym=True, desc_act=False, in_features=K, out_features=N, bias=bias, **kw)
    m.weight.data = torch.from_numpy(F.make_codes(seed, N, K)).view(torch.float8_e4m3fn)
    return m


class _Expert(nn.Module):
    def __init__(self, gate, up, down):
        super().__init__()
        self.gate_proj, self.up_proj, self.down_proj, self.act_fn = gate, up, down, nn.SiLU()


class _Experts(nn.ModuleList):
    def forward(self, hidden_states, top_k_index, top_k_weights):
        raise AssertionError("not called here")


class _Block(nn.Module):
    def __init__(self, experts):
        super().__init__()
        self.experts = experts


def cpu_lists(E=2, H=256, I=128, **kw):
    return ([fp8_linear(H, I, seed=3 * e, **kw) for e in range(E)], [fp8_linear(H, I, seed=3 * e + 1, **kw) for e in range(E)],
            [fp8_linear(I, H, seed=3 * e + 2, **kw) for e in range(E)])


def test_from_linears_declines_with_nothing_modified(kernels_available, lib):
    def declined(lists, match):
        sizes = [m.weight.numel() for l in lists for m in l]
        with pytest.raises(NotImplementedError, match=match):
            HipFp8MoeExperts.from_linears(*lists)
        assert [m.weight.numel() for l in lists for m in l] == sizes and all(m.weight.dtype == torch.float8_e4m3fn for l in lists for m in l if isinstance(m, HipFp8Linear))

    declined(cpu_lists(), "ROCm device")                                   # CPU buffers
    g, u, d = cpu_lists()
    declined((g, u[:1], d), "equal-length")
    g, u, d = cpu_lists()
    u[1] = fp8_linear(256, 128, bias=True)
    declined((g, u, d), "biases")
    g, u, d = cpu_lists()
    d[0].adapter = object()
    declined((g, u, d), "adapters")
    g, u, d = cpu_lists()
    u[1] = fp8_linear(256, 256)
    declined((g, u, d), "shape")
    g, u, d = cpu_lists()
    u[0] = fp8_linear(256, 128, block=(64, 128))                           # gate / up differ
    declined((g, u, d), "block size")
    g, u, d = cpu_lists()
    g[1], u[1] = fp8_linear(256, 128, method="row"), fp8_linear(256, 128, method="row")      # experts differ
    declined((g, u, d), "scale method")
    g, u, d = cpu_lists()
    d[1] = fp8_linear(128, 256, block=(64, 128))                           # down differs between experts
    declined((g, u, d), "block size")
    g, u, d = cpu_lists()
    g[0] = nn.Linear(256, 128, bias=False)
    declined((g, u, d), "not a HIP FP8 linear")
    with pytest.raises(NotImplementedError, match="inference only"):
        HipFp8MoeExperts(2, 256, 128, "row", None, "block", (128, 128)).train(True)
    m = HipFp8MoeExperts(2, 256, 128, "block", (128, 128), "row", None)
    assert m.eval() is m and "format=float8_e4m3fn" in m.extra_repr() and "gate_up_scales=block(128, 128)" in m.extra_repr() \
        and "down_scales=row" in m.extra_repr()


def test_fuse_moe_experts_declines_cpu_modules_with_the_reason_recorded(kernels_available, lib):
    from gptqmodel_amd.utils.moe import auto_fuse_moe, fuse_moe_experts
    g, u, d = cpu_lists()
    blk = _Block(_Experts([_Expert(*t) for t in zip(g, u, d)]))
    before = blk.experts
    assert fuse_moe_experts(blk) is False and blk.experts is before and "ROCm device" in blk._gptqhip_moe_skipped
    # a mix of FP8 and other projections is declined before either stand-in is tried
    g, u, d = cpu_lists()
    d[1] = nn.Linear(128, 256, bias=False)
    mixed = _Block(_Experts([_Expert(*t) for t in zip(g, u, d)]))
    assert fuse_moe_experts(mixed) is False and "mix FP8" in mixed._gptqhip_moe_skipped and isinstance(mixed.experts, _Experts)
    # mismatched block sizes
    g, u, d = cpu_lists()
    u[0] = fp8_linear(256, 128, block=(64, 128))
    mism = _Block(_Experts([_Expert(*t) for t in zip(g, u, d)]))
    assert fuse_moe_experts(mism) is False and "block size" in mism._gptqhip_moe_skipped
    model = nn.Sequential(blk, mixed)
    assert auto_fuse_moe(model) == 0 and len(model._gptqhip_moe_skipped) == 2
