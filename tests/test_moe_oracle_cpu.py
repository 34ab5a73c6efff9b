"""Fused MoE experts, the part that needs no GPU: the oracle composition is self-consistent, the host-side predicate and argument validation
of the gptqhip_moe_* entry points answer without touching a device, and the bar tests/test_gpu_moe.py holds stage two to is meaningful on
its own inputs (one rounding of the float64 result is never further from it than the reference chain is)."""
import ctypes
import os
import zlib

import numpy as np
import pytest

import moe_oracle as MO
from helpers import WEIGHT_RANGE_DTYPES
from oracle import gptq_oracle as O


@pytest.fixture(scope="module")
def lib():
    from gptqmodel_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


@pytest.mark.parametrize("act,scale_dtype", WEIGHT_RANGE_DTYPES)
def test_one_hot_routing_reproduces_the_single_expert_mlp_bit_for_bit(act, scale_dtype):
    shape = "384x640e5k3"
    H, I, E, _, gs = MO.SHAPES[shape]
    x = MO.make_x(11, 3, H, act)
    ids = np.array([[4], [0], [4]], np.int32)
    rw = np.ones((3, 1), np.float32)
    got = MO.evaluate(MO.rounded_weights(shape, act, scale_dtype), x, ids, rw, act)
    for t in range(3):
        ex = MO.experts_of(shape, scale_dtype)[int(ids[t, 0])]
        fwd = lambda name, v: O.forward_gptq(v, *ex[name], 4, act_dtype=act, scale_dtype=scale_dtype)   # noqa: E731
        h = O.silu_mul_ref(fwd("gate", x[t:t + 1]), fwd("up", x[t:t + 1]), act)
        assert np.array_equal(got["act_ref"][t], h[0])
        assert np.array_equal(got["chain"][t], fwd("down", h)[0])
    # float64 on the same rounded weights, rounded once: within one rounding of the chain's fp32 matmul
    assert MO.rel64(got["y_once"], got["y64"]) <= MO.rel64(got["chain"], got["y64"]) + 1e-6


def test_moe_supported_is_host_logic(lib):
    from gptqmodel_amd import ops
    for H, I, k in ((2048, 768, 8), (4096, 14336, 2)):          # Qwen3-30B-A3B, Mixtral-8x7B
        for T in (1, 16):
            assert lib.gptqhip_moe_supported(H, I, 128, 4, 0, T, k) == 1 and ops.moe_supported(H, I, 128, 4, False, T, k)
    ok = (2048, 768, 128, 4, 0, 1, 8)
    for i, bad in ((3, 8), (4, 1), (2, 64), (1, 704), (5, 17), (6, 0)):     # bits 8, has_perm, gs 64, I = 704, T = 17, top_k = 0
        args = list(ok)
        args[i] = bad
        assert lib.gptqhip_moe_supported(*args) == 0, args
    assert lib.gptqhip_moe_supported(2048, 768, 256, 4, 0, 4, 16) == 1 and lib.gptqhip_moe_supported(2048, 768, 384, 4, 0, 4, 8) == 0
    assert lib.gptqhip_moe_supported(512, 256, -1, 4, 0, 2, 4) == 1       # one group for the whole K of each projection
    assert lib.gptqhip_moe_supported(512, 256, 512, 4, 0, 2, 4) == 0      # ... which a single explicit group size cannot say when H != I


def test_moe_entry_points_validate_before_any_device_access(lib):
    EINVAL = -22
    one, odd = ctypes.c_void_p(256), ctypes.c_void_p(260)
    gu = lambda *a: lib.gptqhip_moe_gate_up(*a)       # noqa: E731  (x, qw, meta, ids, act, status, T, k, E, H, I, gs, bits, adt, sdt, stream)
    dn = lambda *a: lib.gptqhip_moe_down(*a)          # noqa: E731  (act, qw, meta, ids, weights, out, status, T, k, E, H, I, gs, bits, adt, sdt, stream)
    tail = (8, 2048, 768, 128, 4, 0, 0, None)
    assert gu(None, one, one, one, one, one, 1, 8, *tail) == EINVAL and b"null" in lib.gptqhip_last_error()
    assert gu(one, one, one, one, one, None, 1, 8, *tail) == EINVAL and b"null" in lib.gptqhip_last_error()
    assert dn(one, one, one, one, None, one, one, 1, 8, *tail) == EINVAL and b"null" in lib.gptqhip_last_error()
    assert gu(one, one, one, one, one, one, 17, 8, *tail) == EINVAL and b"T=17" in lib.gptqhip_last_error()
    assert dn(one, one, one, one, one, one, one, 0, 8, *tail) == EINVAL and b"T=0" in lib.gptqhip_last_error()
    assert dn(one, one, one, one, one, one, one, 1, 17, *tail) == EINVAL and b"top_k=17" in lib.gptqhip_last_error()
    assert gu(odd, one, one, one, one, one, 1, 8, *tail) == EINVAL and b"aligned" in lib.gptqhip_last_error()
    assert gu(one, one, one, one, one, one, 1, 8, 8, 2048, 704, 128, 4, 0, 0, None) == EINVAL and b"shape" in lib.gptqhip_last_error()
    assert gu(one, one, one, one, one, one, 1, 8, 8, 2048, 768, 64, 4, 0, 0, None) == EINVAL
    assert dn(one, one, one, one, one, one, one, 1, 8, 8, 2048, 768, 128, 8, 0, 0, None) == EINVAL
    assert gu(one, one, one, one, one, one, 1, 8, 8, 2048, 768, 128, 4, 1, 0, None) == EINVAL and b"dtypes" in lib.gptqhip_last_error()
    assert gu(one, one, one, one, one, one, 1, 8, 0, 2048, 768, 128, 4, 0, 0, None) == EINVAL


def test_moe_ops_refuse_cpu_tensors(lib):
    import torch
    from gptqmodel_amd import ops
    x = torch.zeros((1, 256), dtype=torch.float16)
    w = torch.zeros(256, dtype=torch.int32)
    ids = torch.zeros((1, 2), dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.moe_gate_up(x, w, w, ids, torch.zeros((2, 128), dtype=torch.float16), ids, 8, 128, 128, torch.float16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.moe_down(torch.zeros((2, 128), dtype=torch.float16), w, w, ids, torch.zeros((1, 2)), x, ids, 8, 128, torch.float16)


@pytest.mark.parametrize("act,scale_dtype", WEIGHT_RANGE_DTYPES)
@pytest.mark.parametrize("T", MO.TOKENS)
@pytest.mark.parametrize("shape", sorted(MO.SHAPES))
def test_bar_in_force_on_the_gpu_test_inputs(shape, T, act, scale_dtype):
    """The GPU bar is `no worse than the reference chain or one output rounding, + 1e-4`.  It only asks something of the kernel while one
    rounding of the float64 result is not the larger of the two terms: checked here for every parametrisation of tests/test_gpu_moe.py."""
    c = MO.case(shape, T, act, scale_dtype)
    e_chain, e_once = MO.rel64(c["chain"], c["y64"]), MO.rel64(c["y_once"], c["y64"])
    print(f"{shape} T={T} {act}x{scale_dtype}: rel_err(chain, y64)={e_chain:.3e} rel_err(y64 rounded once, y64)={e_once:.3e}")
    assert e_once <= e_chain, (e_once, e_chain)
    assert np.isfinite(c["chain"]).all() and float(np.abs(c["y64"]).max()) > 1e-3


@pytest.mark.parametrize("act,scale_dtype", WEIGHT_RANGE_DTYPES)
@pytest.mark.parametrize("T", MO.DEEP_TOKENS)
@pytest.mark.parametrize("shape", sorted(MO.DEEP_SHAPES))
def test_bar_in_force_on_the_deep_gpu_test_inputs(shape, T, act, scale_dtype):
    """The condition of test_bar_in_force_on_the_gpu_test_inputs on every case of test_deep_k_and_wide_top_k_against_the_oracle."""
    c = MO.case(shape, T, act, scale_dtype)
    e_chain, e_once = MO.rel64(c["chain"], c["y64"]), MO.rel64(c["y_once"], c["y64"])
    print(f"{shape} T={T} {act}x{scale_dtype}: rel_err(chain, y64)={e_chain:.3e} rel_err(y64 rounded once, y64)={e_once:.3e} "
          f"max|act_ref|={float(np.abs(c['act_ref']).max()):.3g}")
    assert e_once <= e_chain, (e_once, e_chain)
    assert np.isfinite(c["chain"]).all() and np.isfinite(c["act_ref"]).all() and float(np.abs(c["y64"]).max()) > 1e-3


def crc(a) -> int:
    return zlib.crc32(np.ascontiguousarray(a).tobytes())


# (shape, T, act, scale_dtype) -> crc32 of x, ids, rw, expert 0's gate qweight, the last expert's down scales and chain, recorded on the commit
# before DEEP_SHAPES existed: adding shapes must not move the seeds, and with them the inputs, of any case that was there before
PINNED_INPUTS = {
    ("384x640e5k3", 5, "fp16", "fp16"): (3309585142, 835754259, 631227568, 2735770339, 2432401560, 1693009199),
    ("512x256e4k4gK", 16, "bf16", "bf16"): (2907791435, 1350817424, 2812721836, 4073838750, 358299668, 696317412),
    ("256x128e8k2", 1, "fp16", "bf16"): (730660419, 3602260385, 609785316, 1835270922, 2075872091, 1310518014),
    (MO.GS64_SHAPE, 17, "fp16", "fp16"): (3514689607, 3191745950, 2445480233, 2770426853, 676093602, 1817073913),
}


@pytest.mark.parametrize("key", sorted(PINNED_INPUTS))
def test_inputs_of_the_existing_cases_keep_their_bits(key):
    shape, T, act, scale_dtype = key
    c, ex = MO.case(*key), MO.experts_of(shape, scale_dtype)
    assert c["x"].dtype == np.float32 and c["ids"].dtype == np.int32 and ex[0]["gate"][0].dtype == np.int32
    got = (crc(c["x"]), crc(c["ids"]), crc(c["rw"]), crc(ex[0]["gate"][0]), crc(ex[-1]["down"][2]), crc(c["chain"]))
    assert got == PINNED_INPUTS[key], got


def test_deep_shapes_have_seeds_of_their_own():
    assert not set(MO.DEEP_SHAPES) & set(MO.SHAPES) and MO.GS64_SHAPE not in MO.DEEP_SHAPES
    old = {MO._seed_index(s) for s in MO._SEEDED_SHAPES}
    new = {MO._seed_index(s) for s in MO.DEEP_SHAPES}
    assert old == set(range(len(MO._SEEDED_SHAPES))) and len(new) == len(MO.DEEP_SHAPES) and min(new) > max(old)
