"""NVFP4 weight-only linear without a GPU: the oracle's tables, the premise of the kernels (every code x scale product is exact in fp16 and
bf16), the host quantiser, the C ABI's predicate and argument validation, kernel selection, the class contract and what fuse_moe_experts
declines.  Nothing here launches a kernel."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

import fp4_oracle as F4
from conftest import ROOT
from gptqmodel_amd import _lib, ops
from gptqmodel_amd.nn_modules.qlinear.hip_fp4 import E2M1_VALUES, HipFp4Linear, quantize_nvfp4_weight
from gptqmodel_amd.utils import importer
from gptqmodel_amd.utils.backend import BACKEND, normalize_backend
from gptqmodel_amd.utils.const import DEVICE, FORMAT, METHOD

EINVAL = -22
NEW_SYMBOLS = ("gptqhip_fp4_supported", "gptqhip_fp4_tiled_bytes", "gptqhip_fp4_scale_bytes", "gptqhip_fp4_repack", "gptqhip_fp4_gemm",
               "gptqhip_fp4_dequant")
MAX_ROWS = 65535 * 64      # gptqhip_fp8_gemm's limit


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


@pytest.fixture
def kernels_available(monkeypatch):
    """Pretend the native library + a gfx950 device are usable (nothing here launches a kernel)."""
    monkeypatch.setattr(HipFp4Linear, "validate_once", classmethod(lambda c: (True, None)))
    HipFp4Linear.cached_validate_once.cache_clear()
    yield
    HipFp4Linear.cached_validate_once.cache_clear()


# ---- tables and the premise ---------------------------------------------------------------------------------------------------------------
def test_decode_table_and_nibble_order():
    mags = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]
    assert list(F4.E2M1[:8]) == mags and list(F4.E2M1[8:]) == [-m for m in mags] and np.signbit(F4.E2M1[8])
    assert list(E2M1_VALUES) == mags
    for c in range(16):        # `s e1 e0 m`
        s, e, m = c >> 3, (c >> 1) & 3, c & 1
        v = m * 0.5 if e == 0 else (1 + m / 2) * 2.0 ** (e - 1)
        assert F4.E2M1[c] == (-v if s else v)
    if hasattr(torch, "float4_e2m1fn_x2"):
        assert torch.zeros(4, dtype=torch.uint8).view(torch.float4_e2m1fn_x2).element_size() == 1
    packed = np.array([[0x21, 0xF7]], np.uint8)           # byte b: low nibble = feature 2 b, high nibble = feature 2 b + 1
    assert F4.unpack(packed).tolist() == [[1, 2, 7, 15]] and np.array_equal(F4.pack(F4.unpack(packed)), packed)
    codes = np.arange(16, dtype=np.uint8).reshape(1, 16)
    assert np.array_equal(F4.weights64(codes, np.array([[0x40]], np.uint8), 0.5), F4.E2M1[None, :] * 2.0 * 0.5)       # 0x40 = 2.0


def test_every_code_times_every_finite_scale_is_exact_in_fp16_and_bf16():
    """The premise of the kernels: 16 codes x 254 finite e4m3 bytes, every product representable in both 16-bit dtypes."""
    prod = F4.E2M1[:, None] * F4.E4M3[F4.FINITE_CODES][None, :]
    assert prod.shape == (16, 254) and np.isfinite(prod).all()
    for act in ("fp16", "bf16"):
        assert np.array_equal(F4.round_to(prod, act), prod), act
    nz = np.abs(prod[prod != 0])
    assert nz.min() == 2.0 ** -10 and nz.max() == 2688.0
    m, _ = np.frexp(nz)
    assert np.array_equal(m * 64, np.round(m * 64))          # at most 6 significant bits


def test_chain_and_once_agree_with_float64_to_their_roundings():
    c = F4.case(3, 256, 48, "fp16", True)
    assert c["y64"].shape == (3, 48) and np.isfinite(c["chain"]).all()
    assert F4.rel64(c["y_once"], c["y64"]) <= 2.0 ** -11 and F4.rel64(c["chain"], c["y64"]) <= 5e-3
    codes, scale = F4.layer(256, 48)
    assert np.array_equal(F4.kernel_w(codes, scale, 1.0).astype(np.float64), F4.block_weights64(codes, scale))
    assert np.abs(F4.kernel_w(codes, scale, F4.S2) / np.maximum(np.abs(F4.weights64(codes, scale, F4.S2)), 1e-300)
                  - np.sign(F4.weights64(codes, scale, F4.S2))).max() <= 2.0 ** -23 + 1.0    # one fp32 rounding (zeros: 0 / tiny)


# ---- quantiser -------------------------------------------------------------------------------------------------------------------------------
def grid_weight(N=32, K=256, s2=2.0 ** -10 * 1.3125, seed=0):
    """Weights already on the NVFP4 grid whose quantisation is unique: every block holds a +-6 (so block_amax / 6 / scale_2 is its scale), the
    largest scale is 448 (so scale_2 = amax / 2688 is s2 -- s2 has few mantissa bits, every product below is exact in fp32), scales are
    positive normals."""
    rng = np.random.RandomState(seed)
    codes = rng.randint(0, 16, size=(N, K)).astype(np.uint8)
    codes[:, 0::16] = np.where(rng.rand(N, K // 16) < 0.5, 7, 15)
    scale = rng.randint(0x08, 0x7F, size=(N, K // 16)).astype(np.uint8)
    scale[0, 0] = 0x7E
    w = (F4.block_weights64(codes, scale) * s2).astype(np.float32)
    return codes, scale, np.float32(s2), w


def test_quantiser_round_trips_weights_on_the_grid():
    codes, scale, s2, w = grid_weight()
    packed, qs, qs2 = quantize_nvfp4_weight(torch.from_numpy(w))
    assert packed.dtype == torch.uint8 and tuple(packed.shape) == (32, 128)
    assert qs.dtype == torch.float8_e4m3fn and tuple(qs.shape) == (32, 16)
    assert qs2.dtype == torch.float32 and tuple(qs2.shape) == ()
    assert float(qs2) == float(s2)
    assert np.array_equal(qs.view(torch.uint8).numpy(), scale)
    got = F4.unpack(packed.numpy())
    same = (got == codes) | ((got & 7) == 0) & ((codes & 7) == 0)        # (the quantiser sees -0.0 weights: their sign bit survives or not)
    assert same.all()
    assert np.array_equal(F4.weights64(got, qs.view(torch.uint8).numpy(), float(qs2)).astype(np.float32), w)


def test_quantiser_on_random_weights_zero_blocks_and_ties():
    rng = np.random.RandomState(4)
    w = (rng.randn(48, 384) * 0.02).astype(np.float32)
    w[5, 32:48] = 0.0                                   # an all-zero block
    w[7] = 0.0                                          # an all-zero row
    packed, qs, qs2 = quantize_nvfp4_weight(torch.from_numpy(w))
    codes, sb = F4.unpack(packed.numpy()), qs.view(torch.uint8).numpy()
    assert float(qs2) == float(np.float32(np.abs(w).max()) / np.float32(2688.0))
    assert (sb[5, 2] == 0) and (codes[5, 32:48] == 0).all() and (sb[7] == 0).all() and (codes[7] == 0).all()
    assert ((sb & 0x7F) != 0x7F).all() and (sb < 0x80).all()            # finite, non-negative scales
    rec = F4.weights64(codes, sb, float(qs2))
    step = np.repeat(F4.E4M3[sb], 16, axis=1) * float(qs2)                # the widest code step is 2 (4 -> 6): half of it is one block scale
    live = step > 0
    assert (np.abs(rec - w)[live] <= step[live] * (1 + 1e-6)).all()
    small = np.abs(w) <= 2 * step                                         # below 2 the code step is 0.5: within a quarter of the block scale
    assert (np.abs(rec - w)[live & small] <= 0.25 * step[live & small] * (1 + 1e-6)).all()
    # ties go to the even code, and values beyond 6 clamp: one block with scale 1 (amax 6 x 448 elsewhere pins scale_2 to 1)
    t = np.zeros((16, 128), np.float32)
    t[0, :16] = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, 6.0, -0.25, -0.75, -1.25, -1.75, -2.5, -3.5, -5.0, -6.0]
    t[1, 0] = 2688.0
    p, s, s2 = quantize_nvfp4_weight(torch.from_numpy(t))
    assert float(s2) == 1.0 and s.view(torch.uint8)[0, 0] == 0x38 and s.view(torch.uint8)[1, 0] == 0x7E
    assert F4.unpack(p.numpy())[0, :16].tolist() == [0, 2, 2, 4, 4, 6, 6, 7, 8, 10, 10, 12, 12, 14, 14, 15]
    with pytest.raises(ValueError, match="2D"):
        quantize_nvfp4_weight(torch.zeros(4))
    with pytest.raises(ValueError, match="divisible"):
        quantize_nvfp4_weight(torch.zeros(4, 24))


def test_module_pack_fills_the_checkpoint_buffers(kernels_available):
    codes, scale, s2, w = grid_weight(N=32, K=256)
    lin = nn.Linear(256, 32, bias=True)
    with torch.no_grad():
        lin.weight.copy_(torch.from_numpy(w))
    m = HipFp4Linear(bits=4, group_size=16, sym=True, desc_act=False, in_features=256, out_features=32, bias=True, weight_block_size=16)
    assert m.weight.dtype == torch.uint8 and tuple(m.weight.shape) == (32, 128) and tuple(m.weight_scale.shape) == (32, 16)
    assert m.weight_scale.dtype == torch.float8_e4m3fn and tuple(m.weight_scale_2.shape) == () and float(m.weight_scale_2) == 1.0
    for fn in (m.pack, m.pack_block, m.pack_original):
        fn(lin, None, None)
        assert np.array_equal(m.weight_scale.view(torch.uint8).numpy(), scale) and float(m.weight_scale_2) == float(s2)
        assert m.bias.dtype == torch.float16 and sorted(m.state_dict()) == ["bias", "weight", "weight_scale", "weight_scale_2"]
    with pytest.raises(RuntimeError, match="before post_init"):
        m(torch.zeros(1, 256))
    with pytest.raises(ValueError, match="weight shape"):
        m.pack(nn.Linear(128, 32), None, None)


# ---- C ABI -----------------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_bound(lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gptqhip.h")).read(), flags=re.S)
    for s in NEW_SYMBOLS:
        assert re.search(r"\b" + s + r"\s*\(", text) and s in _lib.SIGNATURES and hasattr(lib, s), s
    assert lib.gptqhip_abi_version() == 21 and _lib.ABI_VERSION == 21
    assert "#define GPTQHIP_ABI_VERSION 21" in open(os.path.join(ROOT, "include", "gptqhip.h")).read()


def test_supported_predicate_table_and_size_helpers(lib):
    sup = lib.gptqhip_fp4_supported
    for M, K, N in [(1, 128, 16), (16, 4096, 4096), (17, 256, 48), (4096, 14336, 4096), (1, 1152, 272), (0, 4096, 4096), (MAX_ROWS, 128, 16),
                    (1, 4096, 28672)]:
        for act in (0, 1):
            assert sup(M, K, N, 16, act) == 1, (M, K, N)
    no = [(1, 100, 16, 16), (1, 192, 16, 16), (1, 64, 16, 16),      # K % 128
          (1, 128, 24, 16), (1, 128, 8, 16),                          # N % 16
          (1, 256, 48, 32), (1, 256, 48, 8), (1, 256, 48, 128), (1, 256, 48, 0), (1, 256, 48, -1),   # block 16 only
          (-1, 256, 48, 16), (MAX_ROWS + 1, 256, 48, 16), (1, 0, 48, 16), (1, 256, 0, 16), (1, -128, 48, 16)]
    for M, K, N, blk in no:
        assert sup(M, K, N, blk, 0) == 0, (M, K, N, blk)
    for act in (2, 3, -1):                                              # fp32 and unknown activation dtypes
        assert sup(1, 256, 48, 16, act) == 0
    assert ops.fp4_supported(1, 256, 48, 16, torch.bfloat16) and not ops.fp4_supported(1, 256, 48, 16, torch.float32)
    assert not ops.fp4_supported(1, 256, 48, 32) and ops.fp4_supported(0, 256, 48)
    assert lib.gptqhip_fp4_tiled_bytes(4096, 4096) == 4096 * 4096 // 2 and lib.gptqhip_fp4_scale_bytes(4096, 4096) == 4096 * 4096 // 16
    assert lib.gptqhip_fp4_tiled_bytes(128, 16) == 1024 and lib.gptqhip_fp4_scale_bytes(128, 16) == 128
    for K, N in ((100, 16), (128, 24), (0, 16), (128, 0)):
        assert lib.gptqhip_fp4_tiled_bytes(K, N) == 0 and lib.gptqhip_fp4_scale_bytes(K, N) == 0


def test_every_entry_validates_before_touching_a_device(lib):
    one, two, three, odd, odd4 = (ctypes.c_void_p(v) for v in (256, 512, 768, 264, 258))
    err = lib.gptqhip_last_error
    gemm, repack, deq = lib.gptqhip_fp4_gemm, lib.gptqhip_fp4_repack, lib.gptqhip_fp4_dequant
    # gemm(x, weight_t, scale_t, global_scale, bias, out, M, K, N, block, act, flags, stream)
    for i in (0, 1, 2, 5):
        args = [one, one, one, None, None, one]
        args[i] = None
        assert gemm(*args, 1, 256, 48, 16, 0, 0, None) == EINVAL and b"null" in err(), i
    for i in (0, 1, 2, 4, 5):
        args = [one, one, one, None, None, one]
        args[i] = odd
        assert gemm(*args, 1, 256, 48, 16, 0, 0, None) == EINVAL and b"aligned" in err(), i
    assert gemm(one, one, one, odd4, None, one, 1, 256, 48, 16, 0, 0, None) == EINVAL and b"global_scale" in err()
    assert gemm(one, one, one, None, None, one, 1, 100, 48, 16, 0, 0, None) == EINVAL and b"multiple of 128" in err()
    assert gemm(one, one, one, None, None, one, 1, 256, 40, 16, 0, 0, None) == EINVAL and b"multiple of 16" in err()
    assert gemm(one, one, one, None, None, one, 1, 256, 48, 32, 0, 0, None) == EINVAL and b"block size" in err()
    assert gemm(one, one, one, None, None, one, 1, 256, 48, 16, 2, 0, None) == EINVAL and b"dtype" in err()
    assert gemm(one, one, one, None, None, one, 1, 256, 48, 16, 0, 3, None) == EINVAL and b"flags" in err()
    assert gemm(one, one, one, None, None, one, 1, 256, 48, 16, 0, 4, None) == EINVAL and b"flags" in err()
    assert gemm(one, one, one, None, None, one, -1, 256, 48, 16, 0, 0, None) == EINVAL and b"M out of range" in err()
    assert gemm(one, one, one, None, None, one, MAX_ROWS + 1, 256, 48, 16, 0, 0, None) == EINVAL
    assert gemm(None, None, None, None, None, None, 0, 256, 48, 16, 0, 0, None) == 0      # empty batch: a no-op success
    # repack(weight, weight_scale, weight_t, scale_t, K, N, block, stream)
    assert repack(one, one, None, three, 256, 48, 16, None) == EINVAL and b"null" in err()
    assert repack(one, None, two, three, 256, 48, 16, None) == EINVAL and b"null" in err()
    assert repack(one, one, odd, three, 256, 48, 16, None) == EINVAL and b"aligned" in err()
    assert repack(one, two, one, three, 256, 48, 16, None) == EINVAL and b"in place" in err()
    assert repack(one, two, three, two, 256, 48, 16, None) == EINVAL and b"in place" in err()
    assert repack(one, one, two, three, 200, 48, 16, None) == EINVAL and b"multiple of 128" in err()
    assert repack(one, one, two, three, 256, 48, 32, None) == EINVAL and b"block size" in err()
    # dequant(weight_t, scale_t, global_scale, out, K, N, block, out_dtype, stream)
    assert deq(one, None, None, two, 256, 48, 16, 0, None) == EINVAL and b"null" in err()
    assert deq(one, one, None, None, 256, 48, 16, 0, None) == EINVAL and b"null" in err()
    assert deq(one, one, None, odd, 256, 48, 16, 0, None) == EINVAL and b"aligned" in err()
    assert deq(one, one, odd4, two, 256, 48, 16, 0, None) == EINVAL and b"global_scale" in err()
    assert deq(one, one, None, two, 256, 48, 16, 3, None) == EINVAL and b"dtype" in err()
    assert deq(one, one, None, two, 256, 40, 16, 2, None) == EINVAL and b"multiple of 16" in err()
    assert deq(one, one, None, two, 256, 48, 8, 2, None) == EINVAL and b"block size" in err()


def test_ops_refuse_cpu_tensors(lib):
    w = torch.zeros((16, 64), dtype=torch.uint8)
    s = torch.zeros((16, 8), dtype=torch.float8_e4m3fn)
    x = torch.zeros((1, 128), dtype=torch.float16)
    for call in (lambda: ops.fp4_repack(w, s),
                 lambda: ops.fp4_gemm(x, w.reshape(-1), s.view(torch.uint8).reshape(-1), None, None, 16),
                 lambda: ops.fp4_gemm(x, w.reshape(-1), s.view(torch.uint8).reshape(-1), torch.ones(1), None, 16),
                 lambda: ops.fp4_dequant(w.reshape(-1), s.view(torch.uint8).reshape(-1), None, 128, 16)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


# ---- selection and the class contract ---------------------------------------------------------------------------------------------------------
def test_enums_and_backend_alias():
    assert FORMAT.NVFP4.value == "nvfp4" and METHOD.NVFP4.value == "nvfp4" and BACKEND.FP4_HIP.value == "fp4_hip"
    assert normalize_backend("hip", quant_method=METHOD.NVFP4) is BACKEND.FP4_HIP
    assert normalize_backend("fp4_hip") is BACKEND.FP4_HIP
    assert normalize_backend("hip", quant_method=METHOD.GPTQ) is BACKEND.GPTQ_HIP     # unchanged
    assert normalize_backend("hip", quant_method=METHOD.FP8) is BACKEND.FP8_HIP
    assert normalize_backend("hip", quant_method=METHOD.AWQ) is BACKEND.AWQ_HIP


def test_selection_resolves_the_class(kernels_available):
    sel = importer.select_quant_linear
    assert sel(4, 16, False, True, device=DEVICE.ROCM, format=FORMAT.NVFP4, quant_method=METHOD.NVFP4) is HipFp4Linear
    assert sel(4, 16, False, True, device="cuda:0", backend="hip", format="nvfp4", quant_method="nvfp4", pack=True) is HipFp4Linear
    assert sel(4, 16, False, True, device="cuda:0", backend=BACKEND.FP4_HIP, format=FORMAT.NVFP4, quant_method=METHOD.NVFP4,
               dtype=torch.bfloat16) is HipFp4Linear
    assert importer.hf_select_quant_linear_v2(4, 16, False, True, format="nvfp4", quant_method="nvfp4") is HipFp4Linear
    assert importer.get_kernel_for_backend(BACKEND.HIP, METHOD.NVFP4, FORMAT.NVFP4) is HipFp4Linear
    assert importer.AUTO_BACKEND_KERNEL_MAPPING[METHOD.NVFP4][FORMAT.NVFP4][BACKEND.FP4_HIP] is HipFp4Linear
    assert HipFp4Linear.SUPPORTS_FORMATS[FORMAT.NVFP4] == 120
    with pytest.raises(NotImplementedError, match="bits"):
        sel(8, 16, False, True, device="cuda:0", format=FORMAT.NVFP4, quant_method=METHOD.NVFP4)
    for gs in (32, 128, -1):
        with pytest.raises(NotImplementedError, match="group_size"):
            sel(4, gs, False, True, device="cuda:0", format=FORMAT.NVFP4, quant_method=METHOD.NVFP4)
    with pytest.raises(NotImplementedError, match="dtype"):
        sel(4, 16, False, True, device="cuda:0", format=FORMAT.NVFP4, quant_method=METHOD.NVFP4, dtype=torch.float32)
    for method in (METHOD.GPTQ, METHOD.FP8, METHOD.AWQ):
        with pytest.raises(ValueError, match="Unsupported format"):
            sel(4, 16, False, True, device="cuda:0", format=FORMAT.NVFP4, quant_method=method)
    with pytest.raises(ValueError, match="Unsupported format"):
        sel(4, 16, False, True, device="cuda:0", format=FORMAT.GPTQ, quant_method=METHOD.NVFP4)
    # the GPTQ / AWQ / FP8 selections are what they were
    from gptqmodel_amd.nn_modules.qlinear.hip_awq import HipAwqLinear
    from gptqmodel_amd.nn_modules.qlinear.hip_fp8 import HipFp8Linear
    from gptqmodel_amd.nn_modules.qlinear.hip_gptq import HipGptqLinear
    assert importer.AUTO_BACKEND_KERNEL_MAPPING[METHOD.GPTQ][FORMAT.GPTQ][BACKEND.GPTQ_HIP] is HipGptqLinear
    assert importer.AUTO_BACKEND_KERNEL_MAPPING[METHOD.FP8][FORMAT.FP8][BACKEND.FP8_HIP] is HipFp8Linear
    assert importer.AUTO_BACKEND_KERNEL_MAPPING[METHOD.AWQ][FORMAT.GEMM][BACKEND.AWQ_HIP] is HipAwqLinear
    assert set(importer.AUTO_BACKEND_KERNEL_MAPPING) == {METHOD.GPTQ, METHOD.AWQ, METHOD.FP8, METHOD.NVFP4}


def test_class_contract_and_soft_fail_without_a_gpu():
    HipFp4Linear.verify_supports_params()
    assert HipFp4Linear.SUPPORTS_BITS == [4] and HipFp4Linear.SUPPORTS_GROUP_SIZE == [16] and HipFp4Linear.SUPPORTS_DEVICES == [DEVICE.ROCM]
    assert HipFp4Linear.SUPPORTS_IN_FEATURES_DIVISIBLE_BY == [128] and HipFp4Linear.SUPPORTS_OUT_FEATURES_DIVISIBLE_BY == [16]
    assert HipFp4Linear.SUPPORTS_DTYPES == [torch.float16, torch.bfloat16] and HipFp4Linear.SUPPORTS_METHODS == [METHOD.NVFP4]
    assert list(HipFp4Linear.SUPPORTS_FORMATS) == [FORMAT.NVFP4] and HipFp4Linear.SUPPORTS_BACKENDS == [BACKEND.FP4_HIP]
    from gptqmodel_amd.utils.adapter import Lora
    assert HipFp4Linear.SUPPORTS_ADAPTERS == [Lora] and HipFp4Linear in importer.iter_quant_linear_kernels()
    HipFp4Linear.cached_validate_once.cache_clear()
    if torch.cuda.is_available():
        return
    ok, err = HipFp4Linear.validate_once()
    assert ok is False and isinstance(err, ImportError)
    with pytest.raises(ImportError):
        importer.select_quant_linear(4, 16, False, True, device="cuda", format=FORMAT.NVFP4, quant_method=METHOD.NVFP4)
    HipFp4Linear.cached_validate_once.cache_clear()


KW = dict(bits=4, group_size=16, sym=True, desc_act=False, in_features=256, out_features=64)


def test_constructor_and_post_init_decline_what_the_kernels_do_not_serve(kernels_available):
    for blk in (32, 8, [1, 32], (128,)):
        with pytest.raises(NotImplementedError, match="weight_block_size"):
            HipFp4Linear(weight_block_size=blk, **KW)
    with pytest.raises(ValueError, match="weight_block_size"):
        HipFp4Linear(weight_block_size=(16, 16), **KW)
    with pytest.raises(NotImplementedError, match="group_size"):
        HipFp4Linear(**dict(KW, group_size=32))
    with pytest.raises(NotImplementedError, match="bits"):
        HipFp4Linear(**dict(KW, bits=8))
    with pytest.raises(NotImplementedError, match="in_features"):
        HipFp4Linear(**dict(KW, in_features=192))
    with pytest.raises(NotImplementedError, match="out_features"):
        HipFp4Linear(**dict(KW, out_features=40))
    for blk in (None, 16, [16], (1, 16)):
        assert HipFp4Linear(weight_block_size=blk, **KW).weight_block_size == 16

    def fresh():
        return HipFp4Linear(**KW).eval()

    m = fresh()
    m._buffers["weight_scale"] = torch.ones((64, 16), dtype=torch.float32)                       # an fp32 block scale
    with pytest.raises(NotImplementedError, match="float8_e4m3fn"):
        m.post_init()
    m = fresh()
    m._buffers["weight_scale"] = torch.zeros((128, 4), dtype=torch.float8_e4m3fn)                # a swizzled / padded scale layout
    with pytest.raises(NotImplementedError, match="swizzled"):
        m.post_init()
    m = fresh()
    m._buffers["weight_scale"] = torch.zeros(64 * 16, dtype=torch.float8_e4m3fn)                 # ... or a flattened one
    with pytest.raises(NotImplementedError, match="swizzled"):
        m.post_init()
    m = fresh()
    m._buffers["weight_scale_2"] = torch.ones(64, dtype=torch.float32)                           # per-row global scales
    with pytest.raises(NotImplementedError, match="weight_scale_2"):
        m.post_init()
    m = fresh()
    m._buffers["weight"] = torch.zeros((64, 256), dtype=torch.uint8)                             # one code per byte
    with pytest.raises(NotImplementedError, match="`weight` shape"):
        m.post_init()
    m = fresh()
    m._buffers["weight"] = torch.zeros((64, 128), dtype=torch.int8)
    with pytest.raises(NotImplementedError, match="expected uint8"):
        m.post_init()
    m = fresh()                                                                                  # everything right, but on the CPU
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.post_init()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.dequantize_weight()
    assert m._ready is False and sorted(m.state_dict()) == ["weight", "weight_scale", "weight_scale_2"]
    with pytest.raises(NotImplementedError, match="inference|train"):
        m.train(True)


# ---- fused MoE experts -----------------------------------------------------------------------------------------------------------------------
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


def test_fuse_moe_experts_declines_an_fp4_block_with_the_reason_recorded(kernels_available):
    from gptqmodel_amd.utils.moe import auto_fuse_moe, fuse_moe_experts

    def fp4(k, n):
        return HipFp4Linear(**dict(KW, in_features=k, out_features=n))

    blk = _Block(_Experts([_Expert(fp4(256, 128), fp4(256, 128), fp4(128, 256)) for _ in range(2)]))
    before = blk.experts
    assert fuse_moe_experts(blk) is False and blk.experts is before
    assert "NVFP4" in blk._gptqhip_moe_skipped and "HipFp4Linear" in blk._gptqhip_moe_skipped
    mixed = _Block(_Experts([_Expert(fp4(256, 128), nn.Linear(256, 128, bias=False), fp4(128, 256))]))
    assert fuse_moe_experts(mixed) is False and "NVFP4" in mixed._gptqhip_moe_skipped and isinstance(mixed.experts, _Experts)
    model = nn.Sequential(blk, mixed)
    assert auto_fuse_moe(model) == 0 and len(model._gptqhip_moe_skipped) == 2
