"""FP8 weight-only linear without a GPU: the oracle against goldens from the live reference (TorchFP8Linear.pack + forward on the CPU,
tests/dev/make_fp8_golden.py), the host packer bit for bit, the C ABI's predicate and argument validation, kernel selection and the class
contract.  Nothing here launches a kernel."""
import ctypes

import numpy as np
import pytest
import torch

import fp8_oracle as F
from conftest import load_golden
from gptqmodel_amd import _lib, ops
from gptqmodel_amd.nn_modules.qlinear.hip_fp8 import HipFp8Linear, quantize_fp8_weight
from gptqmodel_amd.utils import importer
from gptqmodel_amd.utils.backend import BACKEND, normalize_backend
from gptqmodel_amd.utils.const import DEVICE, FORMAT, METHOD

GOLDENS = [(m, a) for m in ("row", "tensor", "block") for a in ("fp16", "bf16")]
EINVAL = -22
TENSOR, ROW, BLOCK = ops.FP8_SCALE_TENSOR, ops.FP8_SCALE_ROW, ops.FP8_SCALE_BLOCK
NEW_SYMBOLS = ("gptqhip_fp8_supported", "gptqhip_fp8_tiled_bytes", "gptqhip_fp8_repack", "gptqhip_fp8_gemm", "gptqhip_fp8_dequant")


def golden(method, act):
    g = load_golden(f"ref_fp8_{method}_{act}.npz")
    block = tuple(int(v) for v in g["block"]) if method == "block" else None
    return g, block


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


# ---- oracle <-> goldens ------------------------------------------------------------------------------------------------------------------
def test_decode_table_is_torch_e4m3fn():
    t = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).to(torch.float64).numpy()
    assert np.array_equal(np.isnan(t), np.isnan(F.E4M3)) and int(np.isnan(t).sum()) == 2
    ok = ~np.isnan(t)
    assert np.array_equal(t[ok], F.E4M3[ok]) and np.array_equal(np.signbit(t[ok]), np.signbit(F.E4M3[ok]))
    assert F.E4M3[0x7e] == 448.0 and F.E4M3[0x01] == 2.0 ** -9 and F.FINITE_CODES.size == 254


@pytest.mark.parametrize("method,act", GOLDENS)
def test_chain_reproduces_the_reference_forward(method, act):
    """`chain` is the reference's forward restated: within ONE ulp of the dtype of what TorchFP8Linear.forward returned."""
    g, block = golden(method, act)
    got = F.chain(g["x"], g["weight"], g["scale_inv"], g["bias"], act, block)
    y = g["y"].astype(np.float64)
    eps = 2.0 ** -10 if act == "fp16" else 2.0 ** -7
    ulp = np.maximum(2.0 ** np.floor(np.log2(np.maximum(np.abs(y), 2.0 ** -14))) * eps, 0)
    assert np.all(np.abs(got - y) <= ulp), float(np.abs(got - y).max())


@pytest.mark.parametrize("method,act", GOLDENS)
def test_one_rounding_is_no_further_from_float64_than_the_reference(method, act):
    g, block = golden(method, act)
    ref = F.y64(g["x"], g["weight"], g["scale_inv"], g["bias"], block)
    once = F.y_once(g["x"], g["weight"], g["scale_inv"], g["bias"], act, block)
    assert F.rel64(once, ref) <= F.rel64(g["y"], ref)
    # and the kernels' weight arithmetic (fp32 reciprocal, fp32 product) is within 2^-22 of the quotient: noise next to either dtype's rounding
    w64 = F.weights64(g["weight"], g["scale_inv"], block)
    assert np.all(np.abs(F.kernel_w(g["weight"], g["scale_inv"], block) - w64) <= np.abs(w64) * 2.0 ** -22)


# ---- packer ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method,act", GOLDENS)
def test_packer_reproduces_the_reference_bytes(method, act):
    g, block = golden(method, act)
    codes, scale_inv = quantize_fp8_weight(torch.from_numpy(g["w"]), method, block)
    assert codes.dtype == torch.float8_e4m3fn and scale_inv.dtype == torch.float32
    assert np.array_equal(codes.view(torch.uint8).numpy(), g["weight"])
    assert scale_inv.numpy().shape == g["scale_inv"].shape
    assert np.array_equal(scale_inv.numpy().view(np.uint32), g["scale_inv"].view(np.uint32))
    assert not np.isin(g["weight"], (0x7f, 0xff)).any()      # the packer never emits a NaN code


def test_module_pack_fills_the_checkpoint_buffers(kernels_available):
    g, block = golden("block", "fp16")
    N, K = g["weight"].shape
    lin = torch.nn.Linear(K, N, bias=True)
    with torch.no_grad():
        lin.weight.copy_(torch.from_numpy(g["w"]))
        lin.bias.copy_(torch.from_numpy(g["bias"]))
    cls = importer.select_quant_linear(8, -1, False, True, device=DEVICE.ROCM, format=FORMAT.FP8, quant_method=METHOD.FP8, pack=True)
    assert cls is HipFp8Linear
    m = cls(bits=8, group_size=-1, sym=True, desc_act=False, in_features=K, out_features=N, bias=True,
            weight_scale_method="block", weight_block_size=block)
    assert m.weight.dtype == torch.float8_e4m3fn and tuple(m.weight.shape) == (N, K) and tuple(m.weight_scale_inv.shape) == (2, 2)
    m.pack(lin, None, None)
    assert np.array_equal(m.weight.view(torch.uint8).numpy(), g["weight"])
    assert np.array_equal(m.weight_scale_inv.numpy(), g["scale_inv"])
    assert m.bias.dtype == torch.float16 and np.array_equal(m.bias.float().numpy(), g["bias"])
    assert [tuple(t.shape) for t in m.list_buffers()] == [(N, K), (2, 2), (N,)]
    assert "format=float8_e4m3fn" in m.extra_repr() and "weight_scale_method=block" in m.extra_repr()
    assert sorted(m.state_dict()) == ["bias", "weight", "weight_scale_inv"]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.post_init()
    with pytest.raises(RuntimeError, match="before post_init"):
        m(torch.zeros(1, K, dtype=torch.float16))
    for method, shape in (("tensor", ()), ("row", (N,))):
        mm = cls(bits=8, group_size=-1, sym=True, desc_act=False, in_features=K, out_features=N, weight_scale_method=method)
        assert tuple(mm.weight_scale_inv.shape) == shape and mm.bias is None
        gg, _ = golden(method, "fp16")
        with torch.no_grad():
            lin.weight.copy_(torch.from_numpy(gg["w"]))
        mm.pack_original(lin, None, None)
        assert np.array_equal(mm.weight.view(torch.uint8).numpy(), gg["weight"])


# ---- C ABI -----------------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_bound(lib):
    for s in NEW_SYMBOLS:
        assert s in _lib.SIGNATURES and hasattr(lib, s)
    assert lib.gptqhip_abi_version() == 21


def test_supported_predicate_table(lib):
    sup = lib.gptqhip_fp8_supported
    yes = [(1, 128, 16, TENSOR, 0, 0), (16, 4096, 4096, ROW, 0, 0), (17, 256, 48, ROW, 0, 0), (4096, 14336, 4096, BLOCK, 128, 128),
           (1, 1152, 272, BLOCK, 16, 128), (3, 256, 48, BLOCK, 48, 256), (1, 256, 48, BLOCK, 1, 128), (1, 256, 48, BLOCK, 3, 128),
           (0, 4096, 4096, ROW, 0, 0), (1, 4096, 28672, BLOCK, 128, 512)]
    for M, K, N, mode, br, bc in yes:
        for act in (0, 1):
            assert sup(M, K, N, mode, br, bc, act, 0) == 1, (M, K, N, mode, br, bc)
    no = [(1, 100, 16, ROW, 0, 0),            # K = 100
          (1, 192, 16, ROW, 0, 0),            # K % 128
          (1, 128, 24, ROW, 0, 0),            # N % 16
          (1, 256, 48, BLOCK, 16, 64),        # bc = 64
          (1, 256, 48, BLOCK, 16, 192),       # bc % 128
          (1, 384, 48, BLOCK, 16, 256),       # bc does not divide K
          (1, 256, 48, BLOCK, 32, 128),       # br does not divide N
          (1, 256, 48, BLOCK, 0, 128),        # br < 1
          (1, 256, 48, 3, 0, 0),              # no such scale layout
          (-1, 256, 48, ROW, 0, 0), (1, 0, 48, ROW, 0, 0), (1, 256, 0, ROW, 0, 0)]
    for M, K, N, mode, br, bc in no:
        assert sup(M, K, N, mode, br, bc, 0, 0) == 0, (M, K, N, mode, br, bc)
    assert sup(1, 256, 48, ROW, 0, 0, 2, 0) == 0                      # fp32 activations
    for fmt in (1, 2, 3, 7):                                           # float8_e5m2, float8_e4m3fnuz, float8_e8m0fnu, unknown
        assert sup(1, 256, 48, ROW, 0, 0, 0, fmt) == 0
    assert ops.fp8_supported(1, 256, 48, BLOCK, (16, 128), torch.bfloat16) and not ops.fp8_supported(1, 256, 48, ROW, None, torch.float32)
    assert not ops.fp8_supported(1, 256, 48, ROW, None, torch.float16, "float8_e5m2")
    assert lib.gptqhip_fp8_tiled_bytes(4096, 4096) == 4096 * 4096 and lib.gptqhip_fp8_tiled_bytes(100, 16) == 0


def test_every_entry_validates_before_touching_a_device(lib):
    one, odd = ctypes.c_void_p(256), ctypes.c_void_p(260)
    err = lib.gptqhip_last_error
    # gemm
    assert lib.gptqhip_fp8_gemm(None, one, one, None, one, 1, 256, 48, ROW, 0, 0, 0, 0, None) == EINVAL and b"null" in err()
    assert lib.gptqhip_fp8_gemm(one, one, one, odd, one, 1, 256, 48, ROW, 0, 0, 0, 0, None) == EINVAL and b"aligned" in err()
    assert lib.gptqhip_fp8_gemm(one, one, one, None, one, 1, 100, 48, ROW, 0, 0, 0, 0, None) == EINVAL and b"multiple of 128" in err()
    assert lib.gptqhip_fp8_gemm(one, one, one, None, one, 1, 256, 40, ROW, 0, 0, 0, 0, None) == EINVAL and b"multiple of 16" in err()
    assert lib.gptqhip_fp8_gemm(one, one, one, None, one, 1, 256, 48, BLOCK, 16, 64, 0, 0, None) == EINVAL and b"block columns" in err()
    assert lib.gptqhip_fp8_gemm(one, one, one, None, one, 1, 256, 48, BLOCK, 32, 128, 0, 0, None) == EINVAL and b"block rows" in err()
    assert lib.gptqhip_fp8_gemm(one, one, one, None, one, 1, 256, 48, ROW, 0, 0, 2, 0, None) == EINVAL and b"dtype" in err()
    assert lib.gptqhip_fp8_gemm(one, one, one, None, one, 1, 256, 48, ROW, 0, 0, 1, 3, None) == EINVAL and b"flags" in err()   # bit placement x bf16
    assert lib.gptqhip_fp8_gemm(one, one, one, None, one, 1, 256, 48, ROW, 0, 0, 0, 4, None) == EINVAL and b"flags" in err()
    assert lib.gptqhip_fp8_gemm(one, one, one, None, one, -1, 256, 48, ROW, 0, 0, 0, 0, None) == EINVAL
    assert lib.gptqhip_fp8_gemm(None, None, None, None, None, 0, 256, 48, ROW, 0, 0, 0, 0, None) == 0      # empty batch: a no-op success
    # repack
    two = ctypes.c_void_p(512)
    assert lib.gptqhip_fp8_repack(one, one, None, two, 256, 48, ROW, 0, 0, None) == EINVAL and b"null" in err()
    assert lib.gptqhip_fp8_repack(one, one, odd, two, 256, 48, ROW, 0, 0, None) == EINVAL and b"aligned" in err()
    assert lib.gptqhip_fp8_repack(one, one, one, two, 256, 48, ROW, 0, 0, None) == EINVAL and b"in place" in err()
    assert lib.gptqhip_fp8_repack(one, one, two, ctypes.c_void_p(768), 200, 48, ROW, 0, 0, None) == EINVAL and b"multiple of 128" in err()
    # dequant
    assert lib.gptqhip_fp8_dequant(one, None, two, 256, 48, ROW, 0, 0, 0, None) == EINVAL and b"null" in err()
    assert lib.gptqhip_fp8_dequant(one, one, two, 256, 48, ROW, 0, 0, 3, None) == EINVAL and b"dtype" in err()
    assert lib.gptqhip_fp8_dequant(one, one, two, 256, 48, BLOCK, 16, 100, 2, None) == EINVAL and b"block columns" in err()


def test_ops_refuse_cpu_tensors(lib):
    w = torch.zeros((16, 128), dtype=torch.uint8)
    s = torch.ones(16)
    for call in (lambda: ops.fp8_repack(w, s, ROW),
                 lambda: ops.fp8_gemm(torch.zeros((1, 128), dtype=torch.float16), w.reshape(-1), s, None, 16, ROW),
                 lambda: ops.fp8_dequant(w.reshape(-1), s, 128, 16, ROW)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


# ---- selection and the class contract ---------------------------------------------------------------------------------------------------------
def test_enums_and_backend_alias():
    assert FORMAT.FP8.value == "fp8" and METHOD.FP8.value == "fp8" and BACKEND.FP8_HIP.value == "fp8_hip"
    assert normalize_backend("hip", quant_method=METHOD.FP8) is BACKEND.FP8_HIP
    assert normalize_backend("fp8_hip") is BACKEND.FP8_HIP
    assert normalize_backend("hip", quant_method=METHOD.GPTQ) is BACKEND.GPTQ_HIP     # unchanged


def test_selection_resolves_the_class(kernels_available):
    sel = importer.select_quant_linear
    assert sel(8, -1, False, True, device=DEVICE.ROCM, format=FORMAT.FP8, quant_method=METHOD.FP8) is HipFp8Linear
    assert sel(8, -1, False, True, device="cuda:0", backend="hip", format="fp8", quant_method="fp8", pack=True) is HipFp8Linear
    assert sel(8, -1, False, True, device="cuda:0", backend=BACKEND.FP8_HIP, format=FORMAT.FP8, quant_method=METHOD.FP8,
               dtype=torch.bfloat16) is HipFp8Linear
    assert importer.hf_select_quant_linear_v2(8, -1, False, True, format="fp8", quant_method="fp8") is HipFp8Linear
    assert importer.get_kernel_for_backend(BACKEND.HIP, METHOD.FP8, FORMAT.FP8) is HipFp8Linear
    assert importer.AUTO_BACKEND_KERNEL_MAPPING[METHOD.FP8][FORMAT.FP8][BACKEND.FP8_HIP] is HipFp8Linear
    with pytest.raises(NotImplementedError, match="bits"):
        sel(4, -1, False, True, device="cuda:0", format=FORMAT.FP8, quant_method=METHOD.FP8)
    with pytest.raises(NotImplementedError, match="dtype"):
        sel(8, -1, False, True, device="cuda:0", format=FORMAT.FP8, quant_method=METHOD.FP8, dtype=torch.float32)
    with pytest.raises(ValueError, match="Unsupported format"):
        sel(8, -1, False, True, device="cuda:0", format=FORMAT.FP8, quant_method=METHOD.GPTQ)
    # the GPTQ / AWQ selections are what they were
    from gptqmodel_amd.nn_modules.qlinear.hip_gptq import HipGptqLinear
    assert importer.AUTO_BACKEND_KERNEL_MAPPING[METHOD.GPTQ][FORMAT.GPTQ][BACKEND.GPTQ_HIP] is HipGptqLinear


def test_class_contract_and_soft_fail_without_a_gpu():
    HipFp8Linear.verify_supports_params()
    assert HipFp8Linear.SUPPORTS_BITS == [8] and HipFp8Linear.SUPPORTS_DEVICES == [DEVICE.ROCM]
    assert HipFp8Linear.SUPPORTS_DTYPES == [torch.float16, torch.bfloat16] and HipFp8Linear.SUPPORTS_METHODS == [METHOD.FP8]
    assert list(HipFp8Linear.SUPPORTS_FORMATS) == [FORMAT.FP8] and HipFp8Linear.SUPPORTS_BACKENDS == [BACKEND.FP8_HIP]
    assert HipFp8Linear in importer.iter_quant_linear_kernels()
    HipFp8Linear.cached_validate_once.cache_clear()
    if torch.cuda.is_available():
        return
    ok, err = HipFp8Linear.validate_once()
    assert ok is False and isinstance(err, ImportError)
    with pytest.raises(ImportError):
        importer.select_quant_linear(8, -1, False, True, device="cuda", format=FORMAT.FP8, quant_method=METHOD.FP8)
    HipFp8Linear.cached_validate_once.cache_clear()


def test_constructor_declines_what_the_kernels_do_not_serve(kernels_available):
    kw = dict(bits=8, group_size=-1, sym=True, desc_act=False, in_features=256, out_features=64)
    for fmt in ("float8_e5m2", "e5m2", "float8_e4m3fnuz", "float8_e8m0fnu", "e8m0"):
        with pytest.raises(NotImplementedError, match="float8_e4m3fn only"):
            HipFp8Linear(format=fmt, **kw)
    with pytest.raises(ValueError, match="unsupported `format`"):
        HipFp8Linear(format="float7", **kw)
    with pytest.raises(NotImplementedError, match="Unsupported FP8 scale semantics `direct`"):
        HipFp8Linear(weight_scale_semantics="direct", **kw)
    with pytest.raises(ValueError, match="requires `weight_block_size`"):
        HipFp8Linear(weight_scale_method="block", **kw)
    with pytest.raises(ValueError, match="only valid when"):
        HipFp8Linear(weight_scale_method="row", weight_block_size=(32, 128), **kw)
    with pytest.raises(ValueError, match="to be divisible by `weight_block_size"):
        HipFp8Linear(weight_scale_method="block", weight_block_size=(48, 128), **kw)
    with pytest.raises(NotImplementedError, match="multiple of 128"):
        HipFp8Linear(weight_scale_method="block", weight_block_size=(32, 64), **kw)
    with pytest.raises(NotImplementedError, match="in_features"):
        HipFp8Linear(**dict(kw, in_features=192))
    with pytest.raises(NotImplementedError, match="out_features"):
        HipFp8Linear(**dict(kw, out_features=40))
    for fmt in ("float8_e4m3fn", "e4m3", "fp8", FORMAT.FP8, None):
        m = HipFp8Linear(format=fmt, weight_scale_method=None, weight_block_size=[32, 128], **kw)      # block inferred from the block size, like the reference
        assert m.fp8_format == "float8_e4m3fn" and m.weight_scale_method == "block" and m.weight_block_size == (32, 128)
