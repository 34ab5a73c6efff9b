"""CPU tests of the host-side mirror of the reference plugin interface: BACKEND/DEVICE normalisation, kernel
discovery + selection, the validate() contract and its error conventions, act-order permutation, v1->v2 qzeros,
sibling fusion.  Modelled on the reference's tests/kernels/test_selection.py, test_qlinear_hierarchy.py,
test_backend_naming.py, test_qzero_offsets.py, test_triton_g_idx_bounds.py (which monkeypatch device probes the
same way)."""
import numpy as np
import pytest
import torch
import torch.nn as nn

from conftest import load_golden
from gptqmodel_amd.nn_modules.qlinear import AWQuantLinear, BaseQuantLinear, GPTQQuantLinear
from gptqmodel_amd.nn_modules.qlinear.hip_awq import HipAwqLinear
from gptqmodel_amd.nn_modules.qlinear.hip_common import act_order_permutation, check_g_idx
from gptqmodel_amd.nn_modules.qlinear.hip_gptq import HipGptqLinear
from gptqmodel_amd.utils import importer
from gptqmodel_amd.utils.adapter import Lora
from gptqmodel_amd.utils.backend import BACKEND, normalize_backend
from gptqmodel_amd.utils.const import DEVICE, FORMAT, METHOD, normalize_device
from gptqmodel_amd.utils.model import (convert_gptq_v1_to_v2_format_module, fuse_quant_linears, fuse_siblings,
                                       make_quant)
from helpers import synth_gptq
from oracle import gptq_oracle as O


@pytest.fixture
def kernels_available(monkeypatch):
    """Pretend the native library + a gfx950 device are usable (host-logic tests never launch a kernel)."""
    for cls in (HipGptqLinear, HipAwqLinear):
        monkeypatch.setattr(cls, "validate_once", classmethod(lambda c: (True, None)))
        cls.cached_validate_once.cache_clear()
    yield
    for cls in (HipGptqLinear, HipAwqLinear):
        cls.cached_validate_once.cache_clear()


def test_backend_normalisation():
    assert normalize_backend("gptq_hip") is BACKEND.GPTQ_HIP
    assert normalize_backend("GPTQ_HIP") is BACKEND.GPTQ_HIP
    assert normalize_backend("hip", quant_method=METHOD.GPTQ) is BACKEND.GPTQ_HIP
    assert normalize_backend(BACKEND.HIP, quant_method="awq") is BACKEND.AWQ_HIP
    assert normalize_backend(None) is None and normalize_backend("  ") is None
    with pytest.raises(ValueError):
        normalize_backend("no_such_backend")
    with pytest.raises(TypeError):
        normalize_backend(3)


def test_device_normalisation_maps_cuda_to_rocm_on_a_rocm_build():
    assert normalize_device("cuda:0") is DEVICE.ROCM  # torch here is a ROCm build (torch.version.hip set)
    assert normalize_device(torch.device("cuda", 1)) is DEVICE.ROCM
    assert normalize_device(0) is DEVICE.ROCM
    assert normalize_device("cpu") is DEVICE.CPU
    assert DEVICE.ROCM.type == "cuda"


def test_class_contract_is_complete():
    for cls in (HipGptqLinear, HipAwqLinear):
        cls.verify_supports_params()  # every SUPPORTS_* overridden and non-None (qlinear/__init__.py:300-332)
        assert cls.SUPPORTS_DEVICES == [DEVICE.ROCM]
        assert torch.int32 in cls.SUPPORTS_PACK_DTYPES and Lora in cls.SUPPORTS_ADAPTERS
    assert HipGptqLinear.REQUIRES_FORMAT_V2 is True and HipAwqLinear.REQUIRES_FORMAT_V2 is False
    assert issubclass(HipGptqLinear, GPTQQuantLinear) and issubclass(HipAwqLinear, AWQuantLinear)

    class Broken(BaseQuantLinear):
        SUPPORTS_FORMATS = {}
        SUPPORTS_BACKEND_SELECTION = False
    with pytest.raises(ValueError):
        Broken.verify_supports_params()


def test_discovery_and_priority_maps():
    kernels = importer.iter_quant_linear_kernels()
    assert HipGptqLinear in kernels and HipAwqLinear in kernels
    auto = importer.AUTO_BACKEND_KERNEL_MAPPING
    assert auto[METHOD.GPTQ][FORMAT.GPTQ][BACKEND.GPTQ_HIP] is HipGptqLinear
    assert auto[METHOD.GPTQ][FORMAT.GPTQ_V2][BACKEND.GPTQ_HIP] is HipGptqLinear
    assert auto[METHOD.AWQ][FORMAT.GEMM][BACKEND.AWQ_HIP] is HipAwqLinear
    assert importer.get_kernel_for_backend(BACKEND.HIP, METHOD.AWQ, FORMAT.GEMM) is HipAwqLinear
    with pytest.raises(ValueError, match="Unsupported backend"):
        importer.get_kernel_for_backend(BACKEND.TORCH, METHOD.GPTQ, FORMAT.GPTQ)


def test_selection_soft_fails_without_a_gpu():
    """validate_once() returns (False, ImportError) on a box without a usable device, so AUTO raises it
    (upstream: falls through to the next candidate, importer.py:594-598)."""
    for cls in (HipGptqLinear, HipAwqLinear):
        cls.cached_validate_once.cache_clear()
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(ImportError):
        importer.select_quant_linear(4, 128, False, True, device="cuda", backend=BACKEND.AUTO)
    with pytest.raises(ValueError):
        importer.select_quant_linear(4, 128, False, True, device="cuda", backend=BACKEND.GPTQ_HIP)


def test_selection_with_kernels_available(kernels_available):
    sel = importer.select_quant_linear
    assert sel(4, 128, True, False, device="cuda:0") is HipGptqLinear
    assert sel(8, 32, False, True, device=DEVICE.ROCM, backend="hip", format="gptq_v2") is HipGptqLinear
    assert sel(4, 128, False, False, device=DEVICE.ROCM, format=FORMAT.GEMM, quant_method=METHOD.AWQ) is HipAwqLinear
    assert sel(4, 128, False, True, device=DEVICE.ROCM, multi_select=True) == [HipGptqLinear]
    assert importer.hf_select_quant_linear(4, 128, False, True, "gptq", device_map={"": "cuda:0"}) is HipGptqLinear
    with pytest.raises(NotImplementedError):      # unsupported contract under AUTO re-raises the last kernel error
        sel(4, 48, False, True, device=DEVICE.ROCM)
    with pytest.raises(ValueError):               # explicit backend: hard error
        sel(4, 48, False, True, device=DEVICE.ROCM, backend=BACKEND.GPTQ_HIP)
    for bits in (2, 3, 5, 6, 7):                  # the other bit widths of the reference's torch kernel
        assert sel(bits, 128, False, True, device=DEVICE.ROCM) is HipGptqLinear
        # FORMAT.GPTQ_P (split-plane words): what the reference's config declares for 5 / 6 / 7 bits (config.py:2660-2676)
        assert sel(bits, 128, False, True, device=DEVICE.ROCM, format=FORMAT.GPTQ_P) is HipGptqLinear
    assert importer.hf_select_quant_linear(5, 128, False, True, "gptq_p", device_map={"": "cuda:0"}) is HipGptqLinear
    # planar routing like the reference's constructor (qlinear/__init__.py:766-773): 5 / 6 / 7 always, 3 under gptq_p only,
    # 2 / 4 / 8-bit planar words are bit-identical to the continuous ones
    mk = lambda bits, fmt: HipGptqLinear(bits=bits, group_size=128, sym=True, desc_act=False, in_features=256, out_features=64, format=fmt,
                                         register_buffers=False)
    assert [mk(b, FORMAT.GPTQ_P).planar for b in (2, 3, 4, 5, 8)] == [False, True, False, True, False]
    assert [mk(b, FORMAT.GPTQ_V2).planar for b in (3, 6)] == [False, True]
    with pytest.raises((ValueError, NotImplementedError)):   # CPU device is filtered out (SUPPORTS_DEVICES=[ROCM])
        sel(4, 128, False, True, device="cpu")
    with pytest.raises(ValueError, match="Unsupported format"):
        sel(4, 128, False, True, device=DEVICE.ROCM, format=FORMAT.GEMM)  # AWQ layout under METHOD.GPTQ
    assert sel(4, 128, False, True, device=DEVICE.ROCM, pack=True) is HipGptqLinear   # device packer (pack_block)
    with pytest.raises(ValueError):                                                  # the AWQ class cannot pack
        sel(4, 128, False, False, device=DEVICE.ROCM, format=FORMAT.GEMM, quant_method=METHOD.AWQ, pack=True)


@pytest.mark.parametrize("kw,ok", [
    (dict(bits=4, group_size=128, in_features=4096, out_features=4096), True),
    (dict(bits=8, group_size=-1, in_features=256, out_features=64), True),
    (dict(bits=4, group_size=128, in_features=4096, out_features=4100), False),   # N % 8
    (dict(bits=4, group_size=128, in_features=4100, out_features=4096), False),   # K % 32
    (dict(bits=4, group_size=48, in_features=96, out_features=64), False),        # group size not listed
    (dict(bits=2, group_size=128, in_features=4096, out_features=4096), True),     # widened to 4-bit fields at post_init
    (dict(bits=3, group_size=128, in_features=4096, out_features=4096), True),
    (dict(bits=6, group_size=64, in_features=4096, out_features=4096), True),      # planar, widened to 8-bit fields
    (dict(bits=1, group_size=128, in_features=4096, out_features=4096), False),
    (dict(bits=4, group_size=128, in_features=4096, out_features=4096, dtype=torch.float32), False),
    (dict(bits=4, group_size=128, in_features=4096, out_features=4096, pack_dtype=torch.int16), False),
    (dict(bits=4, group_size=128, in_features=4096, out_features=4096, trainable=True), False),
    (dict(bits=4, group_size=128, in_features=4096, out_features=4096, device=DEVICE.CPU), False),
    (dict(bits=4, group_size=128, in_features=4096, out_features=4096, dynamic={"x": {"bits": 9}}), False),
])
def test_validate_contract(kernels_available, kw, ok):
    kw.setdefault("pack_dtype", torch.int32)
    got, err = HipGptqLinear.validate(desc_act=False, sym=True, **kw)
    assert got is ok
    assert (err is None) if ok else isinstance(err, NotImplementedError)


def test_constructor_registers_checkpoint_buffers(kernels_available):
    lin = HipGptqLinear(bits=4, group_size=128, sym=True, desc_act=False, in_features=512, out_features=256, bias=True)
    sd = lin.state_dict()
    assert {k: tuple(v.shape) for k, v in sd.items()} == {
        "qweight": (64, 256), "qzeros": (4, 32), "scales": (4, 256), "g_idx": (512,), "bias": (256,)}
    assert sd["qweight"].dtype == torch.int32 and sd["scales"].dtype == torch.float16
    awq = HipAwqLinear(bits=4, group_size=128, sym=False, desc_act=False, in_features=512, out_features=256)
    assert {k: tuple(v.shape) for k, v in awq.state_dict().items()} == {
        "qweight": (512, 32), "qzeros": (4, 32), "scales": (4, 256)}
    for bits in (2, 3, 5, 6, 7):                    # checkpoint shapes of the other bit widths (qlinear/__init__.py:595-660)
        o = HipGptqLinear(bits=bits, group_size=128, sym=True, desc_act=False, in_features=512, out_features=256)
        assert (tuple(o.qweight.shape), tuple(o.qzeros.shape)) == ((512 * bits // 32, 256), (4, 256 * bits // 32))
        assert (o.kernel_bits, o.planar) == (4 if bits < 4 else 8, bits in (5, 6, 7))
    with pytest.raises(NotImplementedError):
        HipGptqLinear(bits=1, group_size=128, sym=True, desc_act=False, in_features=512, out_features=256)
    for bits in (2, 3, 6):                          # the other widths work on blocks of 32 codes: features in multiples of 32
        with pytest.raises(NotImplementedError):
            HipGptqLinear(bits=bits, group_size=128, sym=True, desc_act=False, in_features=512, out_features=264)
    HipGptqLinear(bits=4, group_size=128, sym=True, desc_act=False, in_features=512, out_features=264)      # 4 / 8 bits: N % 8
    with pytest.raises(RuntimeError):
        lin(torch.zeros(1, 512, dtype=torch.float16))  # forward before post_init
    with pytest.raises(RuntimeError):
        lin.post_init()  # CPU buffers: loud, no fallback


def test_make_quant_swaps_linears(kernels_available):
    class Block(nn.Module):
        def __init__(self):
            super().__init__()
            self.q_proj = nn.Linear(256, 128, bias=False)
            self.keep = nn.Linear(256, 8)
            self.norm = nn.LayerNorm(256)
    m = nn.ModuleDict({"layer": Block()})
    picked = make_quant(m, ["layer.q_proj"], bits=4, group_size=64, desc_act=False, sym=True)
    assert picked == [HipGptqLinear]
    assert isinstance(m["layer"].q_proj, HipGptqLinear) and isinstance(m["layer"].keep, nn.Linear)
    assert m["layer"].q_proj.name == "layer.q_proj"
    with pytest.raises(ValueError):
        make_quant(m, ["layer.norm"], bits=4, group_size=64, desc_act=False, sym=True)


def test_make_quant_dynamic_overrides(kernels_available):
    """QuantizeConfig.dynamic semantics (quantization/config.py:1614-1652; utils/model.py:545-564): first matching pattern
    in dict order wins, "-:" excludes the module, "+:" / plain patterns override bits / group_size / desc_act / sym."""
    from gptqmodel_amd.utils.model import dynamic_get

    class Block(nn.Module):
        def __init__(self):
            super().__init__()
            self.q_proj = nn.Linear(256, 128, bias=False)
            self.k_proj = nn.Linear(256, 128, bias=False)
            self.down_proj = nn.Linear(256, 256, bias=False)
    m = nn.ModuleDict({"layers": nn.ModuleList([Block(), Block()])})
    dynamic = {r"-:layers\.0\.k_proj": {}, r"+:.*down_proj": {"bits": 8, "group_size": 32}, r"layers\.1\..*": {"desc_act": True}}
    assert dynamic_get(dynamic, "layers.0.k_proj") is False
    assert dynamic_get(dynamic, "layers.1.down_proj") == {"bits": 8, "group_size": 32}   # earlier pattern wins
    assert dynamic_get(dynamic, "layers.1.q_proj") == {"desc_act": True}
    assert dynamic_get(dynamic, "layers.0.q_proj") is None and dynamic_get(None, "x") is None
    names = [n for n, mod in m.named_modules() if isinstance(mod, nn.Linear)]
    make_quant(m, names, bits=4, group_size=128, desc_act=False, sym=True, dynamic=dynamic)
    l0, l1 = m["layers"][0], m["layers"][1]
    assert isinstance(l0.k_proj, nn.Linear) and not isinstance(l0.k_proj, HipGptqLinear)
    assert (l0.q_proj.bits, l0.q_proj.group_size, l0.q_proj.desc_act) == (4, 128, False)
    assert (l0.down_proj.bits, l0.down_proj.group_size) == (8, 32)
    assert (l1.q_proj.bits, l1.q_proj.desc_act) == (4, True) and (l1.down_proj.bits, l1.down_proj.desc_act) == (8, False)


def test_act_order_permutation_and_bounds():
    gs, k = 4, 16
    seq = torch.arange(k, dtype=torch.int32) // gs
    assert act_order_permutation(seq, gs, 4) is None
    perm0 = torch.randperm(k, generator=torch.Generator().manual_seed(0))
    g_idx = (perm0 // gs).to(torch.int32)
    perm = act_order_permutation(g_idx, gs, 4)
    assert perm.dtype == torch.int32
    assert torch.equal(g_idx[perm.long()].long(), torch.arange(k) // gs)
    assert np.array_equal(perm.numpy(), O.act_order_perm(g_idx.numpy()))  # same stable order as the oracle
    # negative indices wrap like torch indexing; out-of-range is rejected before any kernel trusts it
    assert torch.equal(check_g_idx(torch.tensor([-1, 0, -4, 3]), 4), torch.tensor([3, 0, 0, 3]))
    with pytest.raises(ValueError):
        check_g_idx(torch.tensor([0, 4]), 4)
    with pytest.raises(ValueError):
        check_g_idx(torch.tensor([-5, 0]), 4)
    with pytest.raises(NotImplementedError):  # unbalanced groups cannot be row-sorted into fixed-size groups
        act_order_permutation(torch.tensor([0, 0, 0, 0, 0, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3], dtype=torch.int32), gs, 4)


def test_v1_to_v2_qzeros(kernels_available):
    g = load_golden("ref_v1v2.npz")
    for bits in (4, 8):
        lin = HipGptqLinear(bits=bits, group_size=32, sym=False, desc_act=False, in_features=64, out_features=64)
        lin.qzeros = torch.from_numpy(g[f"v1_{bits}"].copy())
        assert lin.qzero_format() == 1
        convert_gptq_v1_to_v2_format_module(lin, bits=bits)
        assert lin.qzero_format() == 2
        assert np.array_equal(lin.qzeros.numpy(), g[f"v2_{bits}"])


def test_fuse_quant_linears_concatenates_along_n(kernels_available):
    K, gs = 256, 64
    mods, parts = [], []
    for i, n in enumerate((64, 32, 32)):
        qweight, qzeros, scales, g_idx = synth_gptq(50 + i, 4, K, n, gs)
        lin = HipGptqLinear(bits=4, group_size=gs, sym=False, desc_act=False, in_features=K, out_features=n, name=f"p{i}")
        lin.qweight, lin.qzeros = torch.from_numpy(qweight), torch.from_numpy(qzeros)
        lin.scales, lin.g_idx = torch.from_numpy(scales).half(), torch.from_numpy(g_idx)
        mods.append(lin)
        parts.append(O.dequant_gptq(qweight, qzeros, scales, g_idx, 4))
    fused = fuse_quant_linears(mods)
    assert fused.out_features == 128 and fused.qweight.shape == (K // 8, 128) and fused.qzeros.shape == (K // gs, 16)
    w = O.dequant_gptq(fused.qweight.numpy(), fused.qzeros.numpy(), fused.scales.float().numpy(), fused.g_idx.numpy(), 4)
    assert np.array_equal(w, np.concatenate(parts, axis=1))
    # act-order siblings with different permutations are left alone
    mods[1].g_idx = torch.from_numpy((np.random.RandomState(0).permutation(K) // gs).astype(np.int32))
    with pytest.raises(NotImplementedError):
        fuse_quant_linears(mods)
    blk = nn.Module()
    blk.a, blk.b = mods[0], mods[1]
    assert fuse_siblings(blk, ["a", "b"]) is None and blk.a is mods[0]


def test_hf_entry_points(kernels_available):
    """The HF/optimum-facing wrappers (upstream importer.py:377-470, utils/model.py:730-748, 1276)."""
    from gptqmodel_amd.utils.importer import hf_select_quant_linear_v2
    from gptqmodel_amd.utils.model import hf_convert_gptq_v1_to_v2_format, hf_gptqmodel_post_init
    from gptqmodel_amd.nn_modules.qlinear.hip_awq import HipAwqLinear
    assert hf_select_quant_linear_v2(4, 128, False, True, "gptq", "gptq", dtype="torch.float16") is HipGptqLinear
    assert hf_select_quant_linear_v2(4, 128, False, True, "gemm", "awq", zero_point=True) is HipAwqLinear
    with pytest.raises(ValueError):
        hf_select_quant_linear_v2(4, 128, False, True, "nope", "gptq")
    m = nn.ModuleDict({"a": nn.Linear(64, 32, bias=False)})
    make_quant(m, ["a"], bits=4, group_size=32, desc_act=False, sym=True)
    m["a"].qzeros.data.fill_(0x77777777)
    _, converted = hf_convert_gptq_v1_to_v2_format(m, bits=4, checkpoint_format="gptq")
    assert converted and int(m["a"].qzeros[0, 0]) == -0x77777778 and m["a"].qzero_format() == 2   # 0x88888888 as int32
    _, again = hf_convert_gptq_v1_to_v2_format(m, bits=4, checkpoint_format="gptq_v2")
    assert not again
    assert callable(hf_gptqmodel_post_init)


def test_autotune_hook_contract(kernels_available):
    """maybe_autotune (qlinear/__init__.py:246-255): off by default; once enabled, `_autotune` runs once, never in
    training mode, and clear_autotune() (called by post_init) drops the cached result."""
    calls = []
    lin = HipGptqLinear(bits=4, group_size=32, sym=True, desc_act=False, in_features=64, out_features=32, bias=False)
    assert lin.maybe_autotune(1) is None and lin.get_autotune_result() is None
    with pytest.raises(NotImplementedError):
        lin._autotune(1)
    lin.eval()
    lin.autotune_enabled = True
    lin._autotune = lambda x: (calls.append(x), {"plan": len(calls)})[1]
    assert lin.maybe_autotune("a") == {"plan": 1} and lin.maybe_autotune("b") == {"plan": 1} and calls == ["a"]
    lin.clear_autotune()
    assert lin.maybe_autotune("c") == {"plan": 2}


def test_rotation_hook_fails_loudly(kernels_available):
    lin = HipGptqLinear(bits=4, group_size=32, sym=True, desc_act=False, in_features=64, out_features=32, bias=False)
    x = torch.zeros(2, 64)
    assert lin._apply_rotation_to_input(x) is x
    lin.set_had_K(torch.eye(4))
    assert "had_K" in dict(lin.named_buffers())
    lin.set_had_K(None)
    assert lin.had_K is None
    lin.online_full_had = True
    with pytest.raises(NotImplementedError, match="Hadamard"):
        lin._apply_rotation_to_input(x)


def test_env_switches(monkeypatch):
    """GPTQHIP_DISABLE makes validate_once() report the kernels unavailable (AUTO then falls through, like a missing
    .so); the tuning variables must be integers."""
    from gptqmodel_amd import _lib
    from gptqmodel_amd.nn_modules.qlinear.hip_common import hip_validate_once
    monkeypatch.setenv("GPTQHIP_DISABLE", "1")
    ok, err = hip_validate_once()
    assert ok is False and isinstance(err, ImportError) and "GPTQHIP_DISABLE" in str(err)


def test_tuning_overrides_are_thread_local():
    """gptqhip_set_tuning must not leak across threads (the header promises re-entrancy across threads, devices and
    streams): a forced cross-block split-K on one thread changes that thread's workspace plan only."""
    import threading
    from gptqmodel_amd import _lib
    lib = _lib.load()
    args = (4, 4096, 512, 128, 4, 0)
    base = lib.gptqhip_workspace_bytes(*args)
    seen = {}

    def worker():
        lib.gptqhip_set_tuning(8, 0, 0)
        seen["forced"] = lib.gptqhip_workspace_bytes(*args)

    t = threading.Thread(target=worker)
    t.start()
    t.join()
    assert seen["forced"] > base                       # 8 fp32 slabs planned on the worker thread
    assert lib.gptqhip_workspace_bytes(*args) == base  # this thread never saw the override


def test_fused_group_cache_never_serves_a_stale_input():
    """the fused-output cache must be keyed on the identity of a LIVE input tensor.  Fresh
    activations created in a decode loop reuse Python ids / allocator addresses of dead ones; every view call must still
    see the result for ITS input, also under torch.inference_mode() (no version counter) and after in-place updates."""
    from gptqmodel_amd.utils.model import FusedSiblingView, _FusedGroup

    class Lin(torch.nn.Module):
        calls = 0

        def forward(self, x):
            Lin.calls += 1
            return torch.cat([x * 2.0, x * 3.0, x * 5.0], dim=-1)

    h = 64
    group = _FusedGroup(Lin(), [h, h, h])
    views = [FusedSiblingView(group, i, h, h) for i in range(3)]
    mult = [2.0, 3.0, 5.0]
    for mode in (torch.no_grad, torch.inference_mode):
        with mode():
            for step in range(400):
                x = torch.full((1, h), float(step % 97) + 1.0)     # a fresh tensor per step: ids / addresses recycle
                x = torch.nn.functional.rms_norm(x + step, (h,))
                for i in (0, 1, 2) if step % 2 else (2, 0, 1):
                    assert torch.equal(views[i](x), x * mult[i]), (step, i)
    assert group._x is None and group._out is None                 # nothing pinned once every sibling was served
    Lin.calls = 0
    x = torch.ones(1, h)
    a = views[0](x)
    x.add_(1.0)                                                     # in-place update bumps the version: recompute
    b = views[1](x)
    assert Lin.calls == 2 and torch.equal(a, torch.full((1, h), 2.0)) and torch.equal(b, torch.full((1, h), 6.0))
    views[2](x)
    c = views[2](x)                                                 # same sibling asked twice: recomputed, not stale
    assert torch.equal(c, x * 5.0)


def test_fused_module_tensors_are_registered_buffers(kernels_available):
    """the fused module's tensors must be buffers so .to() / list_buffers() reach them."""
    from gptqmodel_amd.nn_modules.qlinear.hip_gptq import HipGptqLinear
    from gptqmodel_amd.utils.const import FORMAT
    from gptqmodel_amd.utils.model import fuse_quant_linears
    mods = [HipGptqLinear(bits=4, group_size=128, sym=True, desc_act=False, in_features=256, out_features=n, bias=True,
                          register_buffers=True, format=FORMAT.GPTQ_V2) for n in (64, 32)]
    fused = fuse_quant_linears(mods)
    names = dict(fused.named_buffers())
    assert {"qweight", "qzeros", "scales", "g_idx", "bias"} <= set(names)
    assert names["qweight"].shape == (32, 96) and names["bias"].shape == (96,)
    assert len(fused.list_buffers()) == 5 and fused.format == FORMAT.GPTQ_V2
    assert "meta" not in fused.state_dict() and "perm" not in fused.state_dict()   # derived tensors are non-persistent
    assert all(t is not None for t in fused._buffers.values())   # no None-valued buffers (accelerate offload hooks)


def test_interleave_cols_owns_its_storage():
    """post_init replaces `qweight.data`; a view result would keep its base (a second copy of the packed weights) alive."""
    from gptqmodel_amd.utils.model import _interleave_cols
    a, b = torch.arange(32, dtype=torch.int32).reshape(2, 16), 100 + torch.arange(32, dtype=torch.int32).reshape(2, 16)
    out = _interleave_cols(a, b, 8)
    assert out._base is None and out.is_contiguous()
    assert out[0].tolist() == list(range(0, 8)) + list(range(100, 108)) + list(range(8, 16)) + list(range(108, 116))


def test_fold_act_order_into_producers_is_exact(kernels_available):
    """down_proj's act-order input permutation folded into gate / up output columns: only integer codes move, so the
    dequantised matrices are the permuted originals bit for bit, the consumer's g_idx becomes sequential, and the composite
    y = (g(x) * u(x)) @ W_down is unchanged (checked on the dequantised matrices in float64)."""
    import numpy as np
    from helpers import synth_gptq
    from oracle import gptq_oracle as O
    from gptqmodel_amd.nn_modules.qlinear.hip_gptq import HipGptqLinear
    from gptqmodel_amd.utils.model import fold_act_order_into_producers
    for bits in (4, 8):
        hidden, inter, gs = 128, 192, 32

        def mod(seed, k, n, desc):
            qweight, qzeros, scales, g_idx = synth_gptq(seed, bits, k, n, gs, desc_act=desc)
            m = HipGptqLinear(bits=bits, group_size=gs, sym=False, desc_act=desc, in_features=k, out_features=n, bias=True,
                              register_buffers=True)
            m.load_state_dict({"qweight": torch.from_numpy(qweight), "qzeros": torch.from_numpy(qzeros),
                               "scales": torch.from_numpy(scales).half(), "g_idx": torch.from_numpy(g_idx),
                               "bias": (torch.arange(n).float() * 0.01 + seed).half()})
            return m, O.dequant_gptq(qweight, qzeros, scales, g_idx, bits), g_idx

        gate, w_gate, _ = mod(11, hidden, inter, True)
        up, w_up, _ = mod(12, hidden, inter, True)
        down, w_down, g_down = mod(13, inter, hidden, True)
        b_gate = gate.bias.clone()
        perm = np.argsort(g_down.astype(np.int64), kind="stable")
        assert fold_act_order_into_producers(down, [gate, up])
        deq = lambda m: O.dequant_gptq(m.qweight.numpy(), m.qzeros.numpy(), m.scales.float().numpy(), m.g_idx.numpy(), bits)
        assert np.array_equal(deq(down), w_down[perm])
        assert np.array_equal(deq(gate), w_gate[:, perm]) and np.array_equal(deq(up), w_up[:, perm])
        assert np.array_equal(down.g_idx.numpy(), np.arange(inter) // gs)
        assert torch.equal(gate.bias, b_gate[torch.from_numpy(perm)])
        x = np.random.RandomState(0).randn(3, hidden)
        before = ((x @ w_gate.astype(np.float64)) * (x @ w_up.astype(np.float64))) @ w_down.astype(np.float64)
        after = ((x @ deq(gate).astype(np.float64)) * (x @ deq(up).astype(np.float64))) @ deq(down).astype(np.float64)
        assert np.allclose(before, after, rtol=1e-12, atol=1e-9)
        assert not fold_act_order_into_producers(down, [gate, up])      # nothing left to fold


def test_gate_up_interleaved_fusion_layout(kernels_available):
    """fuse_gate_up_interleaved: output columns alternate in blocks of 8 (g0..7 u0..7 g8..15 ...) on the CHECKPOINT tensors
    (whole packed words move); the dequantised fused matrix is the column-interleave of the two, deinterleave undoes it."""
    import numpy as np
    from helpers import synth_gptq
    from oracle import gptq_oracle as O
    from gptqmodel_amd.nn_modules.qlinear.hip_gptq import HipGptqLinear
    from gptqmodel_amd.utils.model import deinterleave_gate_up, fuse_gate_up_interleaved
    for bits in (4, 8):
        K, N, gs = 256, 48, 64
        mods, dense = [], []
        for seed in (1, 2):
            qweight, qzeros, scales, g_idx = synth_gptq(seed, bits, K, N, gs)
            m = HipGptqLinear(bits=bits, group_size=gs, sym=False, desc_act=False, in_features=K, out_features=N, bias=True,
                              register_buffers=True)
            m.load_state_dict({"qweight": torch.from_numpy(qweight), "qzeros": torch.from_numpy(qzeros),
                               "scales": torch.from_numpy(scales).half(), "g_idx": torch.from_numpy(g_idx),
                               "bias": torch.arange(N).half() + 100 * seed})
            mods.append(m)
            dense.append(O.dequant_gptq(qweight, qzeros, scales, g_idx, bits))
        f = fuse_gate_up_interleaved(*mods)
        assert f.out_features == 2 * N and f.gate_up_interleaved and set(dict(f.named_buffers())) >= {"qweight", "qzeros", "scales", "bias"}
        w = O.dequant_gptq(f.qweight.numpy(), f.qzeros.numpy(), f.scales.float().numpy(), f.g_idx.numpy(), bits)
        g, u = deinterleave_gate_up(torch.from_numpy(w))
        assert np.array_equal(g.numpy(), dense[0]) and np.array_equal(u.numpy(), dense[1])
        assert np.array_equal(w[:, :8], dense[0][:, :8]) and np.array_equal(w[:, 8:16], dense[1][:, :8])
        bg, bu = deinterleave_gate_up(f.bias[None])
        assert torch.equal(bg[0], mods[0].bias) and torch.equal(bu[0], mods[1].bias)


def test_bench_gpus_flag_is_honoured_self_spawn_and_mismatch():
    """`python bench.py --gpus N` (the driver's recorded command form, no torchrun) must itself become N ranks: the launch decision is
    a pure function (bench.spawn_command), and the real thing is exercised end to end through --handshake-only (rendezvous on
    127.0.0.1 + an all-reduce of ones; gloo here, RCCL on a GPU node): ONE JSON line with n_gpus == ranks_seen == N.  Under a foreign
    launcher a WORLD_SIZE that disagrees with --gpus is an error, not a silent one-GPU run (VERDICT r2 missing #1)."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    sys.path.insert(0, root)
    import bench
    assert bench.spawn_command(1, {}, ["--gpus", "1"]) is None
    assert bench.spawn_command(4, {"WORLD_SIZE": "4"}, ["--gpus", "4"]) is None            # already a rank
    cmd = bench.spawn_command(4, {}, ["--gpus", "4", "--steps", "7"])
    assert cmd[1:3] == ["-m", "torch.distributed.run"] and "--nproc-per-node=4" in cmd and "--nnodes=1" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and cmd[-4:] == ["--gpus", "4", "--steps", "7"]
    assert os.path.basename(cmd[cmd.index("--master-port") + 2]) == "bench.py"
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env["CUDA_VISIBLE_DEVICES"] = env["HIP_VISIBLE_DEVICES"] = ""
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--handshake-only"], capture_output=True, text=True,
                       timeout=240, env=env, cwd=root)
    lines = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert r.returncode == 0 and len(lines) == 1, (r.returncode, r.stdout[-500:], r.stderr[-500:])
    assert lines[0]["n_gpus"] == 2 and lines[0]["ranks_seen"] == 2
    bad = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--handshake-only"], capture_output=True, text=True,
                         timeout=120, env=dict(env, WORLD_SIZE="3", RANK="0"), cwd=root)
    assert bad.returncode != 0 and "WORLD_SIZE=3" in (bad.stderr + bad.stdout)


def test_quantize_config_normalisation_and_v1_zero_points():
    """utils.checkpoint: the quantize_config key handling of the reference (quantization/config.py:1504-1525: w_bit / wbits /
    q_group_size / version / checkpoint_format / quant_method synonyms, AWQ zero_point = NOT sym, is_marlin_format rejected; lookup
    order quantize_config.json > quant_config.json > config.json[quantization_config], :3022-3043) and the v2 -> v1 zero-point
    conversion the writer applies (inverse of convert_gptq_v1_to_v2_format_module)."""
    import json
    import tempfile
    from gptqmodel_amd.utils import checkpoint as C
    from gptqmodel_amd.utils.model import _V1_TO_V2_ADD
    n = C.normalize_quantize_config({"w_bit": 4, "q_group_size": 64, "zero_point": True, "version": "GEMM", "quant_method": "awq"})
    assert (n["bits"], n["group_size"], n["sym"], n["format"], n["method"]) == (4, 64, False, "gemm", "awq")
    n = C.normalize_quantize_config({"bits": 8, "checkpoint_format": "gptq_v2", "desc_act": True, "dynamic": {"-:lm_head": {}}})
    assert (n["bits"], n["group_size"], n["desc_act"], n["sym"], n["format"], n["method"]) == (8, 128, True, True, "gptq_v2", "gptq")
    assert n["dynamic"] == {"-:lm_head": {}} and n["pack_dtype"] == "int32"
    with pytest.raises(ValueError):
        C.normalize_quantize_config({"bits": 4, "is_marlin_format": True})
    assert C.normalize_quantize_config({"bits": 5, "checkpoint_format": "gptq_p"})["format"] == "gptq_p"
    with pytest.raises(ValueError):
        C.normalize_quantize_config({"bits": 9})
    with pytest.raises(ValueError):
        C.normalize_quantize_config({"bits": 3, "quant_method": "awq"})
    with tempfile.TemporaryDirectory() as d:
        with pytest.raises(ValueError):
            C.read_quantize_config(d)
        with open(f"{d}/config.json", "w") as f:
            json.dump({"hidden_size": 8, "quantization_config": {"bits": 4, "group_size": 32, "quant_method": "gptq"}}, f)
        assert C.read_quantize_config(d)["group_size"] == 32
        with open(f"{d}/quantize_config.json", "w") as f:
            json.dump({"bits": 4, "group_size": 128, "sym": False}, f)
        assert C.read_quantize_config(d)["group_size"] == 128 and C.read_quantize_config(d)["sym"] is False
    for bits in (4, 8):
        z = torch.randint(-2**31, 2**31 - 1, (5, 7), dtype=torch.int32)
        v1 = C._v2_to_v1_qzeros(z, bits)
        add = _V1_TO_V2_ADD[bits]
        add = add - 2**32 if add >= 2**31 else add
        back = v1 + add                      # int32 wraparound add, what convert_gptq_v1_to_v2_format_module does
        mask = (1 << bits) - 1
        sh = torch.arange(0, 32, bits)
        fields = lambda t: (t.long().unsqueeze(-1) >> sh) & mask
        # field-wise equality modulo 2^bits except where the word-level add carried across a field that held 0 (zero - 1 wraps to
        # maxq on disk; the reference's word add then carries) -- real zero-points are >= 1 after +1, so restrict to those
        ok = fields(z) != 0
        assert torch.equal(fields(back)[ok.all(dim=-1)], fields(z)[ok.all(dim=-1)])
    assert C.quantized_module_names(["a.b.qweight", "a.b.scales", "c.weight", "d.qweight"]) == ["a.b", "d"]
    # the other bit widths go through the decoded values (3-bit fields straddle words, 5 / 6 / 7 bits are planar: ADVICE r3)
    import numpy as np
    from conftest import load_golden
    from gptqmodel_amd.utils.model import shift_v1_qzeros
    g = load_golden("ref_v1v2_bits.npz")             # written by the reference's convert_gptq_v1_to_v2_format_module
    for bits in (2, 3, 5, 6, 7):
        assert C.normalize_quantize_config({"bits": bits})["bits"] == bits
        v1, v2 = torch.from_numpy(g[f"v1_{bits}"]), torch.from_numpy(g[f"v2_{bits}"])
        assert torch.equal(shift_v1_qzeros(v1, bits), v2)
        assert torch.equal(C._v2_to_v1_qzeros(v2, bits), v1)
    g = load_golden("ref_v1v2.npz")
    for bits in (4, 8):
        assert torch.equal(shift_v1_qzeros(torch.from_numpy(g[f"v1_{bits}"]), bits), torch.from_numpy(g[f"v2_{bits}"]))
    # the reference's guard for asymmetric v1 files (models/loader.py:1658-1663; quantization/config.py:2786-2792)
    assert C._written_by_v2_aware_quantizer({"meta": {"quantizer": ["gptqmodel:1.4.2"]}})
    assert C._written_by_v2_aware_quantizer({"meta": {"quantizer": "gptqmodel:0.9.0"}})
    assert not C._written_by_v2_aware_quantizer({"meta": {"quantizer": ["gptqmodel:0.8.1"]}})
    assert not C._written_by_v2_aware_quantizer({"meta": {"quantizer": ["auto_gptq:0.7.1"]}})
    assert not C._written_by_v2_aware_quantizer({"meta": {}})


def test_product_package_never_touches_the_oracle_or_the_reference():
    """The oracle (and the reference snapshot under oracle/_ref) is test / measurement infrastructure: nothing under gptqmodel_amd/
    imports it, executes it or reads /root/reference; a product path that routed through it would void every parity claim."""
    import os
    import re
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gptqmodel_amd")
    pat = re.compile(r"^\s*(from\s+oracle[\s.]|import\s+oracle\b|from\s+gptqmodel\b(?!_amd)|import\s+gptqmodel\b(?!_amd))|/root/reference|oracle/_ref|ref_import")
    hits = []
    for dp, _, fns in os.walk(root):
        for fn in fns:
            if fn.endswith((".py", ".hip", ".h")):
                with open(os.path.join(dp, fn), encoding="utf-8") as f:
                    for i, line in enumerate(f, 1):
                        if pat.search(line):
                            hits.append(f"{os.path.relpath(os.path.join(dp, fn), root)}:{i}: {line.strip()}")
    assert not hits, hits


def test_reference_snapshot_recipe_lists_what_the_shim_executes():
    """oracle/make_ref_snapshot.py (run by __graft_entry__.build() when /root/reference is mounted): the snapshot holds the reference's
    TorchLinear / AwqTorchLinear sources, is git-ignored, and the import shim falls back to it."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    snap = os.path.join(root, "oracle", "_ref")
    if not os.path.isdir(snap):
        pytest.skip("no oracle/_ref snapshot on this box (it is made where /root/reference is mounted)")
    for rel in ("gptqmodel/nn_modules/qlinear/torch.py", "gptqmodel/nn_modules/qlinear/torch_awq.py", "SNAPSHOT.txt"):
        assert os.path.isfile(os.path.join(snap, rel)), rel
    # the repository's own .gitignore keeps it out (read directly: a checkout exported without .git must pass this too) ...
    with open(os.path.join(root, ".gitignore")) as f:
        rules = {ln.strip() for ln in f}
    assert rules & {"oracle/_ref/", "/oracle/_ref/", "oracle/_ref", "/oracle/_ref"}, "oracle/_ref must stay out of the history"
    # ... and, where the checkout is itself a git work tree that git will read, git agrees
    top = subprocess.run(["git", "rev-parse", "--show-toplevel"], cwd=root, capture_output=True, text=True)
    if top.returncode == 0 and os.path.realpath(top.stdout.strip()) == os.path.realpath(root):
        ign = subprocess.run(["git", "check-ignore", "-q", "oracle/_ref/SNAPSHOT.txt"], cwd=root)
        assert ign.returncode == 0, "oracle/_ref must stay out of the history"
    code = ("import os, sys; sys.path.insert(0, %r); os.environ['GPTQ_REFERENCE_ROOT'] = %r\n"
            "from oracle.ref_import import load_reference, REF_IS_SNAPSHOT\n"
            "r = load_reference(); assert REF_IS_SNAPSHOT and r.TorchLinear.__module__ == 'gptqmodel.nn_modules.qlinear.torch'\n" % (root, snap))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-800:]


def test_qzero_offsets_like_the_reference_tests():
    """The reference's tests/test_qzero_offsets.py restated against this package's conversions (int32 words, the only pack dtype of
    the HIP classes): round trip (:145), scalar patterns (:189), the 3-bit canonical pack order (:203), and the module's own width
    winning over the checkpoint-level one (:165)."""
    import types
    from gptqmodel_amd.utils.model import convert_gptq_v1_to_v2_format, shift_v1_qzeros, unshift_v2_qzeros
    gen = torch.Generator().manual_seed(3)
    for bits in (2, 3, 4, 5, 6, 7, 8):
        z = torch.randint(-2**31, 2**31 - 1, (3, 2 * bits), dtype=torch.int32, generator=gen)
        assert torch.equal(unshift_v2_qzeros(shift_v1_qzeros(z, bits), bits), z)
        assert torch.equal(shift_v1_qzeros(unshift_v2_qzeros(z, bits), bits), z)
    zero = torch.zeros((1, 1), dtype=torch.int32)
    for bits, want in ((2, 0x55555555), (4, 0x11111111), (8, 0x01010101)):
        assert int(shift_v1_qzeros(zero, bits).item()) & 0xFFFFFFFF == want
    # 3 bits: thirty-two ones in the canonical continuous order (code i at bit 3 i of the 96-bit stream)
    stream = sum(1 << (3 * i) for i in range(32))
    want = torch.tensor([[(stream >> (32 * w)) & 0xFFFFFFFF for w in range(3)]], dtype=torch.int64)
    got = shift_v1_qzeros(torch.zeros((1, 3), dtype=torch.int32), 3).to(torch.int64) & 0xFFFFFFFF
    assert torch.equal(got, want)
    # a 4-bit module inside a checkpoint whose config says 3 bits is converted at ITS width
    mod = HipGptqLinear.__new__(HipGptqLinear)
    torch.nn.Module.__init__(mod)
    mod.bits, mod.planar, mod.REQUIRES_FORMAT_V2 = 4, False, True
    mod.register_buffer("qzeros", torch.zeros((1, 1), dtype=torch.int32))
    fmt = {"v": 1}
    mod.qzero_format = types.MethodType(lambda self, format=None: fmt.__setitem__("v", format) or format if format is not None else fmt["v"], mod)
    convert_gptq_v1_to_v2_format(torch.nn.Sequential(mod), bits=3)
    assert int(mod.qzeros.item()) == 0x11111111 and mod.qzero_format() == 2


def test_save_writes_each_module_at_its_own_width(kernels_available, tmp_path):
    """A mixed-width model (`dynamic` overrides): `format: gptq` stores zero - 1 at the MODULE's bit width, whatever the
    checkpoint-level `bits` says (the reference writer reads module.bits first, utils/model.py:908); a widened module is refused."""
    pytest.importorskip("safetensors")
    from safetensors.torch import load_file
    from gptqmodel_amd.utils.checkpoint import save_quantized_checkpoint
    from gptqmodel_amd.utils.model import shift_v1_qzeros

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.a = HipGptqLinear(bits=4, group_size=128, sym=False, desc_act=False, in_features=256, out_features=64)
            self.b = HipGptqLinear(bits=3, group_size=128, sym=False, desc_act=False, in_features=256, out_features=64)

    net = Net()
    gen = torch.Generator().manual_seed(1)
    for m in (net.a, net.b):
        m.qzeros.data = torch.randint(-2**31, 2**31 - 1, tuple(m.qzeros.shape), dtype=torch.int32, generator=gen)
        m.qzero_format(format=2)
    with pytest.raises(ValueError, match="meta.quantizer"):      # an asymmetric v1 file needs a producer entry the reference accepts
        save_quantized_checkpoint(net, str(tmp_path), {"bits": 4, "group_size": 128, "sym": False, "checkpoint_format": "gptq"})
    v1 = {"bits": 4, "group_size": 128, "sym": False, "checkpoint_format": "gptq", "meta": {"quantizer": ["gptqmodel:5.0.0"]}}
    save_quantized_checkpoint(net, str(tmp_path), dict(v1, dynamic={"+:b": {"bits": 3}}))
    disk = load_file(str(tmp_path / "model.safetensors"))
    assert torch.equal(shift_v1_qzeros(disk["a.qzeros"], 4), net.a.qzeros) and torch.equal(shift_v1_qzeros(disk["b.qzeros"], 3), net.b.qzeros)
    assert not torch.equal(disk["b.qzeros"], net.b.qzeros)
    net.b.source_bits = 3
    net.b.bits = 4                     # what widen_in_place() leaves behind
    with pytest.raises(RuntimeError, match="widened"):
        save_quantized_checkpoint(net, str(tmp_path), v1)
