"""StackedMoeExperts (nn_modules/moe_base.py) without a GPU: what HipMoeExperts and HipFp8MoeExperts inherit -- the call checks of forward, the
refusal of CPU tensors and of training mode, check_status -- and the int4 class's shape predicates against the C ABI's.  The modules are built
through __init__ alone, with the status word registered by hand on the CPU; nothing here launches a kernel."""
import os

import pytest
import torch

from gptqmodel_amd import ops
from gptqmodel_amd.nn_modules import moe, moe_fp8
from gptqmodel_amd.nn_modules.moe_base import StackedMoeExperts

E, H, I = 4, 256, 128


@pytest.fixture(scope="module")
def lib():
    from gptqmodel_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def make(cls):
    if cls is moe.HipMoeExperts:
        m = cls(E, H, I, 128, 128, torch.float16)
    else:
        m = cls(E, H, I, "block", (128, 128), "row", None)
    m.register_buffer("status", torch.zeros(1, dtype=torch.int32), persistent=False)
    return m


CLASSES = pytest.mark.parametrize("cls", [moe.HipMoeExperts, moe_fp8.HipFp8MoeExperts], ids=["int4", "fp8"])


@CLASSES
def test_one_base_and_one_token_limit(cls):
    assert issubclass(cls, StackedMoeExperts)
    assert moe.MAX_FAST_TOKENS is moe_fp8.MAX_FAST_TOKENS and moe.MAX_FAST_TOKENS == 16
    for name in ("train", "forward", "check_status", "_forward_loop", "_scratch_for", "_device_routing"):
        assert name not in vars(cls), name      # inherited, not restated


@CLASSES
@pytest.mark.parametrize("shapes", [((H,), (1, 2), (1, 2)),             # 1-D hidden
                                    ((3, H + 16), (3, 2), (3, 2)),      # wrong H
                                    ((3, H), (3, 2), (3, 1)),           # ids / weights shapes differ
                                    ((3, H), (3,), (3,)),               # 1-D routing
                                    ((3, H), (2, 2), (2, 2))],          # T differs
                         ids=["hidden-1d", "wrong-H", "ids-vs-weights", "routing-1d", "T-mismatch"])
def test_forward_refuses_malformed_arguments(cls, shapes):
    m = make(cls)
    x, ids, w = torch.zeros(shapes[0], dtype=torch.float16), torch.zeros(shapes[1], dtype=torch.int32), torch.zeros(shapes[2])
    with pytest.raises(RuntimeError, match=rf"{cls.__name__}: expected hidden_states \[T, {H}\]"):
        m(x, ids, w)


@CLASSES
def test_forward_refuses_cpu_tensors(cls):
    m = make(cls)
    for T in (0, 3):      # the refusal comes before the T == 0 return
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            m(torch.zeros((T, H), dtype=torch.float16), torch.zeros((T, 2), dtype=torch.int32), torch.zeros((T, 2)))


@CLASSES
def test_inference_only(cls):
    m = make(cls)
    with pytest.raises(NotImplementedError, match=f"{cls.__name__}: inference only"):
        m.train(True)
    with pytest.raises(NotImplementedError, match="inference only"):
        m.train()
    assert m.train(False) is m and m.eval() is m and m.training is False


@CLASSES
def test_check_status_raises_once_and_clears(cls):
    m = make(cls)
    m.check_status()
    m.status.fill_(1)
    with pytest.raises(IndexError, match=rf"{cls.__name__}: expert index out of range \[0, {E}\)") as ei:
        m.check_status()
    assert "out of range" in str(ei.value) and str(E) in str(ei.value)
    assert int(m.status.item()) == 0
    m.check_status()


# (gate_up group size, down group size) of experts Hx x Ix -> the one group_size argument of the C predicates, None = not servable
@pytest.mark.parametrize("Hx,Ix,gs_gu,gs_d,common", [(256, 128, 128, 128, 128),      # equal group sizes
                                                     (256, 128, 256, 128, -1),       # one group for the whole K of each projection
                                                     (512, 256, 128, 256, None)],    # a mismatched pair
                         ids=["equal", "whole-K", "mismatch"])
def test_int4_predicates_match_the_c_abi(lib, Hx, Ix, gs_gu, gs_d, common):
    m = moe.HipMoeExperts(8, Hx, Ix, gs_gu, gs_d, torch.float16)
    assert m._common_group_size() == (0 if common is None else common)
    for T, k in ((1, 1), (5, 3), (16, 16), (17, 2), (1, 17), (70, 8), (4097, 16)):
        want_fast = common is not None and ops.moe_supported(Hx, Ix, common, 4, False, T, k)
        want_grouped = common is not None and ops.moe_grouped_supported(Hx, Ix, common, 4, False, T, k, 8)
        for dtype, dtype_ok in ((torch.float16, True), (torch.bfloat16, False), (torch.float32, False)):      # fp16 scales: no bf16 activations
            assert m.fast_path(T, k, dtype) is (want_fast and dtype_ok), (T, k, dtype)
            assert m.grouped_path(T, k, dtype) is (want_grouped and dtype_ok), (T, k, dtype)
    if common is not None:      # the table above is not vacuous
        assert m.fast_path(16, 16, torch.float16) and not m.fast_path(17, 2, torch.float16) and m.grouped_path(70, 8, torch.float16)
    b = moe.HipMoeExperts(8, Hx, Ix, gs_gu, gs_d, torch.bfloat16)      # bf16 scales serve both activation dtypes
    assert b.fast_path(1, 1, torch.bfloat16) is b.fast_path(1, 1, torch.float16) is (common is not None)
