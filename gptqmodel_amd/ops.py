"""Thin torch-tensor wrappers over the C ABI (raw device pointers + the current HIP stream).

PyTorch is plumbing here (device memory, streams); all arithmetic happens in libgptqhip.so.
"""
from __future__ import annotations

import ctypes
from typing import Dict, Optional, Tuple

import torch

from . import _lib

FP16, BF16 = 0, 1
_DT = {torch.float16: FP16, torch.bfloat16: BF16}

# per (device index, stream handle) zero-initialised scratch, grown on demand
# (precedent: ExllamaV2 per-device ScratchSpace, gptqmodel/utils/model.py:1304-1313)
_workspaces: Dict[Tuple[int, int], torch.Tensor] = {}
# Outgrown workspaces are RETIRED, never freed: a HIP graph captured earlier still holds the old pointer and relies on
# its arrival counters staying zero, so the allocator must not hand that memory to anyone else.
_retired: list = []
# gptqhip_workspace_bytes per problem signature (it re-runs the launch planners: not free on the eager decode path)
_need_cache: Dict[Tuple[int, int, int, int, int, int], int] = {}


def _ptr(t: Optional[torch.Tensor]):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _stream(device: torch.device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


try:  # raw current-stream handle without building a torch.cuda.Stream object (~1.5 us saved per eager launch)
    _raw_stream = torch._C._cuda_getCurrentRawStream
except AttributeError:  # pragma: no cover - older / newer torch
    _raw_stream = None


def _require_cuda(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError("gptqmodel_amd HIP ops need tensors on a ROCm device (got a CPU tensor); "
                               "there is no CPU fallback")


def device_info(device: int = 0):
    lib = _lib.load()
    cu = ctypes.c_int(0)
    hbm = ctypes.c_size_t(0)
    arch = ctypes.create_string_buffer(64)
    rc = lib.gptqhip_device_info(device, ctypes.byref(cu), ctypes.byref(hbm), arch, 64)
    _lib.check(rc, "gptqhip_device_info")
    return {"cu_count": cu.value, "hbm_bytes": hbm.value, "arch": arch.value.decode()}


def _dev_index(device: torch.device) -> int:
    return device.index if device.index is not None else torch.cuda.current_device()


def _stream_handle(dev_index: int) -> int:
    if _raw_stream is not None:
        return _raw_stream(dev_index)
    return torch.cuda.current_stream(dev_index).cuda_stream


def workspace_for(device: torch.device, nbytes: int, stream_handle: Optional[int] = None) -> torch.Tensor:
    idx = _dev_index(device)
    key = (idx, _stream_handle(idx) if stream_handle is None else stream_handle)
    ws = _workspaces.get(key)
    if ws is None or ws.numel() < nbytes:
        if ws is not None:
            _retired.append(ws)
        # zero-filled: the split-K arrival counters must start at 0 (kernels reset them after use)
        ws = torch.zeros(max(nbytes, 1 << 20), dtype=torch.uint8, device=device)
        _workspaces[key] = ws
    return ws


def reserve_workspace(device: torch.device, nbytes: int) -> torch.Tensor:
    """Pre-size the current stream's workspace (e.g. for the largest prefill) BEFORE capturing a HIP graph, so that no
    later call has to replace the buffer the graph points at."""
    return workspace_for(device, nbytes)


def workspace_bytes(M: int, K: int, N: int, group_size: int, bits: int, has_perm: bool) -> int:
    key = (M, K, N, group_size, bits, 1 if has_perm else 0)
    need = _need_cache.get(key)
    if need is None:
        need = int(_lib.load().gptqhip_workspace_bytes(*key))
        if need == 0:
            raise RuntimeError(f"gptqhip_workspace_bytes: unsupported problem M={M} K={K} N={N} group_size={group_size} bits={bits}")
        if len(_need_cache) > 4096:
            _need_cache.clear()
        _need_cache[key] = need
    return need


def repack_tiled(qweight: Optional[torch.Tensor], qzeros: torch.Tensor, scales: torch.Tensor,
                 perm: Optional[torch.Tensor], group_size: int, bits: int):
    """Checkpoint layout (qweight [K*bits/32,N], qzeros [G,N*bits/32], scales [G,N]) -> (qweight_t, meta) in the
    MFMA-tile-major kernel layout (include/gptqhip.h).  One-time, on device, in post_init.
    qweight=None rebuilds only `meta` (returns (None, meta))."""
    lib = _lib.load()
    _require_cuda(qweight, qzeros, scales, perm)
    if scales.dtype not in _DT:
        raise RuntimeError(f"repack_tiled: unsupported scales dtype {scales.dtype}")
    pf = 32 // bits
    G, N = scales.shape
    K = G * group_size
    if qweight is not None:
        if tuple(qweight.shape) != (K // pf, N):
            raise RuntimeError(f"repack_tiled: qweight shape {tuple(qweight.shape)} != {(K // pf, N)}")
        qweight = qweight.contiguous()
    qzeros, scales = qzeros.contiguous(), scales.contiguous()
    nw = lib.gptqhip_tiled_words(K, N, bits)
    nm = lib.gptqhip_meta_words(K, N, group_size)
    if nw == 0 or nm == 0:
        raise RuntimeError(f"repack_tiled: unsupported shape K={K} N={N} group_size={group_size} bits={bits}")
    qw_t = torch.empty(nw, dtype=torch.int32, device=scales.device) if qweight is not None else None
    meta = torch.empty(nm, dtype=torch.int32, device=scales.device)
    with torch.cuda.device(scales.device):
        rc = lib.gptqhip_repack_tiled(_ptr(qweight), _ptr(qzeros), _ptr(scales), _ptr(perm), _ptr(qw_t), _ptr(meta),
                                      K, N, group_size, bits, _stream(scales.device))
    _lib.check(rc, "gptqhip_repack_tiled")
    return qw_t, meta


def gemm(x: torch.Tensor, qweight_t: torch.Tensor, meta: torch.Tensor, bias: Optional[torch.Tensor],
         perm: Optional[torch.Tensor], N: int, group_size: int, bits: int, scale_dtype: torch.dtype,
         out: Optional[torch.Tensor] = None, partial_f32: bool = False, exact_bf16: bool = False) -> torch.Tensor:
    """out[M,N] = x[M,K] @ dequant(qweight_t, meta) (+bias)  via gptqhip_gemm (tiled layout).
    partial_f32=True returns the unrounded float32 accumulators (tensor-parallel partial sums, no bias).
    exact_bf16=True opts in to GPTQHIP_GEMM_EXACT_BF16 (bf16 decode without the per-weight bf16 rounding; see
    include/gptqhip.h)."""
    # Hot eager path (HF generate calls this once per quantised linear per token): every line here is host time in front
    # of a 5-15 us kernel (tests/dev/eager_overhead.py), so no generic loops, no Stream / c_void_p objects, no device context
    # switch unless the tensor lives on another device than the current one.
    lib = _lib.load()
    if not (x.is_cuda and qweight_t.is_cuda and meta.is_cuda):
        raise RuntimeError("gptqmodel_amd HIP ops need tensors on a ROCm device (got a CPU tensor); "
                           "there is no CPU fallback")
    if x.dim() != 2 or not x.is_contiguous():
        raise RuntimeError("gemm: x must be a contiguous [M,K] tensor")
    adt, sdt = _DT.get(x.dtype), _DT.get(scale_dtype)
    if adt is None or sdt is None:
        raise RuntimeError(f"gemm: unsupported dtypes x={x.dtype} scales={scale_dtype}")
    if bias is not None and bias.dtype != x.dtype:
        raise RuntimeError("gemm: bias dtype must equal activation dtype")
    M, K = x.shape
    if partial_f32 and bias is not None:
        raise RuntimeError("gemm: partial_f32 excludes bias (add it once after the all-reduce)")
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32 if partial_f32 else x.dtype, device=x.device)
    if M == 0:
        return out
    idx = x.device.index
    switch = idx != torch.cuda.current_device()
    if switch:
        prev = torch.cuda.current_device()
        torch.cuda.set_device(idx)
    try:
        sh = _stream_handle(idx)
        ws = workspace_for(x.device, workspace_bytes(M, K, N, group_size, bits, perm is not None), sh)
        rc = lib.gptqhip_gemm(x.data_ptr(), qweight_t.data_ptr(), meta.data_ptr(), 0 if perm is None else perm.data_ptr(),
                              0 if bias is None else bias.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel(), M, K, N,
                              group_size, bits, adt, sdt, (1 if partial_f32 else 0) | (2 if exact_bf16 else 0), sh)
    finally:
        if switch:
            torch.cuda.set_device(prev)
    if rc != 0:
        _lib.check(rc, "gptqhip_gemm")
    return out


GLUE_NONE, GLUE_RMSNORM, GLUE_SILU_MUL = 0, 1, 2
OUT_NONE, OUT_SILU_MUL_PAIRED, OUT_PARTIAL_F32 = 0, 1, 2


def decode_supported(K: int, N: int, group_size: int, has_perm: bool = False, M: int = 1) -> bool:
    """True when gptqhip_decode_linear handles a [K,N] layer (regular pipeline; has_perm: with an act-order permutation
    applied in the kernel; M: rows 1..16), else use gemm()."""
    return bool(_lib.load().gptqhip_decode_supported(K, N, group_size, 1 if has_perm else 0, M))


def make_decode_op(x: torch.Tensor, qweight_t: torch.Tensor, meta: torch.Tensor, bias: Optional[torch.Tensor], out: torch.Tensor,
                   K: int, N: int, group_size: int, bits: int, scale_dtype: torch.dtype, in_glue: int = GLUE_NONE,
                   norm_weight: Optional[torch.Tensor] = None, eps: float = 1e-5, residual: Optional[torch.Tensor] = None,
                   workspace: Optional[torch.Tensor] = None, out_glue: int = OUT_NONE,
                   stats_in: Optional[torch.Tensor] = None, stats_out: Optional[torch.Tensor] = None,
                   perm: Optional[torch.Tensor] = None, M: int = 1, exact: bool = False) -> "_lib.DecodeOp":
    """Fill a struct gptqhip_decode_op (include/gptqhip.h) from tensors.  The struct only holds raw pointers: the caller
    keeps the tensors alive (DecodeStep does) -- binding once and re-launching costs no per-call Python work.
    `workspace`: the stream's scratch (workspace_for); taken from the CURRENT stream when omitted.
    `perm`: the module's act-order permutation (int32 [K]); applied to the glued input inside the kernel.
    `M`: rows (1..16): x [M,K], out / residual [M,N], stats_in [M, K/16], stats_out [M, ceil(N/16)], all contiguous.
    `exact`: the opt-in exact-arithmetic dequant (GPTQHIP_GEMM_EXACT, include/gptqhip.h)."""
    _require_cuda(x, qweight_t, meta, bias, out, norm_weight, residual, workspace, stats_in, stats_out, perm)
    if not 1 <= M <= 16:
        raise RuntimeError("decode op: M must be 1..16")
    if perm is not None and (perm.dtype != torch.int32 or perm.numel() != K or not perm.is_contiguous()):
        raise RuntimeError("decode op: perm must be a contiguous int32 [K] tensor")
    want_out = torch.float32 if out_glue == OUT_PARTIAL_F32 else x.dtype
    if x.dtype not in _DT or out.dtype != want_out or scale_dtype not in _DT:
        raise RuntimeError(f"decode op: unsupported dtypes x={x.dtype} out={out.dtype} scales={scale_dtype}")
    need = (2 * K if in_glue == GLUE_SILU_MUL else K) * M
    n_out = (N // 2 if out_glue == OUT_SILU_MUL_PAIRED else N) * M
    if x.numel() < need or not x.is_contiguous() or out.numel() < n_out or not out.is_contiguous():
        raise RuntimeError(f"decode op: x needs >= {need} contiguous elements (has {x.numel()}), out >= {n_out}")
    tiles_in, tiles_out = -(-K // 16), -(-N // 16)
    for t, n, what in ((stats_in, M * tiles_in, "stats_in"), (stats_out, M * tiles_out, "stats_out")):
        if t is not None and (t.dtype != torch.float32 or t.numel() < n or not t.is_contiguous()):
            raise RuntimeError(f"decode op: {what} must be a contiguous float32 tensor with >= {n} elements")
    for t, n, what in ((bias, N, "bias"), (residual, M * N, "residual"), (norm_weight, K, "norm_weight")):
        if t is not None and (t.dtype != x.dtype or t.numel() < n or not t.is_contiguous()):
            raise RuntimeError(f"decode op: {what} must be a contiguous {x.dtype} tensor with >= {n} elements")
    if in_glue == GLUE_RMSNORM and norm_weight is None:
        raise RuntimeError("decode op: GLUE_RMSNORM needs norm_weight")
    if workspace is None:
        with torch.cuda.device(x.device):
            workspace = workspace_for(x.device, workspace_bytes(M, K, N, group_size, bits, False))
    p = lambda t: 0 if t is None else t.data_ptr()
    return _lib.DecodeOp(p(qweight_t), p(meta), p(bias), p(x), p(norm_weight), p(residual), p(out), p(workspace),
                         workspace.numel(), p(stats_in), p(stats_out), p(perm), float(eps), K, N, group_size, bits, _DT[x.dtype],
                         _DT[scale_dtype], int(in_glue), int(out_glue), tiles_in if stats_in is not None else 0,
                         2 if exact else 0, int(M))


def launch_decode_op(op: "_lib.DecodeOp", device: torch.device) -> None:
    """Enqueue one decode op on the CURRENT stream of `device` (gptqhip_decode_linear)."""
    rc = _lib.load().gptqhip_decode_linear(ctypes.byref(op), _stream(device))
    _lib.check(rc, "gptqhip_decode_linear")


def bind_decode_seq(op_list):
    """ctypes array of pointers to bound decode ops, for launch_decode_seq (keeps the structs alive through the array)."""
    arr = (ctypes.POINTER(_lib.DecodeOp) * len(op_list))(*[ctypes.pointer(o) for o in op_list])
    arr._ops = list(op_list)
    return arr


def launch_decode_seq(seq, device: torch.device) -> None:
    """Enqueue a dependent run of bound decode ops with ONE host call (gptqhip_decode_linear_seq)."""
    rc = _lib.load().gptqhip_decode_linear_seq(ctypes.cast(seq, ctypes.c_void_p), len(seq), _stream(device))
    _lib.check(rc, "gptqhip_decode_linear_seq")


def decode_linear(x: torch.Tensor, qweight_t: torch.Tensor, meta: torch.Tensor, bias: Optional[torch.Tensor], K: int,
                  N: int, group_size: int, bits: int, scale_dtype: torch.dtype, **kw) -> torch.Tensor:
    """One-shot convenience wrapper (tests): out[N] of a batch-1 decode op with optional fused glue."""
    out = kw.pop("out", None)
    if out is None:
        M = int(kw.get("M", 1))
        n_out = N // 2 if kw.get("out_glue", OUT_NONE) == OUT_SILU_MUL_PAIRED else N
        out = torch.empty(n_out if M == 1 else (M, n_out), dtype=torch.float32 if kw.get("out_glue") == OUT_PARTIAL_F32 else x.dtype,
                          device=x.device)
    with torch.cuda.device(x.device):
        op = make_decode_op(x, qweight_t, meta, bias, out, K, N, group_size, bits, scale_dtype, **kw)
        launch_decode_op(op, x.device)
    return out


def moe_supported(H: int, I: int, group_size: int, bits: int = 4, has_perm: bool = False, T: int = 1, top_k: int = 1) -> bool:
    """True when the fused MoE decode ops (gptqhip_moe_gate_up / gptqhip_moe_down) serve experts with hidden size H and intermediate
    size I for T tokens x top_k slots (host logic, no GPU); group_size <= 0: one group for the whole K of each projection."""
    return bool(_lib.load().gptqhip_moe_supported(H, I, group_size, bits, 1 if has_perm else 0, T, top_k))


def _moe_io_check(what: str, x: torch.Tensor, rows: int, cols: int, ids: torch.Tensor, status: torch.Tensor):
    """The x / ids / status checks of every few-token MoE stage, int4 and FP8."""
    if x.dim() != 2 or tuple(x.shape) != (rows, cols) or not x.is_contiguous():
        raise RuntimeError(f"{what}: input must be a contiguous [{rows}, {cols}] tensor (got {tuple(x.shape)})")
    if ids.dtype != torch.int32 or ids.dim() != 2 or not ids.is_contiguous():
        raise RuntimeError(f"{what}: ids must be a contiguous int32 [T, top_k] tensor")
    if status.dtype != torch.int32 or status.numel() < 1:
        raise RuntimeError(f"{what}: status must be an int32 tensor")


def _moe_check(what: str, x: torch.Tensor, rows: int, cols: int, ids: torch.Tensor, status: torch.Tensor, scale_dtype: torch.dtype):
    if x.dtype not in _DT or scale_dtype not in _DT:
        raise RuntimeError(f"{what}: unsupported dtypes x={x.dtype} scales={scale_dtype}")
    _moe_io_check(what, x, rows, cols, ids, status)


def moe_gate_up(x: torch.Tensor, qweight_t: torch.Tensor, meta: torch.Tensor, ids: torch.Tensor, act: torch.Tensor, status: torch.Tensor,
                E: int, I: int, group_size: int, scale_dtype: torch.dtype, bits: int = 4) -> torch.Tensor:
    """Stage one of the fused MoE experts (gptqhip_moe_gate_up): act[t * top_k + j, :I] = silu(g) * u with g | u = x[t] @ the fused, interleaved
    gate|up projection of expert ids[t, j], read from the stacked tiled words / constants of all E experts.  x [T, H], ids int32 [T, top_k]
    (on the device: nothing is read back), act [T * top_k, I] and status (int32, set to 1 by an id outside [0, E)) are the caller's."""
    _require_cuda(x, qweight_t, meta, ids, act, status)
    T, top_k = ids.shape if ids.dim() == 2 else (0, 0)
    H = x.shape[-1]
    _moe_check("moe_gate_up", x, T, H, ids, status, scale_dtype)
    if act.dtype != x.dtype or act.numel() < T * top_k * I or not act.is_contiguous():
        raise RuntimeError(f"moe_gate_up: act must be a contiguous {x.dtype} tensor with >= {T * top_k * I} elements")
    with torch.cuda.device(x.device):
        rc = _lib.load().gptqhip_moe_gate_up(_ptr(x), _ptr(qweight_t), _ptr(meta), _ptr(ids), _ptr(act), _ptr(status), T, top_k, E, H, I,
                                             group_size, bits, _DT[x.dtype], _DT[scale_dtype], _stream(x.device))
    _lib.check(rc, "gptqhip_moe_gate_up")
    return act


def moe_down(act: torch.Tensor, qweight_t: torch.Tensor, meta: torch.Tensor, ids: torch.Tensor, weights: torch.Tensor, out: torch.Tensor,
             status: torch.Tensor, E: int, group_size: int, scale_dtype: torch.dtype, bits: int = 4) -> torch.Tensor:
    """Stage two (gptqhip_moe_down): out[t, :H] = round( sum_j weights[t, j] * (act[t * top_k + j] @ down projection of expert ids[t, j]) ), fp32
    dot products and ONE fp32 weighted sum in slot order, rounded once (deterministic: no atomics).  act [T * top_k, I], weights float32
    [T, top_k], out [T, H]."""
    _require_cuda(act, qweight_t, meta, ids, weights, out, status)
    T, top_k = ids.shape if ids.dim() == 2 else (0, 0)
    I = act.shape[-1]
    _moe_check("moe_down", act, T * top_k, I, ids, status, scale_dtype)
    if weights.dtype != torch.float32 or tuple(weights.shape) != (T, top_k) or not weights.is_contiguous():
        raise RuntimeError("moe_down: weights must be a contiguous float32 [T, top_k] tensor")
    if out.dtype != act.dtype or out.dim() != 2 or out.shape[0] != T or not out.is_contiguous():
        raise RuntimeError(f"moe_down: out must be a contiguous {act.dtype} [T, H] tensor")
    H = out.shape[1]
    with torch.cuda.device(act.device):
        rc = _lib.load().gptqhip_moe_down(_ptr(act), _ptr(qweight_t), _ptr(meta), _ptr(ids), _ptr(weights), _ptr(out), _ptr(status), T, top_k, E,
                                          H, I, group_size, bits, _DT[act.dtype], _DT[scale_dtype], _stream(act.device))
    _lib.check(rc, "gptqhip_moe_down")
    return out


def moe_grouped_supported(H: int, I: int, group_size: int, bits: int = 4, has_perm: bool = False, T: int = 1, top_k: int = 1, E: int = 1) -> bool:
    """True when the expert-grouped MoE ops (moe_align / moe_gate_up_grouped / moe_down_grouped / moe_combine) serve E experts with hidden size H
    and intermediate size I for T tokens x top_k slots (host logic, no GPU); group_size <= 0: one group for the whole K of each projection."""
    return bool(_lib.load().gptqhip_moe_grouped_supported(H, I, group_size, bits, 1 if has_perm else 0, T, top_k, E))


def moe_grouped_units(S: int, E: int) -> int:
    """The most 16-row units S slots on E experts can fill (gptqhip_moe_grouped_units): the length of unit_expert, 1 / 16 of sorted_slots."""
    return int(_lib.load().gptqhip_moe_grouped_units(S, E))


def _moe_sort_check(what: str, S: int, E: int, sorted_slots: torch.Tensor, unit_expert: torch.Tensor, num_units: torch.Tensor) -> None:
    units = moe_grouped_units(S, E)
    for t, n, name in ((sorted_slots, 16 * units, "sorted_slots"), (unit_expert, units, "unit_expert"), (num_units, 1, "num_units")):
        if t.dtype != torch.int32 or t.numel() < max(n, 1) or not t.is_contiguous():
            raise RuntimeError(f"{what}: {name} must be a contiguous int32 tensor with >= {n} elements")


def moe_align(ids: torch.Tensor, sorted_slots: torch.Tensor, unit_expert: torch.Tensor, num_units: torch.Tensor, status: torch.Tensor,
              E: int) -> None:
    """Stable counting sort of the T * top_k slots by expert id on the device (gptqhip_moe_align): sorted_slots int32 [16 * units] (experts
    ascending, slots ascending within an expert, -1 padding to 16-row units), unit_expert int32 [units], num_units int32 [1], with
    units = moe_grouped_units(T * top_k, E); ids outside [0, E) are in no unit and set status to 1."""
    _require_cuda(ids, sorted_slots, unit_expert, num_units, status)
    if ids.dtype != torch.int32 or ids.dim() != 2 or not ids.is_contiguous():
        raise RuntimeError("moe_align: ids must be a contiguous int32 [T, top_k] tensor")
    if status.dtype != torch.int32 or status.numel() < 1:
        raise RuntimeError("moe_align: status must be an int32 tensor")
    T, top_k = ids.shape
    _moe_sort_check("moe_align", T * top_k, E, sorted_slots, unit_expert, num_units)
    with torch.cuda.device(ids.device):
        rc = _lib.load().gptqhip_moe_align(_ptr(ids), _ptr(sorted_slots), _ptr(unit_expert), _ptr(num_units), _ptr(status), T, top_k, E,
                                           _stream(ids.device))
    _lib.check(rc, "gptqhip_moe_align")


def moe_gate_up_grouped(x: torch.Tensor, qweight_t: torch.Tensor, meta: torch.Tensor, sorted_slots: torch.Tensor, unit_expert: torch.Tensor,
                        num_units: torch.Tensor, act: torch.Tensor, top_k: int, E: int, I: int, group_size: int, scale_dtype: torch.dtype,
                        bits: int = 4) -> torch.Tensor:
    """Stage one on the sorted slots (gptqhip_moe_gate_up_grouped): act[s, :I] of every slot in a unit, the rounding chain of moe_gate_up.
    x [T, H]; act: >= T * top_k * I elements of x.dtype (rows of slots in no unit are left untouched)."""
    _require_cuda(x, qweight_t, meta, sorted_slots, unit_expert, num_units, act)
    if x.dtype not in _DT or scale_dtype not in _DT or x.dim() != 2 or not x.is_contiguous():
        raise RuntimeError(f"moe_gate_up_grouped: x must be a contiguous 16-bit [T, H] tensor (got {x.dtype} {tuple(x.shape)})")
    T, H = x.shape
    _moe_sort_check("moe_gate_up_grouped", T * top_k, E, sorted_slots, unit_expert, num_units)
    if act.dtype != x.dtype or act.numel() < T * top_k * I or not act.is_contiguous():
        raise RuntimeError(f"moe_gate_up_grouped: act must be a contiguous {x.dtype} tensor with >= {T * top_k * I} elements")
    with torch.cuda.device(x.device):
        rc = _lib.load().gptqhip_moe_gate_up_grouped(_ptr(x), _ptr(qweight_t), _ptr(meta), _ptr(sorted_slots), _ptr(unit_expert), _ptr(num_units),
                                                     _ptr(act), T, top_k, E, H, I, group_size, bits, _DT[x.dtype], _DT[scale_dtype],
                                                     _stream(x.device))
    _lib.check(rc, "gptqhip_moe_gate_up_grouped")
    return act


def moe_down_grouped(act: torch.Tensor, qweight_t: torch.Tensor, meta: torch.Tensor, sorted_slots: torch.Tensor, unit_expert: torch.Tensor,
                     num_units: torch.Tensor, part: torch.Tensor, top_k: int, E: int, H: int, group_size: int, scale_dtype: torch.dtype,
                     bits: int = 4) -> torch.Tensor:
    """Stage two on the sorted slots (gptqhip_moe_down_grouped): part[s, :H] = act[s] @ the down projection of the slot's expert, UNROUNDED
    fp32.  act [T * top_k, I]; part: >= T * top_k * H float32 elements."""
    _require_cuda(act, qweight_t, meta, sorted_slots, unit_expert, num_units, part)
    if act.dtype not in _DT or scale_dtype not in _DT or act.dim() != 2 or not act.is_contiguous() or act.shape[0] % top_k != 0:
        raise RuntimeError(f"moe_down_grouped: act must be a contiguous 16-bit [T * top_k, I] tensor (got {act.dtype} {tuple(act.shape)})")
    S, I = act.shape
    _moe_sort_check("moe_down_grouped", S, E, sorted_slots, unit_expert, num_units)
    if part.dtype != torch.float32 or part.numel() < S * H or not part.is_contiguous():
        raise RuntimeError(f"moe_down_grouped: part must be a contiguous float32 tensor with >= {S * H} elements")
    with torch.cuda.device(act.device):
        rc = _lib.load().gptqhip_moe_down_grouped(_ptr(act), _ptr(qweight_t), _ptr(meta), _ptr(sorted_slots), _ptr(unit_expert), _ptr(num_units),
                                                  _ptr(part), S // top_k, top_k, E, H, I, group_size, bits, _DT[act.dtype], _DT[scale_dtype],
                                                  _stream(act.device))
    _lib.check(rc, "gptqhip_moe_down_grouped")
    return part


def moe_combine(part: torch.Tensor, ids: torch.Tensor, weights: torch.Tensor, out: torch.Tensor, status: torch.Tensor, E: int) -> torch.Tensor:
    """out[t, :H] = round( sum_j weights[t, j] * part[t * top_k + j] ) (gptqhip_moe_combine): one fp32 sum in slot order, one rounding, ids outside
    [0, E) skipped -- the contract of moe_down.  part float32 [T * top_k, H], ids int32 / weights float32 [T, top_k], out 16-bit [T, H]."""
    _require_cuda(part, ids, weights, out, status)
    if ids.dtype != torch.int32 or ids.dim() != 2 or not ids.is_contiguous():
        raise RuntimeError("moe_combine: ids must be a contiguous int32 [T, top_k] tensor")
    T, top_k = ids.shape
    if weights.dtype != torch.float32 or tuple(weights.shape) != (T, top_k) or not weights.is_contiguous():
        raise RuntimeError("moe_combine: weights must be a contiguous float32 [T, top_k] tensor")
    if out.dtype not in _DT or out.dim() != 2 or out.shape[0] != T or not out.is_contiguous():
        raise RuntimeError("moe_combine: out must be a contiguous 16-bit [T, H] tensor")
    H = out.shape[1]
    if part.dtype != torch.float32 or part.numel() < T * top_k * H or not part.is_contiguous():
        raise RuntimeError(f"moe_combine: part must be a contiguous float32 tensor with >= {T * top_k * H} elements")
    if status.dtype != torch.int32 or status.numel() < 1:
        raise RuntimeError("moe_combine: status must be an int32 tensor")
    with torch.cuda.device(part.device):
        rc = _lib.load().gptqhip_moe_combine(_ptr(part), _ptr(ids), _ptr(weights), _ptr(out), _ptr(status), T, top_k, E, H, _DT[out.dtype],
                                             _stream(part.device))
    _lib.check(rc, "gptqhip_moe_combine")
    return out


FP8_SCALE_TENSOR, FP8_SCALE_ROW, FP8_SCALE_BLOCK = 0, 1, 2
FP8_SCALE_MODES = {"tensor": FP8_SCALE_TENSOR, "row": FP8_SCALE_ROW, "block": FP8_SCALE_BLOCK}
FP8_FORMATS = {"float8_e4m3fn": 0, "float8_e5m2": 1, "float8_e4m3fnuz": 2, "float8_e8m0fnu": 3}
FP8_CVT = {"default": 0, "packed": 1, "f32": 2, "bits": 3}
_DT_OUT = {torch.float16: 0, torch.bfloat16: 1, torch.float32: 2}


def _fp8_block(scale_mode: int, block_size) -> Tuple[int, int]:
    if scale_mode != FP8_SCALE_BLOCK:
        return 0, 0
    if block_size is None or len(block_size) != 2:
        raise RuntimeError("fp8: block scales need a (rows, cols) block size")
    return int(block_size[0]), int(block_size[1])


def _fp8_scale_count(K: int, N: int, scale_mode: int, br: int, bc: int) -> int:
    if scale_mode == FP8_SCALE_TENSOR:
        return 1
    if scale_mode == FP8_SCALE_ROW:
        return N
    return (N // max(br, 1)) * (K // max(bc, 1))


def fp8_supported(M: int, K: int, N: int, scale_mode: int, block_size=None, dtype: torch.dtype = torch.float16,
                  fmt: str = "float8_e4m3fn") -> bool:
    """True when gptqhip_fp8_gemm serves x [M, K] on an FP8 [N, K] weight with this scale layout (FP8_SCALE_*; block_size = (rows, cols)
    of the [N, K] weight per scale), activation dtype and float8 format -- gptqhip_fp8_supported, host logic, no GPU."""
    br, bc = (0, 0) if scale_mode != FP8_SCALE_BLOCK or block_size is None else (int(block_size[0]), int(block_size[1]))
    return bool(_lib.load().gptqhip_fp8_supported(M, K, N, scale_mode, br, bc, _DT.get(dtype, -1), FP8_FORMATS.get(fmt, -1)))


def fp8_repack(weight: torch.Tensor, scale_inv: torch.Tensor, scale_mode: int, block_size=None):
    """Checkpoint tensors (weight float8_e4m3fn | uint8 [N, K], scale_inv fp32 () | (N,) | (N / br, K / bc)) -> (weight_t uint8 [N * K] in
    the MFMA-tile-major kernel layout, rscale fp32 = 1 / scale_inv, same shape).  One-time, on the device, in post_init."""
    lib = _lib.load()
    _require_cuda(weight, scale_inv)
    if weight.dim() != 2 or weight.element_size() != 1:
        raise RuntimeError(f"fp8_repack: weight must be a 2-D one-byte tensor (got {weight.dtype} {tuple(weight.shape)})")
    N, K = weight.shape
    br, bc = _fp8_block(scale_mode, block_size)
    w = weight.contiguous().view(torch.uint8)
    s = scale_inv.to(torch.float32).contiguous()
    want = _fp8_scale_count(K, N, scale_mode, br, bc)
    if s.numel() != want:
        raise RuntimeError(f"fp8_repack: scale_inv has {s.numel()} elements, the scale layout needs {want}")
    nbytes = lib.gptqhip_fp8_tiled_bytes(K, N)
    if nbytes == 0:
        raise RuntimeError(f"fp8_repack: unsupported shape K={K} N={N} (K % 128 == 0 and N % 16 == 0)")
    w_t = torch.empty(nbytes, dtype=torch.uint8, device=weight.device)
    rscale = torch.empty_like(s)
    with torch.cuda.device(weight.device):
        rc = lib.gptqhip_fp8_repack(_ptr(w), _ptr(s), _ptr(w_t), _ptr(rscale), K, N, scale_mode, br, bc, _stream(weight.device))
    _lib.check(rc, "gptqhip_fp8_repack")
    return w_t, rscale


def fp8_gemm(x: torch.Tensor, weight_t: torch.Tensor, rscale: torch.Tensor, bias: Optional[torch.Tensor], N: int, scale_mode: int,
             block_size=None, out: Optional[torch.Tensor] = None, cvt: str = "default") -> torch.Tensor:
    """out[M, N] = x[M, K] @ W^T (+ bias) with W = code * rscale, fp32 accumulation and ONE rounding (gptqhip_fp8_gemm): the decode kernel
    up to 16 rows, the MFMA-tiled general kernel above.  `cvt`: the decode kernel's conversion route (FP8_CVT; a measurement hook)."""
    lib = _lib.load()
    if not (x.is_cuda and weight_t.is_cuda and rscale.is_cuda and (bias is None or bias.is_cuda)):
        raise RuntimeError("gptqmodel_amd HIP ops need tensors on a ROCm device (got a CPU tensor); "
                           "there is no CPU fallback")
    if x.dim() != 2 or not x.is_contiguous():
        raise RuntimeError("fp8_gemm: x must be a contiguous [M,K] tensor")
    adt = _DT.get(x.dtype)
    if adt is None:
        raise RuntimeError(f"fp8_gemm: unsupported activation dtype {x.dtype}")
    if bias is not None and (bias.dtype != x.dtype or bias.numel() != N or not bias.is_contiguous()):
        raise RuntimeError("fp8_gemm: bias must be a contiguous [N] tensor of the activation dtype")
    M, K = x.shape
    if weight_t.dtype != torch.uint8 or weight_t.numel() != K * N or rscale.dtype != torch.float32:
        raise RuntimeError(f"fp8_gemm: weight_t must hold K * N = {K * N} bytes (uint8) and rscale must be float32")
    br, bc = _fp8_block(scale_mode, block_size)
    if rscale.numel() != _fp8_scale_count(K, N, scale_mode, br, bc):
        raise RuntimeError(f"fp8_gemm: rscale has {rscale.numel()} elements, the scale layout needs {_fp8_scale_count(K, N, scale_mode, br, bc)}")
    if out is None:
        out = torch.empty((M, N), dtype=x.dtype, device=x.device)
    elif out.dtype != x.dtype or out.numel() != M * N or not out.is_contiguous():
        raise RuntimeError("fp8_gemm: out must be a contiguous [M,N] tensor of the activation dtype")
    if M == 0:
        return out
    with torch.cuda.device(x.device):
        rc = lib.gptqhip_fp8_gemm(x.data_ptr(), weight_t.data_ptr(), rscale.data_ptr(), 0 if bias is None else bias.data_ptr(),
                                  out.data_ptr(), M, K, N, scale_mode, br, bc, adt, FP8_CVT[cvt], _stream_handle(_dev_index(x.device)))
    if rc != 0:
        _lib.check(rc, "gptqhip_fp8_gemm")
    return out


def fp8_dequant(weight_t: torch.Tensor, rscale: torch.Tensor, K: int, N: int, scale_mode: int, block_size=None,
                out_dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """[K, N] weights from the kernel layout in fp16 | bf16 | fp32, each element rounded once from the fp32 product code * rscale."""
    lib = _lib.load()
    _require_cuda(weight_t, rscale)
    if out_dtype not in _DT_OUT:
        raise RuntimeError(f"fp8_dequant: unsupported output dtype {out_dtype}")
    if weight_t.dtype != torch.uint8 or weight_t.numel() != K * N or rscale.dtype != torch.float32:
        raise RuntimeError(f"fp8_dequant: weight_t must hold K * N = {K * N} bytes (uint8) and rscale must be float32")
    br, bc = _fp8_block(scale_mode, block_size)
    if rscale.numel() != _fp8_scale_count(K, N, scale_mode, br, bc):
        raise RuntimeError(f"fp8_dequant: rscale has {rscale.numel()} elements, the scale layout needs {_fp8_scale_count(K, N, scale_mode, br, bc)}")
    out = torch.empty((K, N), dtype=out_dtype, device=weight_t.device)
    with torch.cuda.device(weight_t.device):
        rc = lib.gptqhip_fp8_dequant(_ptr(weight_t), _ptr(rscale), _ptr(out), K, N, scale_mode, br, bc, _DT_OUT[out_dtype],
                                     _stream(weight_t.device))
    _lib.check(rc, "gptqhip_fp8_dequant")
    return out


FP4_BLOCK = 16
FP4_CVT = {"default": 0, "packed": 1, "f32": 2}


def fp4_supported(M: int, K: int, N: int, block_size: int = FP4_BLOCK, dtype: torch.dtype = torch.float16) -> bool:
    """True when gptqhip_fp4_gemm serves x [M, K] on an NVFP4 [N, K] weight (one e4m3 scale per `block_size` input features) with this
    activation dtype -- gptqhip_fp4_supported, host logic, no GPU."""
    return bool(_lib.load().gptqhip_fp4_supported(M, K, N, int(block_size), _DT.get(dtype, -1)))


def _fp4_global_scale(global_scale: Optional[torch.Tensor], what: str) -> Optional[torch.Tensor]:
    if global_scale is not None and (global_scale.dtype != torch.float32 or global_scale.numel() != 1):
        raise RuntimeError(f"{what}: global_scale must be a float32 tensor of one element (or None = 1.0)")
    return global_scale


def _fp4_check_layout(what: str, weight_t: torch.Tensor, scale_t: torch.Tensor, K: int, N: int):
    if weight_t.dtype != torch.uint8 or weight_t.numel() * 2 != K * N or scale_t.dtype != torch.uint8 or scale_t.numel() * FP4_BLOCK != K * N:
        raise RuntimeError(f"{what}: weight_t must hold K * N / 2 = {K * N // 2} bytes and scale_t K * N / 16 = {K * N // 16} bytes (uint8)")


def fp4_repack(weight: torch.Tensor, weight_scale: torch.Tensor, block_size: int = FP4_BLOCK):
    """Checkpoint tensors (weight uint8 | float4_e2m1fn_x2 [N, K / 2], low nibble = even feature; weight_scale float8_e4m3fn | uint8
    [N, K / 16]) -> (weight_t uint8 [K * N / 2], scale_t uint8 [K * N / 16]) in the MFMA-tile-major kernel layout.  One-time, on the device."""
    lib = _lib.load()
    _require_cuda(weight, weight_scale)
    if weight.dim() != 2 or weight.element_size() != 1 or weight_scale.dim() != 2 or weight_scale.element_size() != 1:
        raise RuntimeError(f"fp4_repack: weight and weight_scale must be 2-D one-byte tensors (got {weight.dtype} {tuple(weight.shape)}, "
                           f"{weight_scale.dtype} {tuple(weight_scale.shape)})")
    if weight_scale.dtype not in (torch.uint8, torch.float8_e4m3fn):
        raise RuntimeError(f"fp4_repack: weight_scale must be float8_e4m3fn (or its uint8 view), got {weight_scale.dtype}")
    N, K = weight.shape[0], weight.shape[1] * 2
    if tuple(weight_scale.shape) != (N, K // max(int(block_size), 1)):
        raise RuntimeError(f"fp4_repack: weight_scale shape {tuple(weight_scale.shape)} != {(N, K // max(int(block_size), 1))} "
                           "(plain row-major; a swizzled scale layout is not supported)")
    nbytes, sbytes = lib.gptqhip_fp4_tiled_bytes(K, N), lib.gptqhip_fp4_scale_bytes(K, N)
    if nbytes == 0 or int(block_size) != FP4_BLOCK:
        raise RuntimeError(f"fp4_repack: unsupported shape K={K} N={N} block size {block_size} (K % 128 == 0, N % 16 == 0, block size 16)")
    w = weight.contiguous().view(torch.uint8)
    s = weight_scale.contiguous().view(torch.uint8)
    w_t = torch.empty(nbytes, dtype=torch.uint8, device=weight.device)
    s_t = torch.empty(sbytes, dtype=torch.uint8, device=weight.device)
    with torch.cuda.device(weight.device):
        rc = lib.gptqhip_fp4_repack(_ptr(w), _ptr(s), _ptr(w_t), _ptr(s_t), K, N, int(block_size), _stream(weight.device))
    _lib.check(rc, "gptqhip_fp4_repack")
    return w_t, s_t


def fp4_gemm(x: torch.Tensor, weight_t: torch.Tensor, scale_t: torch.Tensor, global_scale: Optional[torch.Tensor],
             bias: Optional[torch.Tensor], N: int, block_size: int = FP4_BLOCK, out: Optional[torch.Tensor] = None,
             cvt: str = "default") -> torch.Tensor:
    """out[M, N] = x[M, K] @ W^T (+ bias) with W = code * block scale * global_scale: exact block-scaled weights on the matrix pipe, fp32
    sums, the global scale and the bias on the accumulator, ONE rounding (gptqhip_fp4_gemm): the decode kernel up to 16 rows, the MFMA-tiled
    general kernel above.  `global_scale`: a one-element float32 DEVICE tensor or None (1.0).  `cvt`: the conversion route (FP4_CVT)."""
    lib = _lib.load()
    if not (x.is_cuda and weight_t.is_cuda and scale_t.is_cuda and (bias is None or bias.is_cuda)
            and (global_scale is None or global_scale.is_cuda)):
        raise RuntimeError("gptqmodel_amd HIP ops need tensors on a ROCm device (got a CPU tensor); "
                           "there is no CPU fallback")
    if x.dim() != 2 or not x.is_contiguous():
        raise RuntimeError("fp4_gemm: x must be a contiguous [M,K] tensor")
    adt = _DT.get(x.dtype)
    if adt is None:
        raise RuntimeError(f"fp4_gemm: unsupported activation dtype {x.dtype}")
    if bias is not None and (bias.dtype != x.dtype or bias.numel() != N or not bias.is_contiguous()):
        raise RuntimeError("fp4_gemm: bias must be a contiguous [N] tensor of the activation dtype")
    M, K = x.shape
    _fp4_check_layout("fp4_gemm", weight_t, scale_t, K, N)
    _fp4_global_scale(global_scale, "fp4_gemm")
    if out is None:
        out = torch.empty((M, N), dtype=x.dtype, device=x.device)
    elif out.dtype != x.dtype or out.numel() != M * N or not out.is_contiguous():
        raise RuntimeError("fp4_gemm: out must be a contiguous [M,N] tensor of the activation dtype")
    if M == 0:
        return out
    with torch.cuda.device(x.device):
        rc = lib.gptqhip_fp4_gemm(x.data_ptr(), weight_t.data_ptr(), scale_t.data_ptr(), 0 if global_scale is None else global_scale.data_ptr(),
                                  0 if bias is None else bias.data_ptr(), out.data_ptr(), M, K, N, int(block_size), adt, FP4_CVT[cvt],
                                  _stream_handle(_dev_index(x.device)))
    if rc != 0:
        _lib.check(rc, "gptqhip_fp4_gemm")
    return out


def fp4_dequant(weight_t: torch.Tensor, scale_t: torch.Tensor, global_scale: Optional[torch.Tensor], K: int, N: int,
                block_size: int = FP4_BLOCK, out_dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """[K, N] weights from the kernel layout in fp16 | bf16 | fp32, each element round(fp32(code * block scale) * global_scale), once."""
    lib = _lib.load()
    _require_cuda(weight_t, scale_t, global_scale)
    if out_dtype not in _DT_OUT:
        raise RuntimeError(f"fp4_dequant: unsupported output dtype {out_dtype}")
    _fp4_check_layout("fp4_dequant", weight_t, scale_t, K, N)
    _fp4_global_scale(global_scale, "fp4_dequant")
    out = torch.empty((K, N), dtype=out_dtype, device=weight_t.device)
    with torch.cuda.device(weight_t.device):
        rc = lib.gptqhip_fp4_dequant(_ptr(weight_t), _ptr(scale_t), _ptr(global_scale), _ptr(out), K, N, int(block_size), _DT_OUT[out_dtype],
                                     _stream(weight_t.device))
    _lib.check(rc, "gptqhip_fp4_dequant")
    return out


def moe_fp8_supported(H: int, I: int, gate_up_block_cols: int = 0, down_scale_mode: int = FP8_SCALE_ROW, down_block_size=None, T: int = 1,
                      top_k: int = 1, dtype: torch.dtype = torch.float16) -> bool:
    """True when the fused FP8 MoE decode ops (gptqhip_moe_fp8_gate_up / gptqhip_moe_fp8_down) serve experts with hidden size H and intermediate
    size I for T tokens x top_k slots (host logic, no GPU).  gate_up_block_cols: 0 = one scale per fused column, bc = K-block scales of bc
    columns; down_scale_mode / down_block_size: the down projection's FP8_SCALE_* layout and (rows, cols) block."""
    br, bc = (0, 0) if down_scale_mode != FP8_SCALE_BLOCK or down_block_size is None else (int(down_block_size[0]), int(down_block_size[1]))
    return bool(_lib.load().gptqhip_moe_fp8_supported(H, I, int(gate_up_block_cols), down_scale_mode, br, bc, T, top_k, _DT.get(dtype, -1)))


def _moe_fp8_stacked_check(what: str, weight_t: torch.Tensor, rscale: torch.Tensor, E: int, w_bytes: int, n_scales: int):
    """The stacked weights / reciprocal scales of every FP8 MoE stage, few-token and grouped."""
    if weight_t.dtype != torch.uint8 or weight_t.numel() != E * w_bytes or not weight_t.is_contiguous():
        raise RuntimeError(f"{what}: weight_t must be a contiguous uint8 tensor of E * {w_bytes} bytes")
    if rscale.dtype != torch.float32 or rscale.numel() != E * n_scales or not rscale.is_contiguous():
        raise RuntimeError(f"{what}: rscale must be a contiguous float32 tensor of E * {n_scales} elements")


def _moe_fp8_check(what: str, x: torch.Tensor, rows: int, cols: int, ids: torch.Tensor, status: torch.Tensor, weight_t: torch.Tensor,
                   rscale: torch.Tensor, E: int, w_bytes: int, n_scales: int):
    if x.dtype not in _DT:
        raise RuntimeError(f"{what}: unsupported activation dtype {x.dtype}")
    _moe_io_check(what, x, rows, cols, ids, status)
    _moe_fp8_stacked_check(what, weight_t, rscale, E, w_bytes, n_scales)


def moe_fp8_gate_up(x: torch.Tensor, weight_t: torch.Tensor, rscale: torch.Tensor, ids: torch.Tensor, act: torch.Tensor, status: torch.Tensor,
                    E: int, I: int, block_cols: int = 0) -> torch.Tensor:
    """Stage one of the fused FP8 MoE experts (gptqhip_moe_fp8_gate_up): act[t * top_k + j, :I] = silu(g) * u with g | u = x[t] @ the fused,
    row-interleaved gate|up weight of expert ids[t, j], read from the stacked kernel-layout bytes [E, 2I * H] and reciprocal scales ([E, 2I], or
    [E, 2I, H / block_cols] with K-block scales) of all E experts.  x [T, H], ids int32 [T, top_k] (on the device: nothing is read back),
    act [T * top_k, I] and status (int32, set to 1 by an id outside [0, E)) are the caller's."""
    _require_cuda(x, weight_t, rscale, ids, act, status)
    T, top_k = ids.shape if ids.dim() == 2 else (0, 0)
    H = x.shape[-1]
    bc = int(block_cols)
    _moe_fp8_check("moe_fp8_gate_up", x, T, H, ids, status, weight_t, rscale, E, 2 * I * H, 2 * I * (H // bc if bc > 0 else 1))
    if act.dtype != x.dtype or act.numel() < T * top_k * I or not act.is_contiguous():
        raise RuntimeError(f"moe_fp8_gate_up: act must be a contiguous {x.dtype} tensor with >= {T * top_k * I} elements")
    with torch.cuda.device(x.device):
        rc = _lib.load().gptqhip_moe_fp8_gate_up(_ptr(x), _ptr(weight_t), _ptr(rscale), _ptr(ids), _ptr(act), _ptr(status), T, top_k, E, H, I,
                                                 bc, _DT[x.dtype], _stream(x.device))
    _lib.check(rc, "gptqhip_moe_fp8_gate_up")
    return act


def moe_fp8_down(act: torch.Tensor, weight_t: torch.Tensor, rscale: torch.Tensor, ids: torch.Tensor, weights: torch.Tensor, out: torch.Tensor,
                 status: torch.Tensor, E: int, scale_mode: int, block_size=None) -> torch.Tensor:
    """Stage two (gptqhip_moe_fp8_down): out[t, :H] = round( sum_j weights[t, j] * (act[t * top_k + j] @ down weight of expert ids[t, j]) ), fp32
    dot products and ONE fp32 weighted sum in slot order, rounded once (deterministic: no atomics).  act [T * top_k, I], weights float32
    [T, top_k], out [T, H]; weight_t uint8 [E, I * H], rscale float32 [E] | [E, H] | [E, H / br, I / bc]."""
    _require_cuda(act, weight_t, rscale, ids, weights, out, status)
    T, top_k = ids.shape if ids.dim() == 2 else (0, 0)
    I = act.shape[-1]
    if out.dim() != 2:
        raise RuntimeError(f"moe_fp8_down: out must be a contiguous {act.dtype} [T, H] tensor")
    H = out.shape[1]
    br, bc = _fp8_block(scale_mode, block_size)
    _moe_fp8_check("moe_fp8_down", act, T * top_k, I, ids, status, weight_t, rscale, E, I * H, _fp8_scale_count(I, H, scale_mode, br, bc))
    if weights.dtype != torch.float32 or tuple(weights.shape) != (T, top_k) or not weights.is_contiguous():
        raise RuntimeError("moe_fp8_down: weights must be a contiguous float32 [T, top_k] tensor")
    if out.dtype != act.dtype or out.shape[0] != T or not out.is_contiguous():
        raise RuntimeError(f"moe_fp8_down: out must be a contiguous {act.dtype} [T, H] tensor")
    with torch.cuda.device(act.device):
        rc = _lib.load().gptqhip_moe_fp8_down(_ptr(act), _ptr(weight_t), _ptr(rscale), _ptr(ids), _ptr(weights), _ptr(out), _ptr(status), T, top_k,
                                              E, H, I, scale_mode, br, bc, _DT[act.dtype], _stream(act.device))
    _lib.check(rc, "gptqhip_moe_fp8_down")
    return out


def moe_fp8_grouped_supported(H: int, I: int, gate_up_block_cols: int = 0, down_scale_mode: int = FP8_SCALE_ROW, down_block_size=None, T: int = 1,
                              top_k: int = 1, E: int = 1, dtype: torch.dtype = torch.float16) -> bool:
    """True when the expert-grouped FP8 MoE ops (moe_align / moe_fp8_gate_up_grouped / moe_fp8_down_grouped / moe_combine) serve E experts with
    hidden size H and intermediate size I for T tokens x top_k slots (gptqhip_moe_fp8_grouped_supported: host logic, no GPU): the shape and
    scale rules of moe_fp8_supported at ANY T, within the routing limits of the grouped ops."""
    br, bc = (0, 0) if down_scale_mode != FP8_SCALE_BLOCK or down_block_size is None else (int(down_block_size[0]), int(down_block_size[1]))
    return bool(_lib.load().gptqhip_moe_fp8_grouped_supported(H, I, int(gate_up_block_cols), down_scale_mode, br, bc, T, top_k, E,
                                                              _DT.get(dtype, -1)))


def _moe_fp8_grouped_check(what: str, x: torch.Tensor, weight_t: torch.Tensor, rscale: torch.Tensor, E: int, w_bytes: int, n_scales: int):
    """_moe_fp8_check on a grouped stage, whose input has no ids / status beside it."""
    if x.dtype not in _DT or x.dim() != 2 or not x.is_contiguous():
        raise RuntimeError(f"{what}: input must be a contiguous 16-bit 2-D tensor (got {x.dtype} {tuple(x.shape)})")
    _moe_fp8_stacked_check(what, weight_t, rscale, E, w_bytes, n_scales)


def moe_fp8_gate_up_grouped(x: torch.Tensor, weight_t: torch.Tensor, rscale: torch.Tensor, sorted_slots: torch.Tensor, unit_expert: torch.Tensor,
                            num_units: torch.Tensor, act: torch.Tensor, top_k: int, E: int, I: int, block_cols: int = 0) -> torch.Tensor:
    """Stage one on the sorted slots (gptqhip_moe_fp8_gate_up_grouped): act[s, :I] of every slot in a unit, the rounding chain of
    moe_fp8_gate_up.  x [T, H]; weight_t / rscale: the stacked buffers of moe_fp8_gate_up; act: >= T * top_k * I elements of x.dtype (rows of
    slots in no unit are left untouched)."""
    _require_cuda(x, weight_t, rscale, sorted_slots, unit_expert, num_units, act)
    bc = int(block_cols)
    H = x.shape[-1]
    _moe_fp8_grouped_check("moe_fp8_gate_up_grouped", x, weight_t, rscale, E, 2 * I * H, 2 * I * (H // bc if bc > 0 else 1))
    T = x.shape[0]
    _moe_sort_check("moe_fp8_gate_up_grouped", T * top_k, E, sorted_slots, unit_expert, num_units)
    if act.dtype != x.dtype or act.numel() < T * top_k * I or not act.is_contiguous():
        raise RuntimeError(f"moe_fp8_gate_up_grouped: act must be a contiguous {x.dtype} tensor with >= {T * top_k * I} elements")
    with torch.cuda.device(x.device):
        rc = _lib.load().gptqhip_moe_fp8_gate_up_grouped(_ptr(x), _ptr(weight_t), _ptr(rscale), _ptr(sorted_slots), _ptr(unit_expert),
                                                         _ptr(num_units), _ptr(act), T, top_k, E, H, I, bc, _DT[x.dtype], _stream(x.device))
    _lib.check(rc, "gptqhip_moe_fp8_gate_up_grouped")
    return act


def moe_fp8_down_grouped(act: torch.Tensor, weight_t: torch.Tensor, rscale: torch.Tensor, sorted_slots: torch.Tensor, unit_expert: torch.Tensor,
                         num_units: torch.Tensor, part: torch.Tensor, top_k: int, E: int, H: int, scale_mode: int, block_size=None) -> torch.Tensor:
    """Stage two on the sorted slots (gptqhip_moe_fp8_down_grouped): part[s, :H] = act[s] @ the down weight of the slot's expert, UNROUNDED fp32
    with the reciprocal scales applied; moe_combine finishes it.  act [T * top_k, I]; weight_t / rscale: the stacked buffers of moe_fp8_down;
    part: >= T * top_k * H float32 elements."""
    _require_cuda(act, weight_t, rscale, sorted_slots, unit_expert, num_units, part)
    br, bc = _fp8_block(scale_mode, block_size)
    I = act.shape[-1]
    _moe_fp8_grouped_check("moe_fp8_down_grouped", act, weight_t, rscale, E, I * H, _fp8_scale_count(I, H, scale_mode, br, bc))
    S = act.shape[0]
    if top_k < 1 or S % top_k != 0:
        raise RuntimeError(f"moe_fp8_down_grouped: act must have T * top_k rows (got {S} rows, top_k = {top_k})")
    _moe_sort_check("moe_fp8_down_grouped", S, E, sorted_slots, unit_expert, num_units)
    if part.dtype != torch.float32 or part.numel() < S * H or not part.is_contiguous():
        raise RuntimeError(f"moe_fp8_down_grouped: part must be a contiguous float32 tensor with >= {S * H} elements")
    with torch.cuda.device(act.device):
        rc = _lib.load().gptqhip_moe_fp8_down_grouped(_ptr(act), _ptr(weight_t), _ptr(rscale), _ptr(sorted_slots), _ptr(unit_expert),
                                                      _ptr(num_units), _ptr(part), S // top_k, top_k, E, H, I, scale_mode, br, bc, _DT[act.dtype],
                                                      _stream(act.device))
    _lib.check(rc, "gptqhip_moe_fp8_down_grouped")
    return part


def dequant(qweight, qzeros, scales, g_idx, group_size: int, bits: int, out_dtype=None) -> torch.Tensor:
    """[K,N] weights from the CHECKPOINT layout (bit-exact with the reference's dequantize_weight())."""
    lib = _lib.load()
    _require_cuda(qweight, qzeros, scales, g_idx)
    pf = 32 // bits
    K, N = qweight.shape[0] * pf, qweight.shape[1]
    out_dtype = out_dtype or scales.dtype
    out = torch.empty((K, N), dtype=out_dtype, device=qweight.device)
    with torch.cuda.device(qweight.device):
        rc = lib.gptqhip_dequant(_ptr(qweight), _ptr(qzeros), _ptr(scales), _ptr(g_idx), _ptr(out), K, N, group_size,
                                 bits, _DT[scales.dtype], _DT[out_dtype], _stream(qweight.device))
    _lib.check(rc, "gptqhip_dequant")
    return out


def dequant_tiled(qweight_t, meta, perm, K: int, N: int, group_size: int, bits: int, scale_dtype, out_dtype=None):
    """[K,N] weights from the TILED layout; rows come back in checkpoint order when perm is given."""
    lib = _lib.load()
    _require_cuda(qweight_t, meta, perm)
    out_dtype = out_dtype or scale_dtype
    out = torch.empty((K, N), dtype=out_dtype, device=qweight_t.device)
    with torch.cuda.device(qweight_t.device):
        rc = lib.gptqhip_dequant_tiled(_ptr(qweight_t), _ptr(meta), _ptr(perm), _ptr(out), K, N, group_size, bits,
                                       _DT[scale_dtype], _DT[out_dtype], _stream(qweight_t.device))
    _lib.check(rc, "gptqhip_dequant_tiled")
    return out


PLANAR_ONLY_BITS = (5, 6, 7)


def kernel_bits(bits: int) -> int:
    """Field width of the layout the kernels read for a checkpoint of `bits`-bit codes (gptqhip_widen_codes)."""
    return 4 if bits <= 4 else 8


def widen_codes(qweight: torch.Tensor, qzeros: torch.Tensor, bits: int, planar: Optional[bool] = None):
    """(qweight, qzeros) of a 2 / 3 / 5 / 6 / 7-bit checkpoint -> the same codes in the continuous 4- or 8-bit layout + that width."""
    lib = _lib.load()
    _require_cuda(qweight, qzeros)
    if planar is None:
        planar = bits in PLANAR_ONLY_BITS
    K, N, G = qweight.shape[0] * 32 // bits, qweight.shape[1], qzeros.shape[0]
    wide = kernel_bits(bits)
    qw = torch.empty((K * wide // 32, N), dtype=torch.int32, device=qweight.device)
    qz = torch.empty((G, N * wide // 32), dtype=torch.int32, device=qweight.device)
    with torch.cuda.device(qweight.device):
        rc = lib.gptqhip_widen_codes(_ptr(qweight.contiguous()), _ptr(qzeros.contiguous()), _ptr(qw), _ptr(qz), K, N, G, bits,
                                     1 if planar else 0, _stream(qweight.device))
    _lib.check(rc, "gptqhip_widen_codes")
    return qw, qz, wide


def repack_awq(qweight_awq: torch.Tensor, qzeros_awq: torch.Tensor):
    lib = _lib.load()
    _require_cuda(qweight_awq, qzeros_awq)
    K, N = qweight_awq.shape[0], qweight_awq.shape[1] * 8
    G = qzeros_awq.shape[0]
    qw = torch.empty((K // 8, N), dtype=torch.int32, device=qweight_awq.device)
    qz = torch.empty_like(qzeros_awq)
    with torch.cuda.device(qweight_awq.device):
        rc = lib.gptqhip_repack_awq(_ptr(qweight_awq.contiguous()), _ptr(qzeros_awq.contiguous()), _ptr(qw), _ptr(qz),
                                    K, N, G, _stream(qweight_awq.device))
    _lib.check(rc, "gptqhip_repack_awq")
    return qw, qz


def embedding(ids: torch.Tensor, qweight_t: torch.Tensor, meta: torch.Tensor, inv_perm: Optional[torch.Tensor],
              K: int, N: int, group_size: int, bits: int, scale_dtype: torch.dtype) -> torch.Tensor:
    """Rows ids[...] of the dequantised [K,N] matrix (tiled layout) in the scales dtype; raises IndexError on ids
    outside [0, K) like torch.nn.functional.embedding."""
    lib = _lib.load()
    _require_cuda(ids, qweight_t, meta, inv_perm)
    flat = ids.reshape(-1).to(torch.int64).contiguous()
    T = flat.numel()
    out = torch.empty((T, N), dtype=scale_dtype, device=qweight_t.device)
    status = torch.zeros(1, dtype=torch.int32, device=qweight_t.device)
    with torch.cuda.device(qweight_t.device):
        for t0 in range(0, T, 65535):
            t1 = min(T, t0 + 65535)
            rc = lib.gptqhip_embedding(_ptr(flat[t0:t1]), _ptr(qweight_t), _ptr(meta), _ptr(inv_perm), _ptr(out[t0:t1]),
                                       _ptr(status), t1 - t0, K, N, group_size, bits, _DT[scale_dtype],
                                       _stream(qweight_t.device))
            _lib.check(rc, "gptqhip_embedding")
    if int(status.item()) != 0:
        raise IndexError("index out of range in quantised embedding lookup")
    return out.reshape(tuple(ids.shape) + (N,))


def pack_gptq(weight: torch.Tensor, scales: torch.Tensor, zeros: torch.Tensor, g_idx: torch.Tensor, bits: int, planar: Optional[bool] = None):
    """Device quantise-and-pack: weight [N,K], scales [G,N], zeros [G,N], g_idx [K] -> (qweight, qzeros) in the
    checkpoint layout, bit-exact with the reference's pack_block.  bits 2..8; planar: split-plane words (default: the bit
    width's own layout -- 5 / 6 / 7 bits are planar, 3 bits only under FORMAT.GPTQ_P)."""
    lib = _lib.load()
    _require_cuda(weight, scales, zeros, g_idx)
    N, K = weight.shape
    G = scales.shape[0]
    if planar is None:
        planar = bits in PLANAR_ONLY_BITS
    w = weight.to(torch.float32).contiguous()
    s = scales.to(torch.float32).contiguous()
    z = zeros.to(torch.int32).contiguous()
    gi = g_idx.to(torch.int32).contiguous()
    if gi.numel() != K:
        raise ValueError(f"g_idx length {gi.numel()} != in_features {K}")
    gn = torch.where(gi < 0, gi + G, gi)
    if gn.numel() and (int(gn.min()) < 0 or int(gn.max()) >= G):
        raise IndexError(f"pack_gptq: g_idx values out of range (groups={G})")
    qweight = torch.empty((K * bits // 32, N), dtype=torch.int32, device=weight.device)
    qzeros = torch.empty((G, N * bits // 32), dtype=torch.int32, device=weight.device)
    with torch.cuda.device(weight.device):
        rc = lib.gptqhip_pack_gptq(_ptr(w), _ptr(s), _ptr(z), _ptr(gi), _ptr(qweight), _ptr(qzeros), K, N, G, bits,
                                   1 if planar else 0, _stream(weight.device))
    _lib.check(rc, "gptqhip_pack_gptq")
    return qweight, qzeros


def pack_gptq_host(weight: torch.Tensor, scales: torch.Tensor, zeros: torch.Tensor, g_idx: torch.Tensor, bits: int,
                   threads: int = 0, planar: Optional[bool] = None):
    """Host (CPU tensors) quantise-and-pack through the library's threaded C++ packer -- the equivalent of the
    reference's native pack_block_cpu.  Same contract as pack_gptq; needs no GPU."""
    lib = _lib.load()
    for t in (weight, scales, zeros, g_idx):
        if t.is_cuda:
            raise RuntimeError("pack_gptq_host takes CPU tensors (use pack_gptq on the device)")
    N, K = weight.shape
    G = scales.shape[0]
    if planar is None:
        planar = bits in PLANAR_ONLY_BITS
    w = weight.to(torch.float32).contiguous()
    s = scales.to(torch.float32).contiguous()
    z = zeros.to(torch.int32).contiguous()
    gi = g_idx.to(torch.int32).contiguous()
    if gi.numel() != K:
        raise ValueError(f"g_idx length {gi.numel()} != in_features {K}")
    qweight = torch.empty((K * bits // 32, N), dtype=torch.int32)
    qzeros = torch.empty((G, N * bits // 32), dtype=torch.int32)
    rc = lib.gptqhip_pack_gptq_host(_ptr(w), _ptr(s), _ptr(z), _ptr(gi), _ptr(qweight), _ptr(qzeros), K, N, G, bits,
                                    1 if planar else 0, threads)
    _lib.check(rc, "gptqhip_pack_gptq_host")
    return qweight, qzeros


def gather_cols(x: torch.Tensor, perm: torch.Tensor) -> torch.Tensor:
    lib = _lib.load()
    _require_cuda(x, perm)
    M, K = x.shape
    out = torch.empty_like(x)
    with torch.cuda.device(x.device):
        rc = lib.gptqhip_gather_cols(_ptr(x), _ptr(perm), _ptr(out), M, K, _stream(x.device))
    _lib.check(rc, "gptqhip_gather_cols")
    return out


def rmsnorm_gather(h: torch.Tensor, weight: torch.Tensor, eps: float, perm: Optional[torch.Tensor] = None,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """HF LlamaRMSNorm over the last dimension fused with an act-order gather: out[.., k'] = weight[p] * act(h32[.., p] * rsqrt(mean
    h32^2 + eps)), p = perm[k'] (perm None: plain RMSNorm).  Feed the result to HipGptqLinear.forward_pregathered of the q|k|v or
    gate|up module whose `perm` this is: the linear then needs no gather pass of its own."""
    lib = _lib.load()
    _require_cuda(h, weight)
    if h.dtype not in _DT or weight.dtype != h.dtype or not h.is_contiguous() or not weight.is_contiguous():
        raise RuntimeError("rmsnorm_gather: h and weight must be contiguous fp16 / bf16 tensors of the same dtype")
    K = h.shape[-1]
    M = h.numel() // K
    if weight.numel() != K or (perm is not None and (perm.dtype != torch.int32 or perm.numel() != K or not perm.is_contiguous())):
        raise RuntimeError("rmsnorm_gather: weight / perm must have K elements (perm int32)")
    if out is None:
        out = torch.empty_like(h)
    elif out.shape != h.shape or out.dtype != h.dtype or not out.is_contiguous() or out.data_ptr() == h.data_ptr():
        raise RuntimeError("rmsnorm_gather: out must be a distinct contiguous tensor like h")
    with torch.cuda.device(h.device):
        rc = lib.gptqhip_rmsnorm_gather(_ptr(h), _ptr(weight), _ptr(perm), _ptr(out), M, K, float(eps), _DT[h.dtype], _stream(h.device))
    _lib.check(rc, "gptqhip_rmsnorm_gather")
    return out


def plan_describe(M: int, K: int, N: int, group_size: int, bits: int = 4, has_perm: bool = False) -> str:
    """Kernel family + launch geometry gptqhip_gemm would pick for this call (host logic; needs no GPU)."""
    import ctypes
    buf = ctypes.create_string_buffer(256)
    _lib.check(_lib.load().gptqhip_plan_describe(M, K, N, group_size, bits, 1 if has_perm else 0, buf, 256), "gptqhip_plan_describe")
    return buf.value.decode()


def set_tuning(force_split_k: int = 0, force_kernel: int = 0, force_waves: int = 0) -> None:
    _need_cache.clear()  # forced plans change the workspace layout
    _lib.check(_lib.load().gptqhip_set_tuning(force_split_k, force_kernel, force_waves), "gptqhip_set_tuning")


def set_decode_form(form: int = -1) -> None:
    """Batch-1 decode form for the calling thread (include/gptqhip.h gptqhip_set_decode_form documents all six): 5 = preload kernel + raw codes
    as fp16 denormals (the default for fp16 and bf16 activations), 3 = preload + group-factored dequant, 4 = preload + the reference's per-weight
    rounding (bit-faithful; the default for fp16 activations with bf16 scales), 0 / 2 = the rounds 1-5 kernel (bit-faithful / group-factored), 1 = the LDS-DMA stream kernel (opt-in, slower),
    -1 = the process default (GPTQHIP_DECODE_BITFAITHFUL=1 in the environment makes that 4 for every dtype)."""
    _lib.check(_lib.load().gptqhip_set_decode_form(form), "gptqhip_set_decode_form")
