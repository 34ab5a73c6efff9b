"""HipMoeExperts: the experts of a sparse mixture-of-experts block on the fused MoE decode ops.

GPTQModel quantises MoE checkpoints per expert (three GPTQ linears each) and leaves the execution to the HF modeling code: a host-routed
loop (one_hot + nonzero() / where() on the router output, i.e. a device-to-host sync per layer) with three QuantLinear.forward calls and an
index_add_ per active expert.  This module holds ALL experts' tiled words / constants stacked in two buffers per projection and serves the
call signature of transformers' experts modules (Qwen3MoeExperts.forward / MixtralExperts.forward):

    forward(hidden_states [T, H], top_k_index [T, k], top_k_weights [T, k]) -> [T, H]

The call checks, the device-routed fast path, the grouped path's window, buffers and capture rule, the status word and the host-routed slow path are
StackedMoeExperts' (nn_modules/moe_base.py, which states the rounding contract); this module adds the 4-bit stacking and:

* fast path (ops.moe_supported: 4 bits, group_size = 128 * 2^n, no act-order, T <= 16, top_k <= 16): gptqhip_moe_gate_up + gptqhip_moe_down.
* grouped path (ops.moe_grouped_supported: the same shapes at ANY T): gptqhip_moe_align + gptqhip_moe_gate_up_grouped + gptqhip_moe_down_grouped
  + gptqhip_moe_combine -- the slots sorted by expert on the device, every 16-row unit of one expert on the matrix pipe, the same combine
  contract (one fp32 weighted sum in slot order, one rounding), the same status word, no host synchronisation.  Taken when `grouped_routing`
  is set and grouped_min_tokens <= T <= grouped_max_tokens (off by default; GPTQHIP_MOE_GROUPED=1 at construction turns it on), and for
  T > 16 under stream capture, where the host-routed loop cannot run at all.
* slow path (more tokens, other shapes): the host-routed per-expert loop of the HF module on ops.gemm over views into the same stacked
  buffers -- arithmetically what a loop over the original modules does.
"""
from __future__ import annotations

from typing import Dict, Sequence

import torch
import torch.nn as nn

from .. import _lib, ops
from ..utils.model import fuse_gate_up_interleaved
from .moe_base import MAX_FAST_TOKENS, StackedMoeExperts

# eager window of the grouped path when grouped_routing is set.  NOT measured yet: the first T the ungrouped ops do not serve,
# and the ops' slot limit; tests/dev/moe_grouped_probe.py prints the values the measurement rule gives.
GROUPED_MIN_TOKENS = 17
GROUPED_MAX_TOKENS = 65536


def _interleave_tiled(gate: torch.Tensor, up: torch.Tensor, tiles: int, inner: int, per_lane: int) -> torch.Tensor:
    """Column-interleave two TILED arrays in blocks of 8 (what fuse_gate_up_interleaved + post_init produce from the checkpoint layout):
    fused tile 2 t + h takes columns 8 h .. 8 h + 7 of gate tile t as its columns 0 .. 7 and those of up tile t as 8 .. 15.
    words: [tile][chunk][rq][c][j] -> inner = chunks * 4, per_lane = 4; meta: [tile][group][c] -> inner = groups, per_lane = 1."""
    g = gate.view(tiles, inner, 2, 8, per_lane)
    u = up.view(tiles, inner, 2, 8, per_lane)
    out = torch.empty((tiles, 2, inner, 2, 8, per_lane), dtype=gate.dtype, device=gate.device)
    out[:, :, :, 0] = g.permute(0, 2, 1, 3, 4)
    out[:, :, :, 1] = u.permute(0, 2, 1, 3, 4)
    return out.view(-1)


class HipMoeExperts(StackedMoeExperts):
    _SOURCE_KIND = "HIP GPTQ linear"
    _RELEASE_NAMES = ("qweight", "qzeros", "scales", "g_idx", "meta")
    GROUPED_WINDOW = (GROUPED_MIN_TOKENS, GROUPED_MAX_TOKENS)

    def __init__(self, num_experts: int, hidden_dim: int, intermediate_dim: int, gate_up_group_size: int, down_group_size: int,
                 scale_dtype: torch.dtype):
        super().__init__(num_experts, hidden_dim, intermediate_dim)
        self.gate_up_group_size = gate_up_group_size
        self.down_group_size = down_group_size
        self.scale_dtype = scale_dtype
        self.bits = 4

    @staticmethod
    def _is_source(m) -> bool:
        return getattr(m, "_GPTQHIP_KERNEL_CLASS", False) and getattr(m, "QUANT_TYPE", "") == "hip_gptq"

    def extra_repr(self) -> str:
        return (f"experts={self.num_experts}, hidden={self.hidden_dim}, intermediate={self.intermediate_dim}, bits=4, "
                f"group_size={self.gate_up_group_size}/{self.down_group_size}")

    # ---------------------------------------------------------------------------------------------------------------------------
    @classmethod
    def from_linears(cls, gate: Sequence[nn.Module], up: Sequence[nn.Module], down: Sequence[nn.Module]) -> "HipMoeExperts":
        """Three equal-length lists of HIP GPTQ linears (expert e = gate[e], up[e], down[e]) on the ROCm device, either already
        post_init()ed (tile-major) or still in the checkpoint layout (then post_init() runs here).  gate | up are fused per expert with
        the column interleave of fuse_gate_up_interleaved, all experts are stacked into two contiguous buffers per projection, and the
        per-expert copies are released as they are stacked (peak extra memory: one expert).  Raises NotImplementedError when the experts
        cannot share the stacked layout; nothing has been modified then."""
        gate, up, down = cls._check_lists(gate, up, down)
        E, g0, d0 = len(gate), gate[0], down[0]
        H, I = g0.in_features, g0.out_features
        for e in range(E):
            for m, (k, n) in ((gate[e], (H, I)), (up[e], (H, I)), (down[e], (I, H))):
                cls._check_module(e, m, k, n)
                if m.bits != 4 or getattr(m, "planar", False):
                    raise NotImplementedError(f"expert {e}: {m.bits}-bit codes (4-bit only)")
                if m.scales.dtype != g0.scales.dtype or m.group_size != (g0 if k == H else d0).group_size or m._ready != g0._ready:
                    raise NotImplementedError(f"expert {e}: group size / scale dtype / layout differ from expert 0")
                if not m.qweight.is_cuda:
                    raise NotImplementedError("buffers must be on the ROCm device")
                if m._ready:
                    if m.perm is not None:
                        raise NotImplementedError(f"expert {e}: act-order")
                else:
                    gi = getattr(m, "g_idx", None)
                    if gi is not None and gi.numel() == k and not torch.equal(
                            gi.long(), torch.arange(k, device=gi.device, dtype=torch.int64) // m.group_size):
                        raise NotImplementedError(f"expert {e}: act-order")
        if I % 16 != 0 or H % 16 != 0:
            raise NotImplementedError("hidden and intermediate sizes must be multiples of 16")
        self = cls(E, H, I, g0.group_size, d0.group_size, g0.scales.dtype)
        dev = g0.qweight.device
        lib = _lib.load()
        sizes = [(lib.gptqhip_tiled_words(H, 2 * I, 4), lib.gptqhip_meta_words(H, 2 * I, g0.group_size)),
                 (lib.gptqhip_tiled_words(I, H, 4), lib.gptqhip_meta_words(I, H, d0.group_size))]
        bufs = [torch.empty((E, n), dtype=torch.int32, device=dev) for pair in sizes for n in pair]
        chunks_h = -(-H // 128)
        ready = g0._ready
        for e in range(E):
            if ready:
                bufs[0][e] = _interleave_tiled(gate[e].qweight.data, up[e].qweight.data, I // 16, chunks_h * 4, 4)
                bufs[1][e] = _interleave_tiled(gate[e].meta, up[e].meta, I // 16, H // g0.group_size, 1)
            else:
                gu = fuse_gate_up_interleaved(gate[e], up[e])
                gu.post_init()
                bufs[0][e], bufs[1][e] = gu.qweight.data, gu.meta
                del gu
                down[e].post_init()
            bufs[2][e], bufs[3][e] = down[e].qweight.data, down[e].meta
            for m in (gate[e], up[e], down[e]):
                cls._release(m)
        for name, t in zip(("gate_up_qweight", "gate_up_meta", "down_qweight", "down_meta"), bufs):
            self.register_buffer(name, t, persistent=False)
        self.register_buffer("status", torch.zeros(1, dtype=torch.int32, device=dev), persistent=False)
        return self

    # ---------------------------------------------------------------------------------------------------------------------------
    def fast_path(self, T: int, top_k: int, dtype: torch.dtype) -> bool:
        """Whether forward() serves this call with the two fused launches."""
        key = (T, top_k)
        ok = self._fast_ok.get(key)
        if ok is None:
            gs = self._common_group_size()
            ok = gs != 0 and ops.moe_supported(self.hidden_dim, self.intermediate_dim, gs, self.bits, False, T, top_k)
            self._fast_ok[key] = ok
        return ok and self._dtype_ok(dtype)

    def _dtype_ok(self, dtype: torch.dtype) -> bool:
        return dtype in (torch.float16, torch.bfloat16) and not (dtype == torch.bfloat16 and self.scale_dtype == torch.float16)

    def _common_group_size(self) -> int:
        """The one group_size argument of the shape predicates: -1 = one group for the whole K of each projection, 0 = not servable."""
        gs = self.gate_up_group_size
        if gs != self.down_group_size:
            gs = -1 if (gs == self.hidden_dim and self.down_group_size == self.intermediate_dim) else 0
        return gs

    def grouped_path(self, T: int, top_k: int, dtype: torch.dtype) -> bool:
        """Whether the expert-grouped ops can serve this call (the shape predicate; forward() takes them only inside the grouped_routing window
        or under stream capture)."""
        key = (T, top_k)
        ok = self._grouped_ok.get(key)
        if ok is None:
            gs = self._common_group_size()
            ok = gs != 0 and ops.moe_grouped_supported(self.hidden_dim, self.intermediate_dim, gs, self.bits, False, T, top_k, self.num_experts)
            self._grouped_ok[key] = ok
        return ok and self._dtype_ok(dtype)

    def _grouped_gate_up(self, x: torch.Tensor, b: Dict, act: torch.Tensor, top_k: int) -> None:
        ops.moe_gate_up_grouped(x, self.gate_up_qweight, self.gate_up_meta, b["sorted"], b["unit_expert"], b["num_units"], act, top_k,
                                self.num_experts, self.intermediate_dim, self.gate_up_group_size, self.scale_dtype)

    def _grouped_down(self, act: torch.Tensor, b: Dict, part: torch.Tensor, top_k: int) -> None:
        ops.moe_down_grouped(act, self.down_qweight, self.down_meta, b["sorted"], b["unit_expert"], b["num_units"], part, top_k, self.num_experts,
                             self.hidden_dim, self.down_group_size, self.scale_dtype)

    def _fused_gate_up(self, x: torch.Tensor, ids: torch.Tensor, act: torch.Tensor) -> None:
        ops.moe_gate_up(x, self.gate_up_qweight, self.gate_up_meta, ids, act, self.status, self.num_experts, self.intermediate_dim,
                        self.gate_up_group_size, self.scale_dtype)

    def _fused_down(self, act: torch.Tensor, ids: torch.Tensor, w: torch.Tensor, out: torch.Tensor) -> None:
        ops.moe_down(act, self.down_qweight, self.down_meta, ids, w, out, self.status, self.num_experts, self.down_group_size, self.scale_dtype)

    def _expert_gemm(self, e: int, projection: str, x: torch.Tensor) -> torch.Tensor:
        if projection == "gate_up":
            return ops.gemm(x, self.gate_up_qweight[e], self.gate_up_meta[e], None, None, 2 * self.intermediate_dim, self.gate_up_group_size,
                            self.bits, self.scale_dtype)
        return ops.gemm(x, self.down_qweight[e], self.down_meta[e], None, None, self.hidden_dim, self.down_group_size, self.bits, self.scale_dtype)


__all__ = ["HipMoeExperts", "MAX_FAST_TOKENS"]
