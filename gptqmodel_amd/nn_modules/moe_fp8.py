"""HipFp8MoeExperts: the experts of an FP8 (float8_e4m3fn, weight-only) sparse mixture-of-experts block on the fused FP8 MoE decode ops.

Block-scaled FP8 checkpoints (Qwen3-30B-A3B-FP8, the DeepSeek-V3 family: weight_block_size [128, 128]) are sparse-MoE models whose experts
load as three HipFp8Linear modules each and run through the HF host-routed loop: a nonzero() host sync per layer, three launches and an
index_add_ per active expert, no graph capture.  This module holds ALL experts' kernel-layout bytes and reciprocal scales stacked in two
buffers per projection and serves the call signature of transformers' experts modules, like nn_modules/moe.py does for 4-bit GPTQ experts:

    forward(hidden_states [T, H], top_k_index [T, k], top_k_weights [T, k]) -> [T, H]

Stacked layout (fixed by from_linears, on the device):
  gate_up_weight uint8 [E, 2I * H]   per expert the [2I, H] weight whose ROWS interleave gate and up in blocks of 8 (fused rows 16 t .. 16 t + 7 =
                                     gate rows 8 t .. 8 t + 7, fused rows 16 t + 8 .. 16 t + 15 = up rows 8 t .. 8 t + 7: the rule of
                                     fuse_gate_up_interleaved), in the layout of gptqhip_fp8_repack
  gate_up_rscale fp32                ONE SCALE ROW PER FUSED COLUMN: [E, 2I] from tensor and row sources, [E, 2I, H / bc] from (br, bc) block
                                     sources -- what gptqhip_fp8_gemm takes as block (1, bc).  With bc = 128 that is 64 B of scales per 2 KiB of
                                     weights (3 %); it buys one indexing rule in the kernel and a slow path that calls fp8_gemm on a view.
  down_weight uint8 [E, I * H], down_rscale fp32 [E, 1] | [E, H] | [E, H / br, I / bc]: the module's native layout, not interleaved.
The reciprocals are the ones gptqhip_fp8_repack forms (IEEE fp32 division, once).

The call checks, the device-routed fast path, the grouped path's window, buffers and capture rule, the status word and the host-routed slow path are
StackedMoeExperts' (nn_modules/moe_base.py, which states the rounding contract); this module adds the FP8 stacking and:

* fast path (ops.moe_fp8_supported: H % 128 == 0, I % 128 == 0, T <= 16, top_k <= 16, fp16 | bf16): gptqhip_moe_fp8_gate_up + gptqhip_moe_fp8_down.
* grouped path (ops.moe_fp8_grouped_supported: the same shapes and scale layouts at ANY T, top_k <= 16, E <= 512, T * top_k <= 65536):
  gptqhip_moe_align + gptqhip_moe_fp8_gate_up_grouped + gptqhip_moe_fp8_down_grouped + gptqhip_moe_combine on the same stacked buffers.  Taken
  when `grouped_routing` is set and grouped_min_tokens <= T <= grouped_max_tokens (off by default; GPTQHIP_MOE_GROUPED=1 at construction turns
  it on), and for T > 16 under stream capture: FP8 MoE prefill and large-batch decode inside torch.cuda.graph.  Same contract as the fast path,
  another K summation order: the two agree within the bar, not bit for bit.
* slow path (more tokens with the flag off, other dtypes): the host-routed per-expert loop of the HF module on ops.fp8_gemm over views into the
  same stacked buffers -- arithmetically what a loop over the original HipFp8Linear modules does."""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple

import torch
import torch.nn as nn

from .. import ops
from .moe_base import MAX_FAST_TOKENS, StackedMoeExperts

# eager window of the grouped path when grouped_routing is set, MEASURED (profiles/r14_moe_fp8_grouped.txt, the rule of 4.4.1):
# the smallest T from which grouped eager is not slower than the few-token ops on Qwen3-30B-A3B and Mixtral-8x7B, and the largest measured T at
# which it is not slower than the host loop on both (on Mixtral the two meet there).  tests/dev/moe_fp8_grouped_probe.py prints both.
GROUPED_MIN_TOKENS = 16
GROUPED_MAX_TOKENS = 1024


def interleave_rows8(gate: torch.Tensor, up: torch.Tensor) -> torch.Tensor:
    """[I, ...] x 2 -> [2I, ...]: rows in alternating blocks of 8 (g0..g7, u0..u7, g8..g15, ...), the order fuse_gate_up_interleaved gives the
    output columns of a fused gate|up projection."""
    n = gate.shape[0]
    rest = tuple(gate.shape[1:])
    return torch.stack((gate.reshape((n // 8, 8) + rest), up.reshape((n // 8, 8) + rest)), dim=1).reshape((2 * n,) + rest)


def _interleave_tiled(gate: torch.Tensor, up: torch.Tensor, tiles: int, inner: int) -> torch.Tensor:
    """The same interleave on two arrays ALREADY in the FP8 kernel layout ([tile][chunk][half][rq][c][16 bytes]; inner = chunks * 2): fused tile
    2 t + h takes columns 8 h .. 8 h + 7 of gate tile t as its columns 0 .. 7 and those of up tile t as 8 .. 15."""
    g = gate.view(tiles, inner, 4, 2, 8, 16)
    u = up.view(tiles, inner, 4, 2, 8, 16)
    out = torch.empty((tiles, 2, inner, 4, 2, 8, 16), dtype=gate.dtype, device=gate.device)
    out[:, :, :, :, 0] = g.permute(0, 3, 1, 2, 4, 5)
    out[:, :, :, :, 1] = u.permute(0, 3, 1, 2, 4, 5)
    return out.view(-1)


def _scale_rows(s: torch.Tensor, method: str, block: Optional[Tuple[int, int]], n: int) -> torch.Tensor:
    """A [N, K] projection's scales (scale_inv or their reciprocals) in its own layout -> one scale row per weight row: [n] (tensor, row) or
    [n, K / bc] (block)."""
    if method == "tensor":
        return s.reshape(1).expand(n)
    if method == "row":
        return s.reshape(n)
    return s.repeat_interleave(block[0], dim=0)


class HipFp8MoeExperts(StackedMoeExperts):
    _SOURCE_KIND = "HIP FP8 linear"
    _RELEASE_NAMES = ("weight", "weight_scale_inv", "rscale")
    GROUPED_WINDOW = (GROUPED_MIN_TOKENS, GROUPED_MAX_TOKENS)

    def __init__(self, num_experts: int, hidden_dim: int, intermediate_dim: int, gate_up_scale_method: str,
                 gate_up_block_size: Optional[Tuple[int, int]], down_scale_method: str, down_block_size: Optional[Tuple[int, int]]):
        super().__init__(num_experts, hidden_dim, intermediate_dim)
        self.fp8_format = "float8_e4m3fn"
        self.gate_up_scale_method = gate_up_scale_method      # of the source modules; the stacked scales are row or block (1, bc)
        self.gate_up_block_size = gate_up_block_size
        self.down_scale_method = down_scale_method
        self.down_block_size = down_block_size
        self.gate_up_block_cols = gate_up_block_size[1] if gate_up_scale_method == "block" else 0

    @staticmethod
    def _is_source(m) -> bool:
        return bool(getattr(m, "_GPTQHIP_KERNEL_CLASS", False)) and getattr(m, "QUANT_TYPE", "") == "hip_fp8"

    def _layout_repr(self, method, block) -> str:
        return f"block{tuple(block)}" if method == "block" else method

    def extra_repr(self) -> str:
        return (f"experts={self.num_experts}, hidden={self.hidden_dim}, intermediate={self.intermediate_dim}, format={self.fp8_format}, "
                f"gate_up_scales={self._layout_repr(self.gate_up_scale_method, self.gate_up_block_size)}, "
                f"down_scales={self._layout_repr(self.down_scale_method, self.down_block_size)}")

    # the stacked gate|up scales as gptqhip_fp8_gemm / gptqhip_fp8_dequant name them
    def _gate_up_mode(self):
        if self.gate_up_block_cols:
            return ops.FP8_SCALE_BLOCK, (1, self.gate_up_block_cols)
        return ops.FP8_SCALE_ROW, None

    def _down_mode(self):
        return ops.FP8_SCALE_MODES[self.down_scale_method], self.down_block_size

    # ---------------------------------------------------------------------------------------------------------------------------
    @classmethod
    def from_linears(cls, gate: Sequence[nn.Module], up: Sequence[nn.Module], down: Sequence[nn.Module]) -> "HipFp8MoeExperts":
        """Three equal-length lists of HipFp8Linear (expert e = gate[e], up[e], down[e]) on the ROCm device, either already post_init()ed
        (kernel layout) or still in the checkpoint layout.  gate | up are fused per expert with the row interleave of
        fuse_gate_up_interleaved, all experts are stacked into two contiguous buffers per projection, and the per-expert copies are
        released as they are stacked (peak extra memory: one expert).  Down may carry a different scale layout from gate / up.  Raises
        NotImplementedError when the experts cannot share the stacked layout; nothing has been modified then."""
        gate, up, down = cls._check_lists(gate, up, down)
        E, g0, d0 = len(gate), gate[0], down[0]
        if not cls._is_source(g0) or not cls._is_source(d0):
            raise NotImplementedError(f"expert 0: {type(g0).__name__} / {type(d0).__name__} is not a HIP FP8 linear")
        H, I = g0.in_features, g0.out_features
        for e in range(E):
            for m, (k, n), ref in ((gate[e], (H, I), g0), (up[e], (H, I), g0), (down[e], (I, H), d0)):
                cls._check_module(e, m, k, n)
                if m.fp8_format != "float8_e4m3fn" or (not m._ready and m.weight.dtype != torch.float8_e4m3fn):
                    raise NotImplementedError(f"expert {e}: {m.fp8_format} / {m.weight.dtype} weights (float8_e4m3fn only)")
                if m.weight_scale_method != ref.weight_scale_method or m.weight_block_size != ref.weight_block_size:
                    raise NotImplementedError(f"expert {e}: scale method / block size {m.weight_scale_method} {m.weight_block_size} differ from "
                                              f"{ref.weight_scale_method} {ref.weight_block_size}")
                if m._ready != g0._ready:
                    raise NotImplementedError(f"expert {e}: a mix of post_init()ed and checkpoint-layout modules")
                if m.weight.numel() != k * n or tuple(m.weight_scale_inv.shape) != m._scale_shape():
                    raise NotImplementedError(f"expert {e}: buffer shapes do not match the module")
        if not all(m.weight.is_cuda and m.weight_scale_inv.is_cuda for m in gate + up + down):
            raise NotImplementedError("buffers must be on the ROCm device")
        gu_bc = g0.weight_block_size[1] if g0.weight_scale_method == "block" else 0
        d_mode = ops.FP8_SCALE_MODES[d0.weight_scale_method]
        if not ops.moe_fp8_supported(H, I, gu_bc, d_mode, d0.weight_block_size, 1, 1, torch.float16):
            raise NotImplementedError(f"experts {H} x {I} with gate/up {g0.weight_scale_method} {g0.weight_block_size} and down "
                                      f"{d0.weight_scale_method} {d0.weight_block_size} scales are outside the fused FP8 MoE ops")
        self = cls(E, H, I, g0.weight_scale_method, g0.weight_block_size, d0.weight_scale_method, d0.weight_block_size)
        dev = g0.weight.device
        gu_mode, gu_block = self._gate_up_mode()
        gu_scales = 2 * I * (H // gu_bc if gu_bc else 1)
        bufs = [torch.empty((E, 2 * I * H), dtype=torch.uint8, device=dev), torch.empty((E, gu_scales), dtype=torch.float32, device=dev),
                torch.empty((E, I * H), dtype=torch.uint8, device=dev), torch.empty((E, max(d0.weight_scale_inv.numel(), 1)), dtype=torch.float32, device=dev)]
        method, block = g0.weight_scale_method, g0.weight_block_size
        ready = g0._ready
        for e in range(E):
            g, u, d = gate[e], up[e], down[e]
            if ready:
                bufs[0][e] = _interleave_tiled(g.weight.data.view(torch.uint8).reshape(-1), u.weight.data.view(torch.uint8).reshape(-1), I // 16,
                                               (H // 128) * 2)
                bufs[1][e] = interleave_rows8(_scale_rows(g.rscale, method, block, I), _scale_rows(u.rscale, method, block, I)).reshape(-1)
                bufs[2][e], bufs[3][e] = d.weight.data.view(torch.uint8).reshape(-1), d.rscale.reshape(-1)
            else:
                w = interleave_rows8(g.weight.data.view(torch.uint8), u.weight.data.view(torch.uint8))
                s = interleave_rows8(_scale_rows(g.weight_scale_inv.data.float(), method, block, I),
                                     _scale_rows(u.weight_scale_inv.data.float(), method, block, I))
                w_t, rs = ops.fp8_repack(w, s, gu_mode, gu_block)
                bufs[0][e], bufs[1][e] = w_t, rs.reshape(-1)
                del w, s, w_t, rs
                w_t, rs = ops.fp8_repack(d.weight.data, d.weight_scale_inv.data, d_mode, d0.weight_block_size)
                bufs[2][e], bufs[3][e] = w_t, rs.reshape(-1)
                del w_t, rs
            for m in (g, u, d):
                cls._release(m)
        bufs[1] = bufs[1].view((E, 2 * I, H // gu_bc) if gu_bc else (E, 2 * I))
        bufs[3] = bufs[3].view((E,) + (tuple(d0._scale_shape()) or (1,)))
        for name, t in zip(("gate_up_weight", "gate_up_rscale", "down_weight", "down_rscale"), bufs):
            self.register_buffer(name, t, persistent=False)
        self.register_buffer("status", torch.zeros(1, dtype=torch.int32, device=dev), persistent=False)
        return self

    # ---------------------------------------------------------------------------------------------------------------------------
    def expert_view(self, e: int, projection: str):
        """(weight_t, rscale, scale_mode, block_size, K, N) of expert e's `gate_up` | `down` projection as ops.fp8_gemm / ops.fp8_dequant take
        them: views into the stacked buffers.  Those ops want 16-byte aligned scales, the fused kernels only 4 bytes: an expert's scales that
        start off a 16-byte boundary (a tensor scale, a handful of blocks) are handed out as a copy."""
        H, I = self.hidden_dim, self.intermediate_dim
        if projection == "gate_up":
            w, rs, (mode, block), K, N = self.gate_up_weight[e], self.gate_up_rscale[e], self._gate_up_mode(), H, 2 * I
        else:
            w, rs, (mode, block), K, N = self.down_weight[e], self.down_rscale[e], self._down_mode(), I, H
        rs = rs.reshape(-1)
        if rs.data_ptr() % 16 != 0:
            rs = rs.clone()
        return w, rs, mode, block, K, N

    def fast_path(self, T: int, top_k: int, dtype: torch.dtype) -> bool:
        """Whether forward() serves this call with the two fused launches."""
        key = (T, top_k)
        ok = self._fast_ok.get(key)
        if ok is None:
            mode, block = self._down_mode()
            ok = ops.moe_fp8_supported(self.hidden_dim, self.intermediate_dim, self.gate_up_block_cols, mode, block, T, top_k, torch.float16)
            self._fast_ok[key] = ok
        return ok and dtype in (torch.float16, torch.bfloat16)

    def grouped_path(self, T: int, top_k: int, dtype: torch.dtype) -> bool:
        """Whether the expert-grouped ops can serve this call (the shape predicate; forward() takes them only inside the grouped_routing window
        or under stream capture)."""
        key = (T, top_k)
        ok = self._grouped_ok.get(key)
        if ok is None:
            mode, block = self._down_mode()
            ok = ops.moe_fp8_grouped_supported(self.hidden_dim, self.intermediate_dim, self.gate_up_block_cols, mode, block, T, top_k,
                                               self.num_experts, torch.float16)
            self._grouped_ok[key] = ok
        return ok and dtype in (torch.float16, torch.bfloat16)

    def _grouped_gate_up(self, x: torch.Tensor, b: Dict, act: torch.Tensor, top_k: int) -> None:
        ops.moe_fp8_gate_up_grouped(x, self.gate_up_weight, self.gate_up_rscale, b["sorted"], b["unit_expert"], b["num_units"], act, top_k,
                                    self.num_experts, self.intermediate_dim, self.gate_up_block_cols)

    def _grouped_down(self, act: torch.Tensor, b: Dict, part: torch.Tensor, top_k: int) -> None:
        mode, block = self._down_mode()
        ops.moe_fp8_down_grouped(act, self.down_weight, self.down_rscale, b["sorted"], b["unit_expert"], b["num_units"], part, top_k,
                                 self.num_experts, self.hidden_dim, mode, block)

    def _fused_gate_up(self, x: torch.Tensor, ids: torch.Tensor, act: torch.Tensor) -> None:
        ops.moe_fp8_gate_up(x, self.gate_up_weight, self.gate_up_rscale, ids, act, self.status, self.num_experts, self.intermediate_dim,
                            self.gate_up_block_cols)

    def _fused_down(self, act: torch.Tensor, ids: torch.Tensor, w: torch.Tensor, out: torch.Tensor) -> None:
        mode, block = self._down_mode()
        ops.moe_fp8_down(act, self.down_weight, self.down_rscale, ids, w, out, self.status, self.num_experts, mode, block)

    def _expert_gemm(self, e: int, projection: str, x: torch.Tensor) -> torch.Tensor:
        w, rs, mode, block, _, N = self.expert_view(e, projection)
        return ops.fp8_gemm(x, w, rs, None, N, mode, block)


__all__ = ["HipFp8MoeExperts", "MAX_FAST_TOKENS", "interleave_rows8"]
