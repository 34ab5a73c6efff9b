"""StackedMoeExperts: what the stacked, device-routed experts modules share (nn_modules/moe.py: HipMoeExperts on 4-bit GPTQ experts;
nn_modules/moe_fp8.py: HipFp8MoeExperts on FP8 experts).

Both hold ALL experts of a sparse mixture-of-experts block stacked in two buffers per projection and serve the call signature of transformers'
experts modules (Qwen3MoeExperts.forward / MixtralExperts.forward):

    forward(hidden_states [T, H], top_k_index [T, k], top_k_weights [T, k]) -> [T, H]

* fast path (T <= MAX_FAST_TOKENS and the subclass's fast_path predicate): two fused launches into persistent buffers with the routing left on
  the device -- no host synchronisation, safe inside torch.cuda.graph.  An expert id outside [0, E) contributes zero and sets the device `status`
  word, which check_status() reads (never forward()).  Rounding: each projection and the SiLU chain as the per-expert modules round them; the
  top_k expert outputs are combined in ONE fp32 weighted sum in slot order and rounded once (csrc/gptqhip_moe_common.h states both contracts),
  where the HF loop rounds every expert's output and every product and accumulates in the activation dtype.
* grouped path (the subclass's grouped_path predicate: the same shapes at ANY T): gptqhip_moe_align + the subclass's two expert-grouped stages
  + gptqhip_moe_combine -- the slots sorted by expert on the device, every 16-row unit of one expert on the matrix pipe, the same combine
  contract (one fp32 weighted sum in slot order, one rounding), the same status word, no host synchronisation.  Taken when `grouped_routing`
  is set and grouped_min_tokens <= T <= grouped_max_tokens (off by default; GPTQHIP_MOE_GROUPED=1 at construction turns it on), and for
  T > 16 under stream capture, where the host-routed loop cannot run at all.
* slow path (_forward_loop: more tokens, other shapes or dtypes): the host-routed per-expert loop of the HF module over views into the same
  stacked buffers -- arithmetically what a loop over the original modules does.

A subclass supplies the kind of linear it stacks (_is_source / _SOURCE_KIND / _RELEASE_NAMES), the stacking itself (from_linears, on the checks
of _check_lists / _check_module), the fast_path and grouped_path predicates, the two fused op calls (_fused_gate_up / _fused_down), the two
grouped stage calls (_grouped_gate_up / _grouped_down), its eager grouped window (GROUPED_WINDOW) and the slow loop's per-expert gemm
(_expert_gemm).
"""
from __future__ import annotations

import os
from typing import Dict, List, Sequence, Tuple

import torch
import torch.nn as nn

from .. import ops
from ..utils.model import deinterleave_gate_up

MAX_FAST_TOKENS = 16


class StackedMoeExperts(nn.Module):
    _SOURCE_KIND = ""                      # "HIP GPTQ linear": the per-expert module from_linears takes, as messages name it
    _RELEASE_NAMES: Tuple[str, ...] = ()   # its device tensors, dropped once stacked
    # eager window of the grouped path when grouped_routing is set: the first T the few-token ops do not serve, and the grouped ops' slot limit
    # (structural; a subclass states the window its own measurement gives)
    GROUPED_WINDOW: Tuple[int, int] = (MAX_FAST_TOKENS + 1, 65536)

    def __init__(self, num_experts: int, hidden_dim: int, intermediate_dim: int):
        super().__init__()
        self.num_experts = num_experts
        self.hidden_dim = hidden_dim
        self.intermediate_dim = intermediate_dim
        self.training = False
        self._scratch: Dict[Tuple, Tuple[torch.Tensor, ...]] = {}
        self._fast_ok: Dict[Tuple[int, int], bool] = {}
        self.grouped_routing = os.environ.get("GPTQHIP_MOE_GROUPED", "0") == "1"
        self.grouped_min_tokens, self.grouped_max_tokens = self.GROUPED_WINDOW
        self._grouped_ok: Dict[Tuple[int, int], bool] = {}
        self._grouped_eager: Dict[Tuple, Dict] = {}        # (dtype, device) -> one grow-only buffer set, sliced per call
        self._grouped_captured: Dict[Tuple, Dict] = {}     # (T, top_k, dtype, device) -> buffers a graph holds: never freed

    def train(self, mode: bool = True):
        if mode:      # the quantised linears it is built from refuse training mode the same way (SUPPORTS_TRAINING = False)
            raise NotImplementedError(f"{type(self).__name__}: inference only (the HIP quant kernels have no backward)")
        return super().train(False)

    # ---- from_linears: the checks every kind of expert shares ---------------------------------------------------------------------------------
    @staticmethod
    def _is_source(m) -> bool:
        raise NotImplementedError

    @staticmethod
    def _check_lists(gate: Sequence[nn.Module], up: Sequence[nn.Module], down: Sequence[nn.Module]) -> Tuple[List, List, List]:
        gate, up, down = list(gate), list(up), list(down)
        if len(gate) == 0 or len(up) != len(gate) or len(down) != len(gate):
            raise NotImplementedError("from_linears needs three equal-length, non-empty lists")
        return gate, up, down

    @classmethod
    def _check_module(cls, e: int, m, k: int, n: int) -> None:
        """Expert e's projection m is a [k -> n] linear of this class's kind, with nothing the stacked experts do not carry."""
        if not cls._is_source(m):
            raise NotImplementedError(f"expert {e}: {type(m).__name__} is not a {cls._SOURCE_KIND}")
        if getattr(m, "adapter", None) is not None or m.bias is not None:
            raise NotImplementedError(f"expert {e}: adapters / biases are not carried by the stacked experts")
        if (m.in_features, m.out_features) != (k, n):
            raise NotImplementedError(f"expert {e}: shape {(m.in_features, m.out_features)} != {(k, n)}")

    @classmethod
    def _release(cls, m) -> None:
        """Drop a per-expert module's device tensors once they are stacked."""
        for name in cls._RELEASE_NAMES:
            t = getattr(m, name, None)
            if isinstance(t, torch.Tensor):
                t.data = torch.empty(0, dtype=t.dtype, device=t.device)
        m._ready = False

    # ---- forward --------------------------------------------------------------------------------------------------------------------------------
    def fast_path(self, T: int, top_k: int, dtype: torch.dtype) -> bool:
        """Whether forward() serves this call with the two fused launches."""
        raise NotImplementedError

    def _fused_gate_up(self, x: torch.Tensor, ids: torch.Tensor, act: torch.Tensor) -> None:
        raise NotImplementedError

    def _fused_down(self, act: torch.Tensor, ids: torch.Tensor, w: torch.Tensor, out: torch.Tensor) -> None:
        raise NotImplementedError

    def _expert_gemm(self, e: int, projection: str, x: torch.Tensor) -> torch.Tensor:
        """x @ expert e's `gate_up` | `down` projection, through the op the per-expert module would call, on views into the stacked buffers."""
        raise NotImplementedError

    def grouped_path(self, T: int, top_k: int, dtype: torch.dtype) -> bool:
        """Whether the expert-grouped ops can serve this call (the shape predicate; forward() takes them only inside the grouped_routing window
        or under stream capture)."""
        raise NotImplementedError

    def _grouped_gate_up(self, x: torch.Tensor, b: Dict, act: torch.Tensor, top_k: int) -> None:
        """Stage one on the sort buffers b["sorted"] / b["unit_expert"] / b["num_units"]."""
        raise NotImplementedError

    def _grouped_down(self, act: torch.Tensor, b: Dict, part: torch.Tensor, top_k: int) -> None:
        raise NotImplementedError

    def _scratch_for(self, T: int, top_k: int, dtype: torch.dtype, device: torch.device):
        key = (T, top_k, dtype)
        s = self._scratch.get(key)
        if s is None or s[0].device != device:
            s = (torch.empty((T * top_k, self.intermediate_dim), dtype=dtype, device=device),
                 torch.empty((T, self.hidden_dim), dtype=dtype, device=device),
                 torch.empty((T, top_k), dtype=torch.int32, device=device),
                 torch.empty((T, top_k), dtype=torch.float32, device=device))
            self._scratch[key] = s
        return s

    @staticmethod
    def _device_routing(hidden_states: torch.Tensor, top_k_index: torch.Tensor, top_k_weights: torch.Tensor, ids_buf: torch.Tensor,
                        w_buf: torch.Tensor):
        """(x, ids, w) as the fused ops take them: the caller's tensors where they already are contiguous 16-bit / int32 / float32, else a copy
        -- of ids / weights into the head of the persistent ids_buf / w_buf (contiguous, >= T * top_k elements)."""
        if top_k_index.dtype == torch.int32 and top_k_index.is_contiguous():
            ids = top_k_index
        else:
            ids = ids_buf.view(-1)[:top_k_index.numel()].view(top_k_index.shape)
            ids.copy_(top_k_index)
        if top_k_weights.dtype == torch.float32 and top_k_weights.is_contiguous():
            w = top_k_weights
        else:
            w = w_buf.view(-1)[:top_k_weights.numel()].view(top_k_weights.shape)
            w.copy_(top_k_weights)
        return hidden_states if hidden_states.is_contiguous() else hidden_states.contiguous(), ids, w

    def _grouped_alloc(self, S: int, T: int, dtype: torch.dtype, device: torch.device) -> Dict:
        units = ops.moe_grouped_units(S, self.num_experts)
        i32 = dict(dtype=torch.int32, device=device)
        return {"S": S, "T": T,
                "ids": torch.empty(S, **i32), "w": torch.empty(S, dtype=torch.float32, device=device),
                "sorted": torch.empty(16 * units, **i32), "unit_expert": torch.empty(units, **i32), "num_units": torch.empty(1, **i32),
                "act": torch.empty(S * self.intermediate_dim, dtype=dtype, device=device),
                "part": torch.empty(S * self.hidden_dim, dtype=torch.float32, device=device),
                "out": torch.empty(T * self.hidden_dim, dtype=dtype, device=device)}

    def _grouped_scratch(self, T: int, top_k: int, dtype: torch.dtype, device: torch.device, capturing: bool) -> Dict:
        S = T * top_k
        if capturing:       # a graph holds these pointers: one set per signature, never freed or reallocated
            key = (T, top_k, dtype, device)
            b = self._grouped_captured.get(key)
            if b is None:
                b = self._grouped_captured[key] = self._grouped_alloc(S, T, dtype, device)
            return b
        key = (dtype, device)
        b = self._grouped_eager.get(key)
        if b is None or b["S"] < S or b["T"] < T:       # grow only: a prefill's varying T shares one set
            b = self._grouped_eager[key] = self._grouped_alloc(max(S, b["S"] if b else 0), max(T, b["T"] if b else 0), dtype, device)
        return b

    def _forward_grouped(self, hidden_states: torch.Tensor, top_k_index: torch.Tensor, top_k_weights: torch.Tensor, capturing: bool) -> torch.Tensor:
        """The four expert-grouped launches.  The result lives in a persistent buffer of this module that the next grouped call overwrites
        (eager calls share one grow-only buffer set; a captured call owns the set of its (T, top_k, dtype) signature)."""
        T, top_k = top_k_index.shape
        S, H, I, E = T * top_k, self.hidden_dim, self.intermediate_dim, self.num_experts
        b = self._grouped_scratch(T, top_k, hidden_states.dtype, hidden_states.device, capturing)
        x, ids, w = self._device_routing(hidden_states, top_k_index, top_k_weights, b["ids"], b["w"])
        act, part, out = b["act"][:S * I].view(S, I), b["part"][:S * H].view(S, H), b["out"][:T * H].view(T, H)
        ops.moe_align(ids, b["sorted"], b["unit_expert"], b["num_units"], self.status, E)
        self._grouped_gate_up(x, b, act, top_k)
        self._grouped_down(act, b, part, top_k)
        ops.moe_combine(part, ids, w, out, self.status, E)
        return out

    def forward(self, hidden_states: torch.Tensor, top_k_index: torch.Tensor, top_k_weights: torch.Tensor) -> torch.Tensor:
        if hidden_states.dim() != 2 or hidden_states.shape[1] != self.hidden_dim or top_k_index.dim() != 2 \
                or top_k_index.shape != top_k_weights.shape or top_k_index.shape[0] != hidden_states.shape[0]:
            raise RuntimeError(f"{type(self).__name__}: expected hidden_states [T, {self.hidden_dim}] and top_k_index / top_k_weights [T, k], got "
                               f"{tuple(hidden_states.shape)}, {tuple(top_k_index.shape)}, {tuple(top_k_weights.shape)}")
        if not hidden_states.is_cuda:
            raise RuntimeError("gptqmodel_amd HIP ops need tensors on a ROCm device (got a CPU tensor); there is no CPU fallback")
        if top_k_index.shape[0] == 0:
            return torch.zeros_like(hidden_states)
        return self._forward_routed(hidden_states, top_k_index, top_k_weights)

    def _forward_routed(self, hidden_states: torch.Tensor, top_k_index: torch.Tensor, top_k_weights: torch.Tensor) -> torch.Tensor:
        """A validated call with T >= 1: the grouped launches inside the grouped_routing window and for T > 16 under capture, the two fused
        launches where fast_path() holds, else the host-routed loop."""
        T, top_k = top_k_index.shape
        if self.grouped_routing and self.grouped_min_tokens <= T <= self.grouped_max_tokens and self.grouped_path(T, top_k, hidden_states.dtype):
            return self._forward_grouped(hidden_states, top_k_index, top_k_weights, torch.cuda.is_current_stream_capturing())
        if T > MAX_FAST_TOKENS and torch.cuda.is_current_stream_capturing() and self.grouped_path(T, top_k, hidden_states.dtype):
            return self._forward_grouped(hidden_states, top_k_index, top_k_weights, True)      # the host-routed loop cannot be captured
        if T > MAX_FAST_TOKENS or not self.fast_path(T, top_k, hidden_states.dtype):
            return self._forward_loop(hidden_states, top_k_index, top_k_weights)
        # the result lives in a persistent buffer of this module (one per (T, top_k, dtype)): the next call with that signature overwrites it
        act, out, ids_buf, w_buf = self._scratch_for(T, top_k, hidden_states.dtype, hidden_states.device)
        x, ids, w = self._device_routing(hidden_states, top_k_index, top_k_weights, ids_buf, w_buf)
        self._fused_gate_up(x, ids, act)
        self._fused_down(act, ids, w, out)
        return out

    def check_status(self) -> None:
        """Host read of the device status word (a synchronisation: call it outside the decode loop).  Raises IndexError when a device-routed call
        since the last check met an expert id outside [0, num_experts) -- that slot contributed zero -- and clears the word."""
        if int(self.status.item()) != 0:
            self.status.zero_()
            raise IndexError(f"{type(self).__name__}: expert index out of range [0, {self.num_experts}) in a fused MoE call")

    def _forward_loop(self, hidden_states: torch.Tensor, top_k_index: torch.Tensor, top_k_weights: torch.Tensor) -> torch.Tensor:
        """The experts loop of the HF module (host-routed) on _expert_gemm."""
        x = hidden_states
        in_dtype = x.dtype
        if in_dtype not in (torch.float16, torch.bfloat16):
            x = x.to(torch.float16)
        idx = top_k_index.long()
        E = self.num_experts
        if bool(((idx < 0) | (idx >= E)).any()):
            raise IndexError(f"{type(self).__name__}: expert index out of range [0, {E})")
        final = torch.zeros_like(x)
        mask = torch.nn.functional.one_hot(idx, num_classes=E).permute(2, 1, 0)
        for e in torch.greater(mask.sum(dim=(-1, -2)), 0).nonzero().flatten().tolist():
            pos, tok = torch.where(mask[e])
            cur = x[tok].contiguous()
            g, u = deinterleave_gate_up(self._expert_gemm(e, "gate_up", cur))
            h = (torch.nn.functional.silu(g) * u).contiguous()
            d = self._expert_gemm(e, "down", h)
            d = d * top_k_weights[tok, pos, None]
            final.index_add_(0, tok, d.to(final.dtype))
        return final if final.dtype == in_dtype else final.to(in_dtype)


__all__ = ["StackedMoeExperts", "MAX_FAST_TOKENS"]
