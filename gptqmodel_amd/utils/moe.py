"""Sparse mixture-of-experts blocks onto the fused MoE decode ops (nn_modules/moe.py: HipMoeExperts; nn_modules/moe_fp8.py: HipFp8MoeExperts).

`fuse_moe_experts(block)` recognises a sparse-MoE block whose `experts` is a container of per-expert MLP modules -- `gate_proj` / `up_proj` /
`down_proj`, or Mixtral's `w1` / `w3` / `w2` -- all of them adapter-free 4-bit HIP GPTQ linears of equal shapes, group size and dtype without
act-order, and replaces `block.experts` by one HipMoeExperts.  A block whose projections are ALL HipFp8Linear (float8_e4m3fn, one scale layout
for gate / up and one for down) gets one HipFp8MoeExperts the same way; a mix of FP8 and other projections is declined, and so is a block
with NVFP4 projections (HipFp4Linear: no stacked form yet).  The stand-in serves
the call the block's forward makes under the installed transformers release, `self.experts(hidden_states, top_k_index, top_k_weights)`; a bare
nn.ModuleList has no such call (the block's own forward indexes it) and is left alone.  Anything not recognised is left untouched with the
reason recorded on the block (`block._gptqhip_moe_skipped`); the helper never raises.  `auto_fuse_moe(model)` applies it to every such block
(the tail of utils.hf_llama.auto_fuse, so both post-init routes get it; GPTQHIP_AUTO_FUSE=0 opts out)."""
from __future__ import annotations

import os
from typing import List, Optional, Tuple

import torch.nn as nn

_NAMINGS = (("gate_proj", "up_proj", "down_proj"), ("w1", "w3", "w2"))      # (gate, up, down)


def _expert_modules(block) -> Optional[List[nn.Module]]:
    experts = getattr(block, "experts", None)
    if not isinstance(experts, nn.Module):
        return None
    children = list(experts.children()) if not isinstance(experts, (nn.ModuleList, nn.ModuleDict)) else (
        list(experts) if isinstance(experts, nn.ModuleList) else list(experts.values()))
    return children or None


def _naming(expert) -> Optional[Tuple[str, str, str]]:
    for names in _NAMINGS:
        if all(isinstance(getattr(expert, n, None), nn.Module) for n in names):
            return names
    return None


def _decline(block, why: str) -> bool:
    try:
        block._gptqhip_moe_skipped = why
    except Exception:  # noqa: BLE001
        pass
    return False


def _is_moe_block(m) -> bool:
    mods = _expert_modules(m)
    return bool(mods) and all(_naming(e) is not None for e in mods)


def fuse_moe_experts(block: nn.Module, grouped_routing: Optional[bool] = None) -> bool:
    """Replace `block.experts` (a container of per-expert HIP GPTQ MLPs) by one HipMoeExperts, or (of per-expert HIP FP8 MLPs) by one
    HipFp8MoeExperts.  True when replaced; False -- with the reason in `block._gptqhip_moe_skipped` and the block untouched -- otherwise.
    Never raises.  grouped_routing: the stand-in's `grouped_routing` attribute (the expert-grouped device-routed path beyond 16 tokens, int4
    and FP8 alike); None keeps its default (GPTQHIP_MOE_GROUPED=1 in the environment)."""
    try:
        from ..nn_modules.moe import HipMoeExperts
        from ..nn_modules.moe_base import StackedMoeExperts
        from ..nn_modules.moe_fp8 import HipFp8MoeExperts
        mods = _expert_modules(block)
        if not mods:
            return _decline(block, "no container of per-expert modules under `experts`")
        experts = block.experts
        if isinstance(experts, StackedMoeExperts):
            return _decline(block, "already fused")
        if type(experts).forward is nn.Module.forward:
            return _decline(block, f"{type(experts).__name__} is indexed by the block's own forward: there is no "
                                   "experts(hidden_states, top_k_index, top_k_weights) call to stand in for")
        names = _naming(mods[0])
        if names is None or any(_naming(e) != names for e in mods):
            return _decline(block, "experts do not all carry gate_proj/up_proj/down_proj (or w1/w3/w2) projections")
        for e in mods:
            act = getattr(e, "act_fn", None)
            if act is not None and not (isinstance(act, nn.SiLU) or type(act).__name__ in ("SiLU", "SiLUActivation")):
                return _decline(block, "expert activation is not SiLU")
        gate, up, down = ([getattr(e, n) for e in mods] for n in names)
        kinds = {getattr(m, "QUANT_TYPE", "") for m in gate + up + down}
        if "hip_fp4" in kinds:
            return _decline(block, "NVFP4 experts (HipFp4Linear) have no stacked fused form: each projection keeps its own launch")
        if "hip_fp8" in kinds and len(kinds) > 1:
            return _decline(block, f"experts mix FP8 and other projections ({', '.join(sorted(str(k) or 'unquantised' for k in kinds))})")
        fused_cls = HipFp8MoeExperts if kinds == {"hip_fp8"} else HipMoeExperts
        try:
            fused = fused_cls.from_linears(gate, up, down)
        except NotImplementedError as e:
            return _decline(block, f"experts cannot share the stacked layout: {e}")
        if grouped_routing is not None:
            fused.grouped_routing = bool(grouped_routing)
        block.experts = fused
        if hasattr(block, "_gptqhip_moe_skipped"):
            del block._gptqhip_moe_skipped
        return True
    except Exception as e:  # noqa: BLE001  (a convenience pass must never break a load)
        return _decline(block, f"{type(e).__name__}: {e}")


def auto_fuse_moe(model: nn.Module, grouped_routing: Optional[bool] = None) -> int:
    """fuse_moe_experts (with `grouped_routing` passed on) on every sparse-MoE block of `model`; returns the number of fused blocks and records
    `model._gptqhip_moe_fused` / `model._gptqhip_moe_skipped` [(block class, reason)].  Models without such blocks see no change.
    Opt-out like auto_fuse: GPTQHIP_AUTO_FUSE=0 in the environment, or `model._gptqhip_auto_fuse = False`."""
    if os.environ.get("GPTQHIP_AUTO_FUSE", "1") == "0" or not isinstance(model, nn.Module) or getattr(model, "_gptqhip_auto_fuse", True) is False:
        return 0
    try:
        blocks = [m for m in model.modules() if _is_moe_block(m)]
        if not blocks:
            return 0
        fused, skipped = 0, []
        for b in blocks:
            if fuse_moe_experts(b, grouped_routing):
                fused += 1
            else:
                skipped.append((type(b).__name__, getattr(b, "_gptqhip_moe_skipped", "")))
        model._gptqhip_moe_fused = fused
        model._gptqhip_moe_skipped = skipped
        return fused
    except Exception as e:  # noqa: BLE001
        import warnings
        warnings.warn(f"gptqmodel_amd: MoE expert fusion skipped ({type(e).__name__}: {e}); the plugin forward() path serves the experts")
        return 0


__all__ = ["fuse_moe_experts", "auto_fuse_moe"]
