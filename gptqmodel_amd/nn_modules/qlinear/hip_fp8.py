"""HipFp8Linear -- BACKEND.FP8_HIP: FP8 (OCP float8_e4m3fn) weight-only linear, W8A16, on the MI355X kernels of
gptqmodel_amd/csrc/gptqhip_fp8.hip.  The mirror of the reference's TorchFP8Linear (gptqmodel/nn_modules/qlinear/fp8.py:115) on
DEVICE.ROCM: same constructor keywords, buffer names / shapes (`weight` fp8 [out, in], `weight_scale_inv` fp32 () | (out,) |
(out / br, in / bc), `bias`), pack() formula and dequantize_weight() orientation ([in, out]); forward() is ONE HIP kernel that streams the
one-byte weights once instead of dequantising the whole matrix per call (fp8.py:423-425).

Numerics (include/gptqhip.h): y = round(sum_kblocks (1 / scale_inv) * (x . codes) + bias) -- exact products, fp32 sums, the reciprocal scale
on the accumulator, ONE rounding.  Deliberately not the reference's chain (every weight rounded to the activation dtype, then the
matmul's and the bias add's roundings).

Only this package's mirror of the plugin contract carries the class; the upstream-tree overlay (integration/) does not yet."""
from __future__ import annotations

from typing import Optional, Tuple

import torch
import torch.nn as nn

from ...utils.adapter import Lora
from ...utils.backend import BACKEND
from ...utils.const import DEVICE, FORMAT, METHOD, PLATFORM
from . import BaseQuantLinear
from .hip_common import flatten_input, hip_validate_once

# aliases of the reference's FP8 config (quantization/config.py:732-746) -> canonical torch dtype names
_FP8_ALIASES = {
    "e4m3": "float8_e4m3fn", "float8_e4m3": "float8_e4m3fn", "float8_e4m3fn": "float8_e4m3fn",
    "e5m2": "float8_e5m2", "float8_e5m2": "float8_e5m2",
    "e4m3fnuz": "float8_e4m3fnuz", "float8_e4m3fnuz": "float8_e4m3fnuz",
    "e5m2fnuz": "float8_e5m2fnuz", "float8_e5m2fnuz": "float8_e5m2fnuz",
    "e8m0": "float8_e8m0fnu", "e8m0fnu": "float8_e8m0fnu", "float8_e8m0": "float8_e8m0fnu", "float8_e8m0fnu": "float8_e8m0fnu",
}
_SCALE_METHODS = ("tensor", "row", "block")
FP8_MAX = 448.0   # torch.finfo(torch.float8_e4m3fn).max


def normalize_fp8_format(value) -> str:
    """Format alias -> canonical dtype name with the reference's wording for unknown names (config.py:764-781); only float8_e4m3fn has
    kernels here, the other float8 formats are declined by the constructor."""
    if isinstance(value, FORMAT):
        if value != FORMAT.FP8:
            raise ValueError(f"FP8Config: unsupported `format` `{value}`.")
        value = None
    name = "float8_e4m3fn" if value is None else str(value).strip().lower()
    if name in ("", FORMAT.FP8.value):
        name = "float8_e4m3fn"
    resolved = _FP8_ALIASES.get(name)
    if resolved is None:
        raise ValueError(f"FP8Config: unsupported `format` `{value}`. Supported values: {', '.join(sorted(_FP8_ALIASES))}.")
    return resolved


def normalize_block_size(value) -> Optional[Tuple[int, int]]:
    if value is None:
        return None
    if not isinstance(value, (list, tuple)) or len(value) != 2:
        raise ValueError("FP8Config: `weight_block_size` must be a 2-item list/tuple or None.")
    rows, cols = int(value[0]), int(value[1])
    if rows <= 0 or cols <= 0:
        raise ValueError("FP8Config: `weight_block_size` entries must be positive integers.")
    return rows, cols


def normalize_scale_method(value, block_size) -> str:
    name = str("block" if (value is None and block_size is not None) else (value or "row")).strip().lower()
    if name not in _SCALE_METHODS:
        raise ValueError(f"FP8Config: `weight_scale_method` must be one of {{{', '.join(sorted(_SCALE_METHODS))}}}, got `{value}`.")
    if name == "block" and block_size is None:
        raise ValueError("FP8Config: `weight_scale_method='block'` requires `weight_block_size`.")
    if name != "block" and block_size is not None:
        raise ValueError("FP8Config: `weight_block_size` is only valid when `weight_scale_method='block'`.")
    return name


def _amax_to_scale_inv(amax: torch.Tensor) -> torch.Tensor:
    """scale_inv = 448 / amax in fp32 (1 where the slice is all zero): the reference's _compute_scale_inv (fp8.py:45-52)."""
    amax = amax.to(torch.float32)
    safe = amax.clamp_min(torch.finfo(torch.float32).tiny)
    return torch.where(amax > 0, torch.full_like(amax, FP8_MAX) / safe, torch.ones_like(amax))


def quantize_fp8_weight(weight: torch.Tensor, weight_scale_method: str = "row",
                        weight_block_size: Optional[Tuple[int, int]] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """[out, in] float weight -> (float8_e4m3fn codes [out, in], scale_inv fp32) by per-tensor / per-row / per-block amax scaling on the host:
    code = fp8(clamp(w * scale_inv, -448, 448)), the formula of the reference's quantize_fp8_weight (fp8.py:55-112), bit for bit
    (tests/test_fp8_cpu.py against goldens packed by the reference).  Not a hot path: plain torch on the CPU."""
    if weight.ndim != 2:
        raise ValueError(f"FP8 quantization expects a 2D weight matrix, got shape {tuple(weight.shape)}.")
    block = normalize_block_size(weight_block_size)
    method = normalize_scale_method(weight_scale_method, block)
    w = weight.detach().to(device="cpu", dtype=torch.float32).contiguous()
    rows, cols = w.shape
    if method == "tensor":
        scale_inv = _amax_to_scale_inv(w.abs().amax())
        scaled = w * scale_inv
    elif method == "row":
        scale_inv = _amax_to_scale_inv(w.abs().amax(dim=1))
        scaled = w * scale_inv[:, None]
    else:
        br, bc = block
        if rows % br != 0 or cols % bc != 0:
            raise ValueError(f"FP8 block quantization expects shape {tuple(w.shape)} to be divisible by block size {block}.")
        tiles = w.reshape(rows // br, br, cols // bc, bc)
        scale_inv = _amax_to_scale_inv(tiles.abs().amax(dim=(1, 3)))
        scaled = (tiles * scale_inv[:, None, :, None]).reshape(rows, cols)
    codes = scaled.clamp(min=-FP8_MAX, max=FP8_MAX).to(torch.float8_e4m3fn)
    return codes.contiguous(), scale_inv.to(torch.float32).contiguous()


class HipFp8Linear(BaseQuantLinear):
    SUPPORTS_BACKENDS = [BACKEND.FP8_HIP]
    SUPPORTS_METHODS = [METHOD.FP8]
    SUPPORTS_FORMATS = {FORMAT.FP8: 120}   # above the reference's TorchFP8Linear (15, fp8.py:118)
    SUPPORTS_BITS = [8]
    SUPPORTS_GROUP_SIZE = [-1]             # FP8 checkpoints have no GPTQ groups: the scale layout is weight_scale_method / weight_block_size
    SUPPORTS_DESC_ACT = [True, False]      # carried by the plugin signature, meaningless for FP8 (the reference ignores them too)
    SUPPORTS_SYM = [True, False]
    SUPPORTS_SHARDS = True
    SUPPORTS_TRAINING = False
    SUPPORTS_AUTO_PADDING = False
    SUPPORTS_IN_FEATURES_DIVISIBLE_BY = [128]
    SUPPORTS_OUT_FEATURES_DIVISIBLE_BY = [16]
    SUPPORTS_DEVICES = [DEVICE.ROCM]
    SUPPORTS_PLATFORM = [PLATFORM.LINUX]
    SUPPORTS_PACK_DTYPES = [torch.int8, torch.int16, torch.int32, torch.int64]   # unused by FP8 (fp8.py:129)
    SUPPORTS_ADAPTERS = [Lora]
    SUPPORTS_DTYPES = [torch.float16, torch.bfloat16]

    QUANT_TYPE = "hip_fp8"
    _GPTQHIP_KERNEL_CLASS = True

    def __init__(self, bits: int, group_size: int, sym: bool, desc_act: bool, in_features: int, out_features: int,
                 bias: bool = False, pack_dtype: torch.dtype = torch.int32, adapter=None, register_buffers: bool = True,
                 format: str = "float8_e4m3fn", weight_scale_method: str = "row",
                 weight_block_size: Optional[Tuple[int, int]] = None, weight_scale_semantics: str = "inverse", **kwargs):
        self_format = normalize_fp8_format(format)
        if self_format != "float8_e4m3fn":
            raise NotImplementedError(f"HipFp8Linear: float8 format `{self_format}` is not supported by the HIP kernels "
                                      "(float8_e4m3fn only; float8_e5m2, float8_e4m3fnuz and float8_e8m0fnu are declined)")
        semantics = "inverse" if weight_scale_semantics is None else str(weight_scale_semantics).strip().lower()
        if semantics != "inverse":
            raise NotImplementedError(f"Unsupported FP8 scale semantics `{semantics}`.")   # the reference's wording (fp8.py:358-361)
        block = normalize_block_size(weight_block_size)
        method = normalize_scale_method(weight_scale_method, block)
        if method == "block":
            br, bc = block
            if out_features % br != 0 or in_features % bc != 0:
                raise ValueError("TorchFP8Linear block scaling requires out_features/in_features "
                                 f"to be divisible by `weight_block_size={block}`.")   # the reference's wording (fp8.py:164-170)
            if bc % 128 != 0:
                raise NotImplementedError(f"HipFp8Linear: `weight_block_size={block}`: the column block must be a multiple of 128 "
                                          "(one reciprocal scale per 128-row chunk of the kernel layout)")
        super().__init__(bits=bits, group_size=group_size, desc_act=desc_act, sym=sym, in_features=in_features,
                         out_features=out_features, bias=bias, pack_dtype=pack_dtype,
                         backend=kwargs.pop("backend", BACKEND.FP8_HIP), adapter=adapter, **kwargs)
        self.fp8_format = self_format
        self.fp8_dtype = torch.float8_e4m3fn
        self.weight_scale_method = method
        self.weight_block_size = block
        self.weight_scale_semantics = semantics
        self.rscale = None      # 1 / weight_scale_inv (fp32, same shape), formed by post_init on the device
        self._ready = False
        self._bias_cache = None
        if register_buffers:
            self.register_buffer("weight", torch.zeros((out_features, in_features), dtype=self.fp8_dtype))
            self.register_buffer("weight_scale_inv", torch.ones(self._scale_shape(), dtype=torch.float32))
            if bias:
                self.register_buffer("bias", torch.zeros(out_features, dtype=torch.float16))
            else:
                self.bias = None
        else:
            self.bias = None

    # ---- contract ------------------------------------------------------------------------------------
    @classmethod
    def validate_once(cls):
        return hip_validate_once()

    def _scale_shape(self) -> Tuple[int, ...]:
        if self.weight_scale_method == "tensor":
            return ()
        if self.weight_scale_method == "row":
            return (self.out_features,)
        br, bc = self.weight_block_size
        return (self.out_features // br, self.in_features // bc)

    def _scale_mode(self) -> int:
        from gptqmodel_amd import ops
        return ops.FP8_SCALE_MODES[self.weight_scale_method]

    def list_buffers(self):
        return [t for t in (getattr(self, "weight", None), getattr(self, "weight_scale_inv", None), getattr(self, "bias", None))
                if t is not None]

    def runtime_device(self):
        w = getattr(self, "weight", None)
        return w.device if isinstance(w, torch.Tensor) else None

    def extra_repr(self) -> str:
        return (f"in_features={self.in_features}, out_features={self.out_features}, bias={self.bias is not None}, "
                f"format={self.fp8_format}, weight_scale_method={self.weight_scale_method}")

    def _set_buffer(self, name: str, tensor: Optional[torch.Tensor], persistent: bool = True) -> None:
        if name in self._buffers:
            self._buffers[name] = tensor
            return
        if hasattr(self, name):
            delattr(self, name)
        if tensor is None:
            setattr(self, name, None)
        else:
            self.register_buffer(name, tensor, persistent=persistent)

    # ---- packing (host torch; same formula as the reference) -------------------------------------------
    @torch.inference_mode()
    def pack_original(self, linear: nn.Module, scales: torch.Tensor = None, zeros: torch.Tensor = None, g_idx: torch.Tensor = None,
                      **_ignored):
        """Quantise a float nn.Linear into the checkpoint buffers.  scales / zeros / g_idx belong to the plugin signature and are unused,
        as in the reference (fp8.py:283-326)."""
        w = linear.weight.detach()
        if w.dim() > 2:
            w = w.flatten(1)
        codes, scale_inv = quantize_fp8_weight(w, self.weight_scale_method, self.weight_block_size)
        if tuple(codes.shape) != (self.out_features, self.in_features):
            raise ValueError(f"HipFp8Linear.pack: weight shape {tuple(codes.shape)} != {(self.out_features, self.in_features)}")
        self._set_buffer("weight", codes)
        self._set_buffer("weight_scale_inv", scale_inv)
        b = getattr(linear, "bias", None)
        self._set_buffer("bias", None if b is None else b.detach().to(device="cpu", dtype=torch.float16))
        self._set_buffer("rscale", None, persistent=False)
        self._ready = False
        self._bias_cache = None

    def pack(self, linear: nn.Module, scales: torch.Tensor = None, zeros: torch.Tensor = None, g_idx: torch.Tensor = None, **kw):
        self.pack_original(linear, scales, zeros, g_idx)

    def pack_block(self, linear: nn.Module, scales: torch.Tensor = None, zeros: torch.Tensor = None, g_idx: torch.Tensor = None,
                   block_in: int = 8192, workers: int = 1):
        self.pack_original(linear, scales, zeros, g_idx)

    # ---- lifecycle -----------------------------------------------------------------------------------
    def post_init(self):
        """One-time device-side relayout of `weight` into the MFMA-tile-major kernel layout and 1 / weight_scale_inv into `rscale`
        (gptqhip_fp8_repack); the checkpoint-layout copy is released, like HipGptqLinear.post_init does."""
        super().post_init()
        if self._ready:
            return
        from gptqmodel_amd import ops
        if not self.weight.is_cuda:
            raise RuntimeError("HipFp8Linear.post_init: buffers must be on the ROCm device (no CPU fallback)")
        if self.weight.dtype != self.fp8_dtype:
            raise RuntimeError(f"HipFp8Linear.post_init: `weight` is {self.weight.dtype}, expected {self.fp8_dtype}")
        if tuple(self.weight.shape) != (self.out_features, self.in_features):
            raise RuntimeError(f"HipFp8Linear.post_init: `weight` shape {tuple(self.weight.shape)} != "
                               f"{(self.out_features, self.in_features)}")
        if tuple(self.weight_scale_inv.shape) != self._scale_shape():
            raise RuntimeError(f"HipFp8Linear.post_init: `weight_scale_inv` shape {tuple(self.weight_scale_inv.shape)} != "
                               f"{self._scale_shape()} ({self.weight_scale_method} scales)")
        if not ops.fp8_supported(1, self.in_features, self.out_features, self._scale_mode(), self.weight_block_size, torch.float16,
                                 self.fp8_format):
            raise NotImplementedError(f"HipFp8Linear: unsupported layer {self.in_features} x {self.out_features} with "
                                      f"{self.weight_scale_method} scales {self.weight_block_size}")
        w_t, rscale = ops.fp8_repack(self.weight.data, self.weight_scale_inv.data, self._scale_mode(), self.weight_block_size)
        self.weight.data = w_t   # kernel layout (uint8 [out * in]); the checkpoint-layout copy is released
        self._set_buffer("rscale", rscale.reshape(self.weight_scale_inv.shape), persistent=False)
        self._ready = True

    def _save_to_state_dict(self, destination, prefix, keep_vars):
        if self._ready:
            raise RuntimeError(f"{self.__class__.__name__} `{self.name}`: state_dict() after post_init() would save "
                               "the kernel (tile-major) layout; save from the original checkpoint instead")
        super()._save_to_state_dict(destination, prefix, keep_vars)

    def _bias_for(self, dtype: torch.dtype, device: torch.device):
        if self.bias is None:
            return None
        c = self._bias_cache
        if c is None or c.dtype != dtype or c.device != device:
            c = self.bias.to(device=device, dtype=dtype).contiguous()   # fp8.py:452-455 casts the bias to the output dtype
            self._bias_cache = c
        return c

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if not self._ready:
            raise RuntimeError("HipFp8Linear.forward called before post_init()")
        from gptqmodel_amd import ops
        out_shape = x.shape[:-1] + (self.out_features,)
        x2, in_dtype = flatten_input(self._apply_rotation_to_input(x), self.in_features)
        out = ops.fp8_gemm(x2, self.weight, self.rscale.reshape(-1), self._bias_for(x2.dtype, x2.device), self.out_features,
                           self._scale_mode(), self.weight_block_size)   # an empty batch returns an empty tensor
        if self.adapter:
            out = self.adapter.apply(x=x2, out=out)   # fp8.py:458-459
        if out.dtype != in_dtype:
            out = out.to(in_dtype)
        return out.reshape(out_shape)

    def dequantize_weight(self, *, device=None, dtype: Optional[torch.dtype] = None) -> torch.Tensor:
        """[in, out] weights (the orientation of TorchFP8Linear.dequantize_weight, fp8.py:350-387) in `dtype` (default float32), each
        element rounded once from the fp32 product code * (1 / scale_inv), by the device kernel."""
        if self.weight_scale_semantics != "inverse":
            raise NotImplementedError(f"Unsupported FP8 scale semantics `{self.weight_scale_semantics}`.")
        from gptqmodel_amd import ops
        dtype = torch.float32 if dtype is None else dtype
        if self._ready:
            w_t, rscale = self.weight, self.rscale
        else:
            if not self.weight.is_cuda:
                raise RuntimeError("HipFp8Linear.dequantize_weight: buffers must be on the ROCm device (no CPU fallback)")
            w_t, rscale = ops.fp8_repack(self.weight.data, self.weight_scale_inv.data, self._scale_mode(), self.weight_block_size)
        out = ops.fp8_dequant(w_t, rscale.reshape(-1), self.in_features, self.out_features, self._scale_mode(), self.weight_block_size,
                              out_dtype=dtype)
        return out if device is None else out.to(device)


__all__ = ["HipFp8Linear", "quantize_fp8_weight"]
