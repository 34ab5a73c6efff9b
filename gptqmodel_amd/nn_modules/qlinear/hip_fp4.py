"""HipFp4Linear -- BACKEND.FP4_HIP: NVFP4 (e2m1 codes, one float8_e4m3fn scale per 16 input features, one fp32 global scale) weight-only linear,
W4A16, on the MI355X kernels of gptqmodel_amd/csrc/gptqhip_fp4.hip.  Serves the checkpoints the reference rebuilds as TorchFP4Linear
(gptqmodel/nn_modules/qlinear/fp4.py:19, models/base.py:2099-2142, 2275-2317), whose forward needs torchao's NVFP4Tensor and hardware that
advertises native NVFP4; same buffer names and shapes on DEVICE.ROCM:

    weight          uint8 [out, in / 2] (a torch.float4_e2m1fn_x2 tensor is taken as its uint8 view); feature 2 b is the LOW nibble of byte b
    weight_scale    float8_e4m3fn [out, in / 16], plain row-major (torchao's swizzled layout is declined)
    weight_scale_2  fp32 scalar (), default 1.0: ModelOpt's global scale (base.py:2113-2115)
    bias            optional

W[n, k] = code[n, k] * weight_scale[n, k / 16] * weight_scale_2.  forward() is ONE HIP kernel:
y = round(weight_scale_2 * sum_k x[k] * (code * weight_scale) + bias) -- exact block-scaled weights on the matrix pipe, fp32 sums, the global
scale and the bias on the fp32 accumulator, ONE rounding (include/gptqhip.h).  Deliberately not the reference's dequantise-then-matmul chain
(quantization/dtype.py:303-340).

Only this package's mirror of the plugin contract carries the class; the upstream-tree overlay (integration/) does not."""
from __future__ import annotations

from typing import Optional, Tuple

import torch
import torch.nn as nn

from ...utils.adapter import Lora
from ...utils.backend import BACKEND
from ...utils.const import DEVICE, FORMAT, METHOD, PLATFORM
from . import BaseQuantLinear
from .hip_common import flatten_input, hip_validate_once

FP4_BLOCK = 16
FP4_MAX = 6.0     # the largest e2m1 magnitude
E4M3_MAX = 448.0  # torch.finfo(torch.float8_e4m3fn).max
_FP4_X2 = getattr(torch, "float4_e2m1fn_x2", None)
# e2m1 magnitudes by the low three code bits `e1 e0 m` (gptqmodel_ext/floatx_cpu.cpp:153-156); bit 3 is the sign
E2M1_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)


def normalize_fp4_block_size(value) -> int:
    """`weight_block_size` of TorchFP4Linear (fp4.py:29): an int (a 1- or 2-item list / tuple names the input-feature block last)."""
    if value is None:
        return FP4_BLOCK
    if isinstance(value, (list, tuple)):
        if len(value) not in (1, 2) or (len(value) == 2 and int(value[0]) != 1):
            raise ValueError(f"NVFP4: `weight_block_size` must be an int or (1, block), got `{value}`.")
        value = value[-1]
    return int(value)


def _nearest_e2m1(v: torch.Tensor) -> torch.Tensor:
    """fp32 values -> e2m1 codes (uint8 0 .. 15): the nearest magnitude, ties to the even code, clamped to +-6."""
    a = v.abs()
    idx = ((a > 0.25).to(torch.uint8) + (a >= 0.75).to(torch.uint8) + (a > 1.25).to(torch.uint8) + (a >= 1.75).to(torch.uint8)
           + (a > 2.5).to(torch.uint8) + (a >= 3.5).to(torch.uint8) + (a > 5.0).to(torch.uint8))
    return idx | (torch.signbit(v).to(torch.uint8) << 3)


def quantize_nvfp4_weight(weight: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """[out, in] float weight -> (packed uint8 [out, in / 2], weight_scale float8_e4m3fn [out, in / 16], weight_scale_2 fp32 ()), on the host
    in fp32:
        weight_scale_2 = amax(W) / (6 * 448)                                   (1 for an all-zero matrix)
        weight_scale   = e4m3(clamp(block_amax / 6 / weight_scale_2, 0, 448))  (round to nearest even)
        code           = nearest e2m1 of W / (fp32(weight_scale) * weight_scale_2), ties to even, clamped to +-6
    A block whose scale comes out 0 (all-zero, or too small for e4m3) gets codes 0.  This is the two-level NVFP4 recipe stated as a formula;
    torchao is not a dependency, so no bit-parity with its nvfp4_quantize is claimed.  Not a hot path: plain torch on the CPU."""
    if weight.ndim != 2:
        raise ValueError(f"NVFP4 quantization expects a 2D weight matrix, got shape {tuple(weight.shape)}.")
    w = weight.detach().to(device="cpu", dtype=torch.float32).contiguous()
    rows, cols = w.shape
    if cols % FP4_BLOCK != 0:
        raise ValueError(f"NVFP4 quantization expects in_features {cols} to be divisible by the block size {FP4_BLOCK}.")
    amax = w.abs().amax() if w.numel() else w.new_zeros(())
    scale_2 = torch.where(amax > 0, amax / (FP4_MAX * E4M3_MAX), torch.ones_like(amax)).to(torch.float32)
    blocks = w.reshape(rows, cols // FP4_BLOCK, FP4_BLOCK)
    scale = (blocks.abs().amax(dim=2) / FP4_MAX / scale_2).clamp(min=0.0, max=E4M3_MAX).to(torch.float8_e4m3fn)
    den = scale.to(torch.float32) * scale_2
    ratio = torch.where(den[:, :, None] > 0, blocks / den.clamp_min(torch.finfo(torch.float32).tiny)[:, :, None], torch.zeros_like(blocks))
    codes = _nearest_e2m1(ratio).reshape(rows, cols)
    codes = torch.where((den > 0).repeat_interleave(FP4_BLOCK, dim=1), codes, torch.zeros_like(codes))
    packed = codes[:, 0::2] | (codes[:, 1::2] << 4)   # the low nibble is the even feature (floatx_cpu.cpp:1998-2003)
    return packed.contiguous(), scale.contiguous(), scale_2.reshape(())


class HipFp4Linear(BaseQuantLinear):
    SUPPORTS_BACKENDS = [BACKEND.FP4_HIP]
    SUPPORTS_METHODS = [METHOD.NVFP4]
    SUPPORTS_FORMATS = {FORMAT.NVFP4: 120}
    SUPPORTS_BITS = [4]
    SUPPORTS_GROUP_SIZE = [FP4_BLOCK]      # the NVFP4 block: one e4m3 scale per 16 input features
    SUPPORTS_DESC_ACT = [True, False]      # carried by the plugin signature, meaningless for NVFP4
    SUPPORTS_SYM = [True, False]
    SUPPORTS_SHARDS = True
    SUPPORTS_TRAINING = False
    SUPPORTS_AUTO_PADDING = False
    SUPPORTS_IN_FEATURES_DIVISIBLE_BY = [128]
    SUPPORTS_OUT_FEATURES_DIVISIBLE_BY = [16]
    SUPPORTS_DEVICES = [DEVICE.ROCM]
    SUPPORTS_PLATFORM = [PLATFORM.LINUX]
    SUPPORTS_PACK_DTYPES = [torch.int8, torch.int16, torch.int32, torch.int64]   # unused by NVFP4
    SUPPORTS_ADAPTERS = [Lora]
    SUPPORTS_DTYPES = [torch.float16, torch.bfloat16]

    QUANT_TYPE = "hip_fp4"
    _GPTQHIP_KERNEL_CLASS = True

    def __init__(self, bits: int, group_size: int, sym: bool, desc_act: bool, in_features: int, out_features: int,
                 bias: bool = False, pack_dtype: torch.dtype = torch.int32, adapter=None, register_buffers: bool = True,
                 weight_block_size=None, **kwargs):
        block = normalize_fp4_block_size(weight_block_size)
        if block != FP4_BLOCK:
            raise NotImplementedError(f"HipFp4Linear: `weight_block_size={block}` is not supported by the HIP kernels (NVFP4's 16 only; "
                                      "MXFP4's 32 with e8m0 scales is declined)")
        if group_size != FP4_BLOCK:
            raise NotImplementedError(f"HipFp4Linear: `group_size={group_size}` is not supported (the NVFP4 block of {FP4_BLOCK} only)")
        super().__init__(bits=bits, group_size=group_size, desc_act=desc_act, sym=sym, in_features=in_features,
                         out_features=out_features, bias=bias, pack_dtype=pack_dtype,
                         backend=kwargs.pop("backend", BACKEND.FP4_HIP), adapter=adapter, **kwargs)
        self.weight_block_size = block
        self._ready = False
        self._bias_cache = None
        if register_buffers:
            self.register_buffer("weight", torch.zeros((out_features, in_features // 2), dtype=torch.uint8))
            self.register_buffer("weight_scale", torch.zeros((out_features, in_features // block), dtype=torch.float8_e4m3fn))
            self.register_buffer("weight_scale_2", torch.ones((), dtype=torch.float32))
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

    def list_buffers(self):
        return [t for t in (getattr(self, n, None) for n in ("weight", "weight_scale", "weight_scale_2", "bias")) if t is not None]

    def runtime_device(self):
        w = getattr(self, "weight", None)
        return w.device if isinstance(w, torch.Tensor) else None

    def extra_repr(self) -> str:
        return (f"in_features={self.in_features}, out_features={self.out_features}, bias={self.bias is not None}, "
                f"format=nvfp4, weight_block_size={self.weight_block_size}")

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

    # ---- packing (host torch) --------------------------------------------------------------------------
    @torch.inference_mode()
    def pack_original(self, linear: nn.Module, scales: torch.Tensor = None, zeros: torch.Tensor = None, g_idx: torch.Tensor = None,
                      **_ignored):
        """Quantise a float nn.Linear into the checkpoint buffers (quantize_nvfp4_weight).  scales / zeros / g_idx belong to the plugin
        signature and are unused."""
        w = linear.weight.detach()
        if w.dim() > 2:
            w = w.flatten(1)
        if tuple(w.shape) != (self.out_features, self.in_features):
            raise ValueError(f"HipFp4Linear.pack: weight shape {tuple(w.shape)} != {(self.out_features, self.in_features)}")
        packed, scale, scale_2 = quantize_nvfp4_weight(w)
        self._set_buffer("weight", packed)
        self._set_buffer("weight_scale", scale)
        self._set_buffer("weight_scale_2", scale_2)
        b = getattr(linear, "bias", None)
        self._set_buffer("bias", None if b is None else b.detach().to(device="cpu", dtype=torch.float16))
        self._ready = False
        self._bias_cache = None

    def pack(self, linear: nn.Module, scales: torch.Tensor = None, zeros: torch.Tensor = None, g_idx: torch.Tensor = None, **kw):
        self.pack_original(linear, scales, zeros, g_idx)

    def pack_block(self, linear: nn.Module, scales: torch.Tensor = None, zeros: torch.Tensor = None, g_idx: torch.Tensor = None,
                   block_in: int = 8192, workers: int = 1):
        self.pack_original(linear, scales, zeros, g_idx)

    # ---- lifecycle -----------------------------------------------------------------------------------
    def _check_buffers(self, what: str) -> None:
        """The checkpoint contract, declined with a message where it is not met; nothing falls back to torch."""
        w, s, s2 = self.weight, self.weight_scale, self.weight_scale_2
        if w.dtype != torch.uint8 and (_FP4_X2 is None or w.dtype != _FP4_X2):
            raise NotImplementedError(f"HipFp4Linear.{what}: `weight` is {w.dtype}, expected uint8 (or float4_e2m1fn_x2): two e2m1 codes per byte")
        if tuple(w.shape) != (self.out_features, self.in_features // 2):
            raise NotImplementedError(f"HipFp4Linear.{what}: `weight` shape {tuple(w.shape)} != {(self.out_features, self.in_features // 2)}")
        if s.dtype != torch.float8_e4m3fn:
            raise NotImplementedError(f"HipFp4Linear.{what}: `weight_scale` is {s.dtype}, expected float8_e4m3fn (an fp32 or e8m0 block scale "
                                      "is not NVFP4 and is not supported)")
        if tuple(s.shape) != (self.out_features, self.in_features // self.weight_block_size):
            raise NotImplementedError(f"HipFp4Linear.{what}: `weight_scale` shape {tuple(s.shape)} != "
                                      f"{(self.out_features, self.in_features // self.weight_block_size)}: only the plain row-major layout is "
                                      "supported (a swizzled / padded scale layout is declined)")
        if s2.numel() != 1:
            raise NotImplementedError(f"HipFp4Linear.{what}: `weight_scale_2` has {s2.numel()} elements, expected one global scale")
        if not (w.is_cuda and s.is_cuda and s2.is_cuda and (self.bias is None or self.bias.is_cuda)):
            raise RuntimeError(f"HipFp4Linear.{what}: buffers must be on the ROCm device (no CPU fallback)")

    def post_init(self):
        """One-time device-side relayout of `weight` / `weight_scale` into the MFMA-tile-major kernel layout (gptqhip_fp4_repack); the
        checkpoint-layout copies are released and `weight_scale_2` stays on the device as one fp32 element."""
        super().post_init()
        if self._ready:
            return
        from gptqmodel_amd import ops
        self._check_buffers("post_init")
        if not ops.fp4_supported(1, self.in_features, self.out_features, self.weight_block_size, torch.float16):
            raise NotImplementedError(f"HipFp4Linear: unsupported layer {self.in_features} x {self.out_features} "
                                      f"(block size {self.weight_block_size})")
        w_t, s_t = ops.fp4_repack(self.weight.data, self.weight_scale.data, self.weight_block_size)
        self._set_buffer("weight", w_t)          # kernel layout (uint8 [out * in / 2]); the checkpoint-layout copy is released
        self._set_buffer("weight_scale", s_t)    # kernel layout (uint8 [out * in / 16])
        self._set_buffer("weight_scale_2", self.weight_scale_2.data.to(torch.float32).reshape(1).contiguous())
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
            c = self.bias.to(device=device, dtype=dtype).contiguous()   # fp4.py:60-62 casts the bias to the input dtype
            self._bias_cache = c
        return c

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if not self._ready:
            raise RuntimeError("HipFp4Linear.forward called before post_init()")
        from gptqmodel_amd import ops
        out_shape = x.shape[:-1] + (self.out_features,)
        x2, in_dtype = flatten_input(self._apply_rotation_to_input(x), self.in_features)
        out = ops.fp4_gemm(x2, self.weight, self.weight_scale, self.weight_scale_2, self._bias_for(x2.dtype, x2.device), self.out_features,
                           self.weight_block_size)   # an empty batch returns an empty tensor
        if self.adapter:
            out = self.adapter.apply(x=x2, out=out)
        if out.dtype != in_dtype:
            out = out.to(in_dtype)
        return out.reshape(out_shape)

    def dequantize_weight(self, *, device=None, dtype: Optional[torch.dtype] = None) -> torch.Tensor:
        """[in, out] weights in `dtype` (default float32), each element round(fp32(code * weight_scale) * weight_scale_2), once, by the
        device kernel."""
        from gptqmodel_amd import ops
        dtype = torch.float32 if dtype is None else dtype
        if self._ready:
            w_t, s_t, s2 = self.weight, self.weight_scale, self.weight_scale_2
        else:
            self._check_buffers("dequantize_weight")
            w_t, s_t = ops.fp4_repack(self.weight.data, self.weight_scale.data, self.weight_block_size)
            s2 = self.weight_scale_2.data.to(torch.float32).reshape(1).contiguous()
        out = ops.fp4_dequant(w_t, s_t, s2, self.in_features, self.out_features, self.weight_block_size, out_dtype=dtype)
        return out if device is None else out.to(device)


__all__ = ["HipFp4Linear", "quantize_nvfp4_weight"]
