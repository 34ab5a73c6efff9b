"""Generates tests/golden/ref_fp8_{row,tensor,block}_{fp16,bf16}.npz from the LIVE reference on the CPU: TorchFP8Linear.pack + forward through
oracle/ref_import.load_reference() (needs the reference checkout; run once, the fixtures are committed).

Each file: weight (the packed float8_e4m3fn bytes as uint8 [N, K]), scale_inv (fp32, the method's layout), w (the float32 weights that were
packed), x, bias, y (float32 holding the activation dtype's values), block (the weight_block_size, zeros when the method has none).
N = 64, K = 256, M = 3, weight_block_size (32, 128)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle.ref_import import load_reference  # noqa: E402

N, K, M, BLOCK = 64, 256, 3, (32, 128)


def main():
    load_reference()
    from gptqmodel.nn_modules.qlinear.fp8 import TorchFP8Linear
    out_dir = os.path.join(ROOT, "tests", "golden")
    for mi, method in enumerate(("row", "tensor", "block")):
        for di, (tag, dt) in enumerate((("fp16", torch.float16), ("bf16", torch.bfloat16))):
            g = torch.Generator().manual_seed(9000 + 10 * mi + di)
            lin = torch.nn.Linear(K, N, bias=True)
            with torch.no_grad():
                lin.weight.copy_(torch.randn(N, K, generator=g) * 0.05)
                lin.weight[5].zero_()                      # an all-zero row: scale_inv falls back to 1
                lin.weight[40:44, 128:].mul_(30.0)         # one loud block
                lin.bias.copy_((torch.randn(N, generator=g) * 0.3).to(dt).float())
            block = BLOCK if method == "block" else None
            mod = TorchFP8Linear(bits=8, group_size=-1, sym=True, desc_act=False, in_features=K, out_features=N, bias=True,
                                 weight_scale_method=method, weight_block_size=block)
            mod.pack(lin, None, None)
            x = (torch.randn(M, K, generator=g) * 0.5).to(dt)
            with torch.no_grad():
                y = mod(x)
            assert y.dtype == dt and mod.weight.dtype == torch.float8_e4m3fn
            np.savez_compressed(os.path.join(out_dir, f"ref_fp8_{method}_{tag}.npz"),
                                weight=mod.weight.view(torch.uint8).numpy(), scale_inv=mod.weight_scale_inv.numpy(),
                                w=lin.weight.detach().numpy(), x=x.float().numpy(), bias=mod.bias.float().numpy(), y=y.float().numpy(),
                                block=np.array(block or (0, 0), np.int32))
            print(method, tag, "scale_inv", tuple(mod.weight_scale_inv.shape), "y", float(y.float().abs().max()))


if __name__ == "__main__":
    main()
