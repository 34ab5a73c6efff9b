"""GPU tests of the batch-1 decode path over the DYNAMIC RANGE of its activations.

The default decode form (5) feeds the raw 4-bit codes to the f16 matrix pipe and takes the zero-points out through the chunk's activation sum;
bf16 activations are first converted to fp16 per wave, divided by a power of two chosen from the wave's own largest |x| (bf16_wave_scale in
gptqmodel_amd/csrc/gptqhip_skinny.hip, used by skinny1_kernel and by the persistent-tile skinny1p_kernel).  Every other decode test draws
randn * {3e-4 .. 3e3}, with all waves of a row at one magnitude.  Here: uniform scales from 1e-12 to 1e6 (bf16) and down to rows made only
of fp16 subnormals (fp16), and structured rows -- one tiny non-zero chunk, a per-chunk ramp (neighbouring waves choose different exponents),
one outlier among tiny values, all zeros, all -0.0 -- through gptqhip_gemm at M = 1 and the decode op at M = 1, 2, 4, 16, under the default form
and the bit-faithful form 4, on a one-tile-per-CU layer, a long-K layer and a two-tiles-per-CU layer (the persistent-tile kernel: the second
conversion site), plus an act-order layer (the gather path of the x pieces) and the fused RMSNorm with a tiny / huge hidden state.

Every case is held against float64 arithmetic on the integer codes, y_exact = x64 @ (scales64[g] * (codes - zeros[g])), or -- for the calls
that keep the reference's per-weight rounding -- against the float64 product with the reference's rounded weights; the bars are the relative
ones of test_gpu_tp8_shapes.py::_assert_partial_f32 (fp32 partial sums, 1e-4) and of test_gpu_decode_forms.py (rounded output of the exact
form no further from y_exact than the reference chain, or one rounding of the output dtype), which hold at every input scale.  The fp32
partial sums carry the check: rounded fp16 outputs are judged only where the largest exact output lies in [2^-10, 6e4] (below, the outputs
are fp16 subnormals and one output ulp is a visible fraction of the vector; above, the reference's and the kernel's fp16 outputs are inf).

Out of scope: non-finite activations.  Form 5 computes s (sum x q - z sum x) and can give NaN where the reference gives +-inf."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from helpers import RANGE_FAMILIES, dynamic_range_rows, f32_to_torch, rel_err, synth_gptq, torch_to_f32
from oracle import gptq_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GS = 128
# (GPTQHIP_DECODE_BITFAITHFUL=1 in the environment: every batch-1 call keeps the reference's per-weight rounding -- no exact form to expect)
EXACT_DEFAULT = os.environ.get("GPTQHIP_DECODE_BITFAITHFUL", "0") in ("", "0")
OUT_ROUNDING = {"fp16": 2.0 ** -11, "bf16": 2.0 ** -8}          # one rounding of the output dtype (the bars of test_gpu_decode_forms.py)
LAYERS = {"4096x4096": (4096, 4096, False), "14336x4096": (14336, 4096, False), "4096x8192": (4096, 8192, False),
          "4096x8192-actorder": (4096, 8192, True)}
ENTRIES = [("gemm", 1), ("decode", 1), ("decode", 2), ("decode", 4), ("decode", 16)]
CASES = [(act, fam) for act in ("bf16", "fp16") for fam in RANGE_FAMILIES[act]]
PARAMS = [pytest.param(name, entry, M, id=f"{name}-{entry}-M{M}") for name, (_, _, desc) in LAYERS.items() for entry, M in ENTRIES
          if not desc or M == 1]                                 # (the in-kernel permutation is exercised on the batch-1 kernels under test)


@pytest.fixture(scope="module")
def ops():
    from gptqmodel_amd import ops as _ops
    yield _ops
    _ops.set_decode_form(-1)


@pytest.fixture(scope="module")
def layers(ops):
    """name -> the layer: repacked once, s (q - z) in float64 once, the reference's rounded weights and the 16 rows of every input family
    with their float64 products once (a case at M rows uses the first M)."""
    cache = {}

    def get(name):
        if name not in cache:
            K, N, desc = LAYERS[name]
            qweight, qzeros, scales, g_idx = synth_gptq(1200 + K // 128 + N // 16 + int(desc), 4, K, N, GS, desc_act=desc)
            g = O.normalize_g_idx(g_idx, scales.shape[0])
            w_exact = np.asarray(scales, np.float64)[g] * (O.unpack_rows(qweight, 4).astype(np.int64) - O.unpack_cols(qzeros, 4).astype(np.int64)[g])
            sc = f32_to_torch(scales, "fp16", DEV)
            perm = torch.from_numpy(np.argsort(g_idx, kind="stable").astype(np.int32)).to(DEV) if desc else None
            qw_t, meta = ops.repack_tiled(torch.from_numpy(qweight).to(DEV), torch.from_numpy(qzeros).to(DEV), sc, perm, GS, 4)
            cache[name] = SimpleNamespace(K=K, N=N, w_exact=w_exact, w_deq=O.dequant_gptq(qweight, qzeros, scales, g_idx, 4, "fp16"),
                                          w_rounded={}, qw_t=qw_t, meta=meta, sdt=sc.dtype, perm=perm, rows={})
        return cache[name]

    return get


def _references(L, x, act):
    """-> (x64 @ s (q - z), x64 @ the reference's rounded weights, the oracle's rounded output).  The last is O.forward_gptq with the layer's
    dequantised weights kept between cases: dequant_gptq, the cast to the activation dtype, matmul_round."""
    if act not in L.w_rounded:
        L.w_rounded[act] = O.round_to(L.w_deq, act)
    x64 = x.astype(np.float64)
    return x64 @ L.w_exact, x64 @ L.w_rounded[act].astype(np.float64), O.matmul_round(x, L.w_rounded[act], None, act).astype(np.float64)


def _family(L, act, family):
    if (act, family) not in L.rows:
        x = dynamic_range_rows(act, family, 16, L.K, seed=L.K // 128 + L.N // 16)
        L.rows[(act, family)] = (x,) + _references(L, x, act)
    return L.rows[(act, family)]


def _row_rel_err(got, ref):
    """rel_err of every row on its own (rows of one call must not hide behind the largest)."""
    return max(rel_err(got[m:m + 1], ref[m:m + 1]) for m in range(got.shape[0]))


def _expects_exact(act, M, form):
    """Which calls take an exact-arithmetic form (as in test_tp8_row_shards_partial_f32_through_the_decode_op): the process default on fp16 rows
    up to 4 and on a single bf16 row; form 4, more rows and GPTQHIP_DECODE_BITFAITHFUL=1 keep the reference's per-weight rounding."""
    return EXACT_DEFAULT and form == -1 and ((act == "fp16" and M <= 4) or (act == "bf16" and M == 1))


def _check(tag, act, exact, part, out, x, y_exact, y_rw, y_oracle):
    """part: fp32 partial sums, out: rounded output (float32 views) of one call pair."""
    assert np.isfinite(part).all(), tag
    e_exact, e_rw = _row_rel_err(part, y_exact), _row_rel_err(part, y_rw)
    print(f"{tag}: partial f32 rel err {e_exact:.3e} vs the exact product, {e_rw:.3e} vs the rounded weights")
    if exact:
        assert e_exact <= 1e-4, (tag, f"partial f32 rel err {e_exact:.3e} vs the exact product")
    else:
        assert e_rw <= 1e-4, (tag, f"partial f32 rel err {e_rw:.3e} vs the reference's rounded weights")
    if not x.any():                                            # all zeros / all -0.0
        assert not part.any() and not out.any(), (tag, "a zero row must give exactly 0")
    if not exact:
        return
    for m in range(out.shape[0]):
        scale = np.abs(y_exact[m]).max()
        if scale == 0.0 or (act == "fp16" and not 2.0 ** -10 <= scale <= 6.0e4):
            continue
        assert np.isfinite(out[m]).all(), tag
        err, err_ref = np.abs(out[m] - y_exact[m]).max() / scale, np.abs(y_oracle[m] - y_exact[m]).max() / scale
        print(f"{tag} row {m}: rounded output {err:.3e} from the exact product (reference chain: {err_ref:.3e})")
        assert err <= max(err_ref * 1.05, OUT_ROUNDING[act]) + 1e-7, (tag, m, err, err_ref)


@pytest.mark.parametrize("form", [-1, 4])
@pytest.mark.parametrize("name,entry,M", PARAMS)
@pytest.mark.parametrize("act,family", CASES)
def test_decode_over_the_activation_range(ops, layers, act, family, name, entry, M, form):
    L = layers(name)
    x, y_exact, y_rw, y_oracle = (a[:M] for a in _family(L, act, family))
    xd = f32_to_torch(x, act, DEV)
    ops.set_decode_form(form)
    try:
        if entry == "gemm":
            part = ops.gemm(xd, L.qw_t, L.meta, None, L.perm, L.N, GS, 4, L.sdt, partial_f32=True)
            out = ops.gemm(xd, L.qw_t, L.meta, None, L.perm, L.N, GS, 4, L.sdt)
        else:
            xin = xd if M > 1 else xd[0]
            part = ops.decode_linear(xin, L.qw_t, L.meta, None, L.K, L.N, GS, 4, L.sdt, out_glue=ops.OUT_PARTIAL_F32, perm=L.perm, M=M)
            out = ops.decode_linear(xin, L.qw_t, L.meta, None, L.K, L.N, GS, 4, L.sdt, perm=L.perm, M=M)
        torch.cuda.synchronize()
    finally:
        ops.set_decode_form(-1)
    assert part.dtype == torch.float32
    _check((act, family, name, entry, M, form), act, _expects_exact(act, M, form), torch_to_f32(part).reshape(M, L.N).astype(np.float64),
           torch_to_f32(out).reshape(M, L.N).astype(np.float64), x, y_exact, y_rw, y_oracle)


@pytest.mark.parametrize("form", [-1, 4])
@pytest.mark.parametrize("entry", ["gemm", "decode"])
@pytest.mark.parametrize("act,family", [(a, f) for a in ("bf16", "fp16") for f in ("zero", "negzero")])
def test_zero_row_gives_exactly_the_bias(ops, layers, act, family, entry, form):
    L = layers("4096x4096")
    x = dynamic_range_rows(act, family, 1, L.K)
    bias = O.round_to(np.random.RandomState(3).randn(L.N).astype(np.float32) * 0.1, act)
    xd, bd = f32_to_torch(x, act, DEV), f32_to_torch(bias, act, DEV)
    ops.set_decode_form(form)
    try:
        if entry == "gemm":
            out = ops.gemm(xd, L.qw_t, L.meta, bd, None, L.N, GS, 4, L.sdt)[0]
        else:
            out = ops.decode_linear(xd[0], L.qw_t, L.meta, bd, L.K, L.N, GS, 4, L.sdt)
        torch.cuda.synchronize()
    finally:
        ops.set_decode_form(-1)
    assert np.array_equal(torch_to_f32(out), bias)


@pytest.mark.parametrize("form", [-1, 4])
@pytest.mark.parametrize("with_stats", [True, False])
@pytest.mark.parametrize("name", ["4096x4096", "4096x8192"])
@pytest.mark.parametrize("hscale", [1e-6, 1e6])
def test_rmsnorm_glue_over_the_hidden_state_range(ops, layers, hscale, name, with_stats, form):
    """bf16 hidden states far below / above 1 through the fused RMSNorm (eps = 1e-5): with eps dominating mean(h^2) a tiny h stays tiny after
    the norm (1e-6 -> about 3e-4), a huge one comes out at the norm weight's scale; producer statistics or the in-kernel sum of squares."""
    act, eps = "bf16", 1e-5
    L = layers(name)
    rng = np.random.RandomState(57)
    h = O.round_to(rng.randn(L.K).astype(np.float32) * np.float32(hscale), act)
    w = O.round_to(1.0 + rng.randn(L.K).astype(np.float32) * 0.1, act)
    xn = O.rmsnorm_ref(h, w, eps, act)[None]
    st_in = torch.from_numpy((h.astype(np.float64) ** 2).reshape(-1, 16).sum(axis=1).astype(np.float32)).to(DEV) if with_stats else None
    kw = dict(in_glue=ops.GLUE_RMSNORM, norm_weight=f32_to_torch(w, act, DEV), eps=eps, stats_in=st_in)
    hd = f32_to_torch(h, act, DEV)
    ops.set_decode_form(form)
    try:
        part = ops.decode_linear(hd, L.qw_t, L.meta, None, L.K, L.N, GS, 4, L.sdt, out_glue=ops.OUT_PARTIAL_F32, **kw)
        out = ops.decode_linear(hd, L.qw_t, L.meta, None, L.K, L.N, GS, 4, L.sdt, **kw)
        torch.cuda.synchronize()
    finally:
        ops.set_decode_form(-1)
    _check(("rmsnorm", hscale, name, with_stats, form), act, _expects_exact(act, 1, form), torch_to_f32(part)[None].astype(np.float64),
           torch_to_f32(out)[None].astype(np.float64), xn, *_references(L, xn, act))
