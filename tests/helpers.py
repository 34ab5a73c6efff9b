"""Shared helpers for the parity tests: golden-fixture decoding and oracle <-> torch conversions."""
import numpy as np
import torch

from oracle import gptq_oracle as O

TDT = {"fp16": torch.float16, "bf16": torch.bfloat16}


def bits_to_torch(bits: np.ndarray, dtype: str, device="cpu") -> torch.Tensor:
    t = torch.from_numpy(np.ascontiguousarray(bits).view(np.int16).copy()).view(TDT[dtype])
    return t.to(device)


def torch_to_bits(t: torch.Tensor) -> np.ndarray:
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def bits_to_f32(bits: np.ndarray, dtype: str) -> np.ndarray:
    if dtype == "fp16":
        return bits.view(np.float16).astype(np.float32)
    return O.bf16_from_bits(bits)


def torch_to_f32(t: torch.Tensor) -> np.ndarray:
    return t.detach().float().cpu().numpy()


def rel_err(a: np.ndarray, b: np.ndarray) -> float:
    """max |a-b| / max |b|  -- the 'relative error of the output vector' gate (SURVEY.md §7 hard part i)."""
    return float(np.abs(a - b).max() / max(float(np.abs(b).max()), 1e-12))


# element-wise tolerances of the reference's own forward test (tests/test_torch_kernel_accuracy.py:111-125):
#   torch.allclose(out, ref, atol=5e-3 if fp16 else 3e-2, rtol=1e-2)
REF_ATOL = {"fp16": 5e-3, "bf16": 3e-2}
REF_RTOL = 1e-2
# norm-wise bar: north_star's <= 1e-3 relative fp16 error; bf16: 8e-3 = one bf16 ulp (2^-7) of the largest output, what a kernel that repeats the
# reference's rounding chain meets.  (The reference's own kernel table, tests/kernels/test_gptq.py:229-266, 353-360, uses 0.008 differently: as the
# atol of an ELEMENT-WISE torch.isclose(ref, out, rtol=0.15, atol=0.008) -- REF_KERNEL_* below; its torch-kernel accuracy test compares against an
# exact-arithmetic fp32 product with allclose(atol=3e-2, rtol=1e-2), tests/test_torch_kernel_accuracy.py:111-125 -- REF_ATOL / REF_RTOL.)
NORM_TOL = {"fp16": 1e-3, "bf16": 8e-3}
# exact-arithmetic decode form on bf16 activations (decode form 5): the output is the correctly rounded exact sum, the reference's is the rounded sum of
# per-weight-rounded products -- they differ by the reference's own rounding noise, i.e. up to one bf16 ulp per rounding step (two with a bias / residual)
NORM_TOL_BF16_EXACT = 2.0 ** -6
REF_KERNEL_RTOL, REF_KERNEL_ATOL = 0.15, {"fp16": 0.004, "bf16": 0.008}     # test_gptq.py: isclose(rtol=0.15, atol=<per backend: Marlin / ExllamaV2 values>)


def decode_norm_tol(act: str, bits: int = 4):
    """Norm-wise bar of a batch-1 call (gptqhip_gemm at M = 1, gptqhip_decode_linear at M = 1) under the process-default decode form: 4-bit codes
    take the exact-arithmetic form 5 (fp16: 1e-3 as everywhere; bf16 activations: one bf16 ulp per rounding step, NORM_TOL_BF16_EXACT);
    GPTQHIP_DECODE_BITFAITHFUL=1 and 8-bit codes keep the reference's rounding chain and the plain bars."""
    import os
    if act == "bf16" and bits == 4 and os.environ.get("GPTQHIP_DECODE_BITFAITHFUL", "0") in ("", "0"):
        return NORM_TOL_BF16_EXACT
    return NORM_TOL[act]


def assert_forward_close(got: np.ndarray, ref: np.ndarray, act: str, tag=None, strict_atol: bool = False, norm_tol: float = None):
    """Both gates on a rounded forward output: (1) the norm-wise relative error of the output (north_star), and
    (2) the reference's own ELEMENT-WISE assertion with its atol/rtol.

    The reference states its atol (5e-3 fp16 / 3e-2 bf16) on ITS test data -- x = randn * 0.5, K = 64, outputs of magnitude <~ 1, compared
    with an exact-arithmetic fp32 product (tests/test_torch_kernel_accuracy.py:111-125).  On a vector whose largest output is S the same
    gate is atol * max(1, S / 5): an absolute 5e-3 on outputs of several hundred (the stress-scale cases of test_gpu_decode_chain.py) is
    2e-5 of the output scale, which only a kernel that repeats the reference's per-weight rounding bit for bit can meet on the elements
    that cancel to ~0 -- it measures the reference's OWN rounding noise, not the kernel's error.  strict_atol=True keeps the unscaled atol:
    used for the bit-faithful decode forms (gptqhip_set_decode_form 0 / 4) and everywhere the outputs stay at the reference's scale."""
    got = np.asarray(got, dtype=np.float32)
    ref = np.asarray(ref, dtype=np.float32)
    assert got.shape == ref.shape, (got.shape, ref.shape, tag)
    e = rel_err(got, ref)
    nt = NORM_TOL[act] if norm_tol is None else norm_tol
    assert e <= nt, (f"norm-wise rel err {e:.3e} > {nt}", tag)
    # the reference's kernel-table gate (element-wise isclose with rtol 0.15), at the output's scale like the gate below
    katol = REF_KERNEL_ATOL[act] * max(1.0, float(np.abs(ref).max()) / 5.0)
    assert not (np.abs(got - ref) > katol + REF_KERNEL_RTOL * np.abs(ref)).any(), ("outside the reference's kernel-table isclose gate", tag)
    atol = REF_ATOL[act] * (1.0 if strict_atol else max(1.0, float(np.abs(ref).max()) / 5.0))
    bad = np.abs(got - ref) > atol + REF_RTOL * np.abs(ref)
    assert not bad.any(), (f"{int(bad.sum())} of {bad.size} elements outside atol={atol:.3g} rtol={REF_RTOL}; "
                           f"worst |d|={float(np.abs(got - ref).max()):.3e}", tag)


def synth_gptq(seed, bits, k, n, gs, desc_act=False, sym=False, scale_dtype="fp16"):
    """Seeded synthetic GPTQ-v2 tensors following BASELINE.md §2 / SURVEY.md §8d."""
    rng = np.random.RandomState(seed)
    g = k // gs
    # (any word pattern is a valid encoding at every bit width / layout: every bit belongs to some code)
    qweight = rng.randint(-2**31, 2**31, size=(k * bits // 32, n), dtype=np.int64).astype(np.int32)
    if sym:
        qzeros = O.pack_cols_any(np.full((g, n), 1 << (bits - 1), dtype=np.uint8), bits)
    else:
        qzeros = rng.randint(-2**31, 2**31, size=(g, n * bits // 32), dtype=np.int64).astype(np.int32)
    scales = O.round_to(rng.rand(g, n).astype(np.float32) * 0.01 + 0.005, scale_dtype)
    g_idx = ((rng.permutation(k) if desc_act else np.arange(k)) // gs).astype(np.int32)
    return qweight, qzeros, scales, g_idx


# ----------------------------------------------------------------------------------------------------------
# FULL-SIZE reference fixtures (tests/golden/full_*.npz, written by oracle/make_golden.py:make_fullsize): the packed
# tensors of a BASELINE-sized layer are far too big to commit, so a fixture stores the SEED + the reference's outputs
# (+ a few dequantised rows + a checksum of the regenerated inputs); both the generator and the tests rebuild the
# inputs with this one function (numpy legacy RandomState: the stream is frozen across numpy versions).
# ----------------------------------------------------------------------------------------------------------
def synth_full_case(kind, seed, bits, k, n, gs, desc_act, sym, scale_dtype, act, m):
    """-> dict(qweight, qzeros, scales (f32, exactly representable in scale_dtype), g_idx | None, x (f32, in act)).
    kind "gptq": checkpoint-layout v2 tensors; kind "awq": AWQ GEMM-layout tensors (no g_idx, asymmetric zeros)."""
    rng = np.random.RandomState(seed)
    g = k // gs
    if kind == "gptq":
        qweight, qzeros, scales, g_idx = synth_gptq(seed, bits, k, n, gs, desc_act=desc_act, sym=sym,
                                                    scale_dtype=scale_dtype)
        rng = np.random.RandomState(seed + 7919)
    else:
        qweight = rng.randint(-2**31, 2**31, size=(k, n // 8), dtype=np.int64).astype(np.int32)
        qzeros = rng.randint(-2**31, 2**31, size=(g, n // 8), dtype=np.int64).astype(np.int32)
        scales = O.round_to(rng.rand(g, n).astype(np.float32) * 0.01 + 0.005, scale_dtype)
        g_idx = None
    x = O.round_to(rng.randn(m, k).astype(np.float32) * 0.5, act)
    return {"qweight": qweight, "qzeros": qzeros, "scales": scales, "g_idx": g_idx, "x": x}


def inputs_checksum(case) -> np.ndarray:
    """Cheap order-sensitive checksum of the regenerated inputs (uint64[4]): detects any RNG / rounding drift."""
    out = []
    for key in ("qweight", "qzeros", "scales", "x"):
        a = np.ascontiguousarray(case[key])
        u = a.view(np.uint32).astype(np.uint64).reshape(-1)
        w = (np.arange(u.size, dtype=np.uint64) % np.uint64(65521)) + np.uint64(1)
        out.append(np.uint64((u * w).sum()))
    return np.array(out, dtype=np.uint64)


def f32_to_torch(a: np.ndarray, dtype: str, device="cpu") -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(TDT[dtype]).to(device)


# ----------------------------------------------------------------------------------------------------------
# numpy model of the MFMA-tile-major kernel layout (gptqmodel_amd/csrc/gptqhip_device.h) -- the checker for the
# device repack kernel (integer work: compared bit-exactly)
# ----------------------------------------------------------------------------------------------------------
def np_repack_tiled(qweight, qzeros, scales_bits, perm, group_size, bits):
    pf = 32 // bits
    codes = O.unpack_rows(qweight, bits).astype(np.uint32)          # [K, N]
    zeros = O.unpack_cols(qzeros, bits).astype(np.uint32)           # [G, N]
    K, N = codes.shape
    G = K // group_size
    if perm is not None:
        codes = codes[np.asarray(perm).astype(np.int64)]
    chunks, tiles = -(-K // 128), -(-N // 16)
    Kp, Np = chunks * 128, tiles * 16
    full = np.zeros((Kp, Np), dtype=np.uint32)
    full[:K, :N] = codes
    if Kp > K:
        full[K:, :N] = zeros[G - 1][None, :]                          # padded rows dequantise to exactly 0
    steps = 4
    if bits == 4:
        # word[tile, chunk, lane=(rq,c), j]: rows 128*chunk + 32*j + 8*rq + e, e at bit 4*(e>>1) + 16*(e&1)
        v = full.reshape(chunks, steps, 4, 8, tiles, 16)              # [chunk, j, rq, e, tile, c]
        sh = np.array([4 * (e >> 1) + 16 * (e & 1) for e in range(8)], dtype=np.uint32)
        words = np.bitwise_or.reduce(v << sh[None, None, None, :, None, None], axis=3)   # [chunk, j, rq, tile, c]
        words = words.transpose(3, 0, 2, 4, 1)                         # [tile, chunk, rq, c, j]
        qw_t = np.ascontiguousarray(words).reshape(-1)
    else:
        # word[tile, chunk, h, lane, jj]: j = 2h + (jj>>1), half = jj&1, rows ... + 4*half + e, e at 8*(e>>1)+16*(e&1)
        v = full.reshape(chunks, 2, 2, 4, 2, 4, tiles, 16)            # [chunk, h, jlo, rq, half, e, tile, c]
        sh = np.array([8 * (e >> 1) + 16 * (e & 1) for e in range(4)], dtype=np.uint32)
        words = np.bitwise_or.reduce(v << sh[None, None, None, None, None, :, None, None], axis=5)
        words = words.transpose(5, 0, 1, 3, 6, 2, 4)                   # [tile, chunk, h, rq, c, jlo, half]
        qw_t = np.ascontiguousarray(words).reshape(-1)
    meta = np.zeros((tiles, G, 16), dtype=np.uint32)
    sb = np.zeros((G, Np), dtype=np.uint32)
    sb[:, :N] = scales_bits.astype(np.uint32)
    zz = np.zeros((G, Np), dtype=np.uint32)
    zz[:, :N] = zeros
    m = sb | ((np.uint32(0xE400) | zz) << np.uint32(16))
    meta = m.reshape(G, tiles, 16).transpose(1, 0, 2)
    return qw_t.view(np.int32), np.ascontiguousarray(meta).reshape(-1).view(np.int32)


def shared_gpu_wait_ms(world: int, default_ms: int = 10000) -> int:
    """Peer-wait bound for the multi-process tests whose ranks all run on ONE GPU.  With 4 / 8 processes (+ the pytest process)
    the GPU scheduler time-slices them -- a collective step costs a rotation of its quanta (measured: ~4.5 ms per all-reduce at
    world 8 vs 56 us at world 2) and an occasional rotation takes seconds -- so the product's 10 s bound, sized for one process
    per GPU, can expire although nothing is lost.  Those tests wait longer instead of failing on the scheduler."""
    return default_ms if world < 4 else max(default_ms, 120000)


# ----------------------------------------------------------------------------------------------------------
# Activation dynamic range of the batch-1 decode path (tests/test_gpu_decode_dynamic_range.py on the GPU,
# tests/test_bf16_wave_scale_model.py on the CPU): the input families, and a numpy statement of the bf16 -> fp16 conversion of
# decode form 5 (gptqmodel_amd/csrc/gptqhip_skinny.hip: wave_max_abs_bf16 / bf16_wave_scale / bf16pair_to_f16pair)
# ----------------------------------------------------------------------------------------------------------
RANGE_UNIFORM = {"bf16": (1e-12, 1e-9, 1e-6, 1e-4, 0.5, 3e3, 1e6), "fp16": (1e-5, 3e-4, 0.5, 3e3)}
RANGE_STRUCTURED = ("chunk_only", "ramp", "outlier", "zero", "negzero")
RANGE_FAMILIES = {"bf16": tuple(f"u{s:g}" for s in RANGE_UNIFORM["bf16"]) + RANGE_STRUCTURED,
                  "fp16": tuple(f"u{s:g}" for s in RANGE_UNIFORM["fp16"]) + ("subnormal",) + RANGE_STRUCTURED}


def dynamic_range_rows(act: str, family: str, m: int, k: int, seed: int = 0) -> np.ndarray:
    """[m, k] float32 activations, exactly representable in `act`, of one input family (k a multiple of 128):
      u<s>        randn * s (fp16: clipped to +-65504)
      subnormal   fp16 only: n * 2^-24 with integer n uniform in [-1023, 1023] -- every element an fp16 subnormal (or 0)
      chunk_only  non-zero in ONE 128-row chunk only, tiny there (bf16: randn * 1e-7, fp16: subnormals), exact zeros elsewhere
      ramp        chunk c scaled by 2^-c, floored at 2^-40 (bf16) / 2^-24 (fp16): neighbouring waves see different magnitudes
      outlier     one large element (bf16 2e5, fp16 6e4), everything else tiny (bf16 randn * 1e-6, fp16 subnormals)
      zero        +0.0 everywhere;  negzero: -0.0 everywhere"""
    assert k % 128 == 0 and family in RANGE_FAMILIES[act], (act, family, k)
    rng = np.random.RandomState(9000 + seed)
    sub = lambda: rng.randint(-1023, 1024, size=(m, k)).astype(np.float32) * np.float32(2.0 ** -24)   # noqa: E731
    tiny = (lambda: rng.randn(m, k).astype(np.float32) * np.float32(1e-6)) if act == "bf16" else sub
    if family.startswith("u"):
        x = rng.randn(m, k).astype(np.float32) * np.float32(float(family[1:]))
        if act == "fp16":
            x = np.clip(x, -65504.0, 65504.0)
    elif family == "subnormal":
        x = sub()
    elif family == "chunk_only":
        x = np.zeros((m, k), np.float32)
        c = 5 % (k // 128)
        x[:, 128 * c:128 * (c + 1)] = (rng.randn(m, k).astype(np.float32) * np.float32(1e-7) if act == "bf16" else sub())[:, :128]
    elif family == "ramp":
        floor = -40 if act == "bf16" else -24
        e = np.maximum(-(np.arange(k) // 128), floor).astype(np.float64)
        x = (rng.randn(m, k) * 0.5 * 2.0 ** e[None, :]).astype(np.float32)
    elif family == "outlier":
        x = tiny()
        x[:, 7] = 2.0e5 if act == "bf16" else 6.0e4
    else:
        x = np.full((m, k), 0.0 if family == "zero" else -0.0, np.float32)
    return O.round_to(x, act)


def np_bf16_wave_to_f16(x_bf16_as_f32: np.ndarray, groups, down_only: bool = False):
    """What a wave of decode form 5 is meant to do with its bf16 x pieces, in numpy.  `x_bf16_as_f32`: [K] float32 holding bf16 values;
    `groups`: the number of consecutive elements that share one wave (an int dividing K) or an int array [K] of group ids.
    Per group: take the maximum of |x|, choose the integer k that puts it in [2^14, 2^15) -- clamped to |k| <= 126, k = 0 when the maximum is
    zero or a bf16 subnormal --, multiply by 2^-k, convert to fp16 with round-toward-zero.  -> (fp16 values [K], 2^k per element [K] float64);
    x is recovered as f16.astype(float64) * up.  down_only=True models the scheme this one replaces (k = max(k, 0): never scaled up)."""
    x = np.asarray(x_bf16_as_f32, np.float32).reshape(-1)
    gid = np.arange(x.size) // int(groups) if np.isscalar(groups) else np.asarray(groups).reshape(-1)
    k = np.zeros(x.size, np.int64)
    for g in np.unique(gid):
        sel = gid == g
        ef = int((np.abs(x[sel]).max().view(np.uint32) >> 23) & 0xFF)          # biased exponent of the group's largest |x|
        kg = 0 if ef == 0 else max(ef - (127 + 14), -126)
        k[sel] = max(kg, 0) if down_only else kg
    y = x.astype(np.float64) * 2.0 ** (-k).astype(np.float64)                   # exact: a power of two, far inside float64's range
    _, e = np.frexp(y)                                                          # |y| = m 2^e with m in [0.5, 1)
    quantum = 2.0 ** np.maximum(e - 11, -24).astype(np.float64)                 # fp16: 11 significant bits, subnormal spacing 2^-24
    h = np.trunc(y / quantum) * quantum                                         # round toward zero
    assert np.abs(h).max(initial=0.0) < 65536.0
    return h.astype(np.float16), 2.0 ** k.astype(np.float64)


# ----------------------------------------------------------------------------------------------------------
# Weight-side dynamic range (tests/test_weight_range_families_cpu.py on the CPU, tests/test_gpu_weight_dynamic_range.py on the GPU):
# scales from fp16 subnormals to the largest the reference's fp16 weights stay finite with, exponents that differ between neighbouring
# groups / columns, negative and zero scales; codes that cluster around the zero-point (what a trained checkpoint holds), sit on it, or
# sit at the ends of the code range.  synth_gptq above draws scales in [0.005, 0.015] and uniform codes only.
# ----------------------------------------------------------------------------------------------------------
WEIGHT_SCALE_STRUCTURED = ("group_ramp", "column_ramp", "outlier_group", "signed", "zero_groups")
WEIGHT_CODE_FAMILIES = ("random", "near_zero_point", "at_zero_point", "extremes", "sym")
WEIGHT_RANGE_FAMILIES = {"scale": ("sub", "u<m>") + WEIGHT_SCALE_STRUCTURED, "code": WEIGHT_CODE_FAMILIES}


def weight_scale_top(bits: int) -> float:
    """The largest ladder step m: (2^bits - 1) * 2 m -- the largest |s (q - z)| of a u<m> layer -- is still finite in fp16."""
    return {4: 2048.0, 8: 64.0}[bits]


def weight_scale_ladder(act: str, scale_dtype: str, bits: int):
    """The steps m of the u<m> families: from the smallest normal of the scale dtype's useful range to the top.  fp16 scales start at
    2^-14; bf16 scales at 2^-60 with bf16 activations and at 2^-24 with fp16 activations (below, every weight the reference casts to
    fp16 is 0 or one fp16 quantum and no fp16 row can bring the output into fp16's normal range).  With fp16 activations -- and with fp16
    scales -- the top is weight_scale_top (the reference's own rounded weights stay finite); bf16 x bf16 goes on to 2^60."""
    top = weight_scale_top(bits)
    if scale_dtype == "fp16":
        return (2.0 ** -14, 1e-3, 0.01, 1.0, top)
    if act == "fp16":
        return (2.0 ** -24, 2.0 ** -14, 1e-3, 0.01, 1.0, top)
    return (2.0 ** -60, 2.0 ** -14, 1e-3, 0.01, 1.0, top, 2.0 ** 60)


def _ladder_name(m: float) -> str:
    e = int(np.round(np.log2(m)))
    return f"u2^{e}" if (2.0 ** e == m and abs(e) > 12) else f"u{m:g}"


def _ladder_value(name: str) -> float:
    return 2.0 ** int(name[3:]) if name.startswith("u2^") else float(name[1:])


def weight_scale_families(act: str, scale_dtype: str, bits: int):
    """Names of every scale family of one (activation dtype, scale dtype, bit width): 'sub' (fp16 scales only), the u<m> ladder
    ('u2^-14', 'u0.001', ..), and the structured ones."""
    return (("sub",) if scale_dtype == "fp16" else ()) + tuple(_ladder_name(m) for m in weight_scale_ladder(act, scale_dtype, bits)) \
        + WEIGHT_SCALE_STRUCTURED


def weight_range_layer(scale_family, code_family, bits, K, N, gs, scale_dtype, desc_act=False, seed=0):
    """-> (qweight, qzeros, scales, g_idx), the contract of synth_gptq (numpy legacy RandomState; scales float32, exactly representable
    in scale_dtype).  Scale families, [G, N], each rounded to scale_dtype:
      sub            fp16 only: n * 2^-24, n uniform in 1..1023 -- every scale an fp16 subnormal
      u<m>           m * (1 + rand)                                    (u2^-14, u0.001, u1, u2048, ..: weight_scale_ladder)
      group_ramp     u0.01 with group g multiplied by 2^((7 g) mod 21 - 10) = 2^-10, 2^-3, 2^4, 2^-10, ..: neighbouring groups of a column 2^7 / 2^14 apart
      column_ramp    u0.01 with column n multiplied by 2^((n mod 16) - 8): the 16 lanes of a column tile carry different exponents
      outlier_group  u2^-20 except ONE group per column at weight_scale_top(bits) * (1 + rand)
      signed         u0.01 with a random sign per (group, column)
      zero_groups    u0.01 with about a quarter of the (group, column) scales exactly +0.0 or -0.0
    Code families (zero-points z [G, N], codes [K, N]):
      random           uniform codes and zero-points
      near_zero_point  z uniform, every code in {z - 1, z, z + 1} clipped to the code range
      at_zero_point    z uniform, every code equal to its z: every weight is exactly 0.  (With zero_groups the groups whose scale IS zero
                       keep uniform codes -- 0 * anything -- so the layer still dequantises to zeros only.)
      extremes         z in {0, max}, codes in {0, max}
      sym              z = 2^(bits - 1), uniform codes"""
    assert code_family in WEIGHT_CODE_FAMILIES and K % gs == 0, (code_family, K, gs)
    rng = np.random.RandomState(7000 + seed)
    G, maxq = K // gs, (1 << bits) - 1
    g_idx = ((rng.permutation(K) if desc_act else np.arange(K)) // gs).astype(np.int32)
    u = lambda m: m * (1.0 + rng.rand(G, N))   # noqa: E731
    if scale_family == "sub":
        assert scale_dtype == "fp16"
        s = rng.randint(1, 1024, size=(G, N)).astype(np.float64) * 2.0 ** -24
    elif scale_family.startswith("u"):
        s = u(_ladder_value(scale_family))
    elif scale_family == "group_ramp":
        s = u(0.01) * 2.0 ** (((7 * np.arange(G)) % 21) - 10.0)[:, None]
    elif scale_family == "column_ramp":
        s = u(0.01) * 2.0 ** ((np.arange(N) % 16) - 8.0)[None, :]
    elif scale_family == "outlier_group":
        s = u(2.0 ** -20)
        s[rng.randint(0, G, size=N), np.arange(N)] = weight_scale_top(bits) * (1.0 + rng.rand(N))
    elif scale_family == "signed":
        s = u(0.01) * rng.choice([-1.0, 1.0], size=(G, N))
    elif scale_family == "zero_groups":
        s = u(0.01)
        s = np.where(rng.rand(G, N) < 0.25, np.where(rng.rand(G, N) < 0.5, 0.0, -0.0), s)
    else:
        raise ValueError(scale_family)
    scales = O.round_to(s.astype(np.float32), scale_dtype)
    if code_family == "sym":
        z = np.full((G, N), 1 << (bits - 1), np.int64)
    elif code_family == "extremes":
        z = rng.randint(0, 2, size=(G, N)) * maxq
    else:
        z = rng.randint(0, maxq + 1, size=(G, N))
    zk = z[g_idx]
    if code_family in ("random", "sym"):
        codes = rng.randint(0, maxq + 1, size=(K, N))
    elif code_family == "near_zero_point":
        codes = np.clip(zk + rng.randint(-1, 2, size=(K, N)), 0, maxq)
    elif code_family == "at_zero_point":
        codes = np.where(scales[g_idx] == 0.0, rng.randint(0, maxq + 1, size=(K, N)), zk)
    else:
        codes = rng.randint(0, 2, size=(K, N)) * maxq
    return O.pack_rows(codes.astype(np.uint8), bits), O.pack_cols(z.astype(np.uint8), bits), scales, g_idx


def weight_exact_f64(qweight, qzeros, scales, g_idx, bits):
    """s (q - z) in float64 on the integer codes: [K, N]."""
    g = O.normalize_g_idx(g_idx, scales.shape[0])
    return np.asarray(scales, np.float64)[g] * (O.unpack_rows(qweight, bits).astype(np.int64) - O.unpack_cols(qzeros, bits).astype(np.int64)[g])


def weight_range_rows(act: str, w_exact: np.ndarray, m: int, seed: int = 0) -> np.ndarray:
    """[m, K] float32 activations, exactly representable in `act`: randn rows times a power of two per row, chosen from the float64
    product so that the row's largest |x @ w_exact| lands in [1, 64] (aimed at 8), and clipped so that the row stays inside the
    activation dtype's normal range (fp16: 2^-10 .. 2^12, i.e. |x| < 65504 and a typical element normal; bf16: 2^+-100).  All waves of a
    row see one magnitude.  An all-zero product (at_zero_point) keeps the plain randn row."""
    rng = np.random.RandomState(9100 + seed)
    x0 = O.round_to(rng.randn(m, w_exact.shape[0]).astype(np.float32), act)
    y0 = np.abs(x0.astype(np.float64) @ w_exact).max(axis=1)
    e = np.where(y0 > 0.0, np.rint(np.log2(8.0 / np.where(y0 > 0.0, y0, 1.0))), 0.0)
    lo, hi = (-10.0, 12.0) if act == "fp16" else (-100.0, 100.0)
    return O.round_to((x0.astype(np.float64) * 2.0 ** np.clip(e, lo, hi)[:, None]).astype(np.float32), act)


# The cases of tests/test_gpu_weight_dynamic_range.py, shared with the CPU test that vouches for them (finite reference weights and
# outputs, every row's largest |y_exact| in [2^-10, 6e4]).  Shapes: the smallest at which each code path exists.
WEIGHT_RANGE_DTYPES = (("fp16", "fp16"), ("bf16", "bf16"), ("fp16", "bf16"))             # (activations, scales)
WEIGHT_RANGE_MAIN = "512x256g128"
WEIGHT_RANGE_DECODE_SHAPES = {                                                            # name -> (bits, K, N, gs, act-order)
    "512x256g128": (4, 512, 256, 128, False),
    "512x256g32": (4, 512, 256, 32, False),            # four group constants per chunk
    "1408x256g64": (4, 1408, 256, 64, False),          # padded last ring round
    "512x8192g128": (4, 512, 8192, 128, False),        # two column tiles per CU: the wide forms at 2..16 rows
    "2048x8192g128": (4, 2048, 8192, 128, False),      # ... with 16 chunks of K: the persistent-tile kernel at one row, the 4-deep ring at 2..4
    "512x256g128-actorder": (4, 512, 256, 128, True),  # act-order through gptqhip_gemm (x gathered in front of the kernel; the decode op declines it)
    "2048x1024g128-actorder": (4, 2048, 1024, 128, True),  # ... and the smallest layer the in-kernel permutation serves (the 4-deep ring)
}
WEIGHT_RANGE_TILED = {                                   # name -> (bits, K, N, gs, M, set_tuning arguments)
    "tiled-384x264g128": (4, 384, 264, 128, 70, (0, 2, 0)),
    "tiled-256x136g64": (4, 256, 136, 64, 33, (0, 2, 0)),
    "tiled8-256x128g64": (8, 256, 128, 64, 77, (0, 2, 0)),
    "tiled-n128-384x264g128": (4, 384, 264, 128, 65, (1, 2, 1000 + 64)),
    "tiled-splitk-384x264g128": (4, 384, 264, 128, 70, (3, 2, 0)),
}
WEIGHT_RANGE_MAIN_ROWS = 48                              # 1..16 rows through the decode op, 24 and 48 through gptqhip_gemm


def weight_range_side_families(scale_dtype: str):
    """(scale family, code family) pairs every shape but the main one takes."""
    return ((("sub", "random"),) if scale_dtype == "fp16" else ()) + (("group_ramp", "random"), ("outlier_group", "random"), ("u0.01", "near_zero_point"))


def weight_range_main_families(act: str, scale_dtype: str, bits: int = 4):
    """... and the main shape: every scale family on uniform codes, every code family (but at_zero_point: its own tests) on u0.01."""
    return tuple((s, "random") for s in weight_scale_families(act, scale_dtype, bits)) + \
        tuple(("u0.01", c) for c in ("near_zero_point", "extremes", "sym"))


def weight_range_layer_of(shape: str, scale_family: str, code_family: str, scale_dtype: str):
    """-> (bits, K, N, gs, rows, (qweight, qzeros, scales, g_idx)) of one named case (the seed follows from the shape)."""
    if shape in WEIGHT_RANGE_DECODE_SHAPES:
        bits, K, N, gs, desc = WEIGHT_RANGE_DECODE_SHAPES[shape]
        rows = WEIGHT_RANGE_MAIN_ROWS if shape == WEIGHT_RANGE_MAIN else (1 if desc else (4 if shape == "2048x8192g128" else 16))
    else:
        bits, K, N, gs, rows, _ = WEIGHT_RANGE_TILED[shape]
        desc = False
    return bits, K, N, gs, rows, weight_range_layer(scale_family, code_family, bits, K, N, gs, scale_dtype, desc_act=desc, seed=K // 32 + N // 8 + gs + bits)
