"""GPU contract tests of the HIP entry points at their ragged edges, through the C ABI (vlp_amd._lib -> libvlp_hip.so).

tests/test_00_kernels_gpu.py checks every kernel on buffers that are exactly as large as their logical shape.  Here every operand comes from
tests/guard_util.py: leading dimensions strictly larger than the width, NaN in every byte a kernel has no business reading (guard rows
before and after, the [cols, ld) padding of every row, workspaces), a sentinel bit pattern in every byte of an output.  Per call:
  (a) the result against an fp32 / fp64 torch restatement with the bound test_00 uses for that op,
  (b) the zero band include/vlp_hip.h promises is exactly zero,
  (c) every output outside its write footprint, and every input, is bit-untouched,
  (d) the result is finite although everything around the operands is NaN.
The guards are deeper than the largest tile of the library, so an overrun lands inside the same allocation and fails an assertion.
"""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from vlp_amd import _lib as K          # noqa: E402
from oracle import vlp_oracle as O      # noqa: E402   (checker only)

from tests import guard_util as G                                                                      # noqa: E402
from tests.guard_util import roundup8                                                                  # noqa: E402
from tests.kernel_util import DEV, LAB, NT_PRODUCT, _adam_ref, attn_mask, attn_ref, drop_mult_ref, h16, rel      # noqa: E402
from tests.test_label_smoothing_cpu import smoothed_grad, smoothed_loss, smoothing_values              # noqa: E402

HALF, F32, I64, I32 = torch.float16, torch.float32, torch.int64, torch.int32


@pytest.fixture
def gen():
    g = torch.Generator(device=DEV)
    g.manual_seed(4321)
    return g


def gin(t, pad=8):
    """Guarded INPUT holding `t` ([rows, cols]): ld = roundup8(cols) + pad, NaN in the padding and in the guard rows."""
    return G.guarded(t.shape[0], t.shape[1], ld=roundup8(t.shape[1]) + pad, dtype=t.dtype, fill="nan", device=DEV).set(t)


def gout(rows, cols, pad=8, dtype=HALF, init=None):
    """Guarded OUTPUT: sentinel everywhere; `init` ([rows, cols]) is what an accumulating call (beta = 1) finds in the logical region."""
    g = G.guarded(rows, cols, ld=roundup8(cols) + pad, dtype=dtype, fill="sentinel", device=DEV)
    return g if init is None else g.set(init)


def vin(t, fill="nan"):
    return G.guarded_vec(t.numel(), t.dtype, fill=fill, device=DEV).set(t)


def vout(n, dtype=F32, init=None):
    g = G.guarded_vec(n, dtype, fill="sentinel", device=DEV)
    return g if init is None else g.set(init)


def nan_ws(nbytes):
    """A workspace of `nbytes` bytes filled with fp32 NaN: stale scratch must not matter."""
    return torch.full(((nbytes + 3) // 4 + 1,), float("nan"), device=DEV)


def check_out(g, ref, bound, written, name, zero_band=None):
    """(a) .. (d) for one guarded output."""
    G.assert_written(g, "logical", name)
    G.assert_finite(g.view, name)
    e = rel(g.view.float(), ref)
    assert e < bound, "%s: rel err %.3e >= %.1e" % (name, e, bound)
    if zero_band is not None:
        G.assert_zero_band(g, zero_band[0], zero_band[1], name)
    G.assert_untouched(g, written=written, name=name)


# =====================================================================================================
# vlp_gemm_nt
# =====================================================================================================
NT_VARIANTS = [0, 1, 2, 3, 5, 17, 19, 21, 27, 29, 77, 264]
NT_N = [28996, 3129, 1001, 129, 127, 7, 1]
NT_M = [1, 127, 129, 255, 257, 1280]
NT_EPI = ["plain", "bias", "gelu_preact", "save_grad", "residual", "mul_gelu_grad", "mul_plain", "dropout", "relu_mask"]


def _nt_cases():
    """Pairwise-style walk through variants x N x M x K x epilogue (not the full product); the large output (N = 28996, M = 1280) once."""
    cases = [(29, 1280, 28996, 768, "bias")]
    for i in range(48):
        v, N = NT_VARIANTS[i % 12], NT_N[(i + i // 12) % 7]
        M = NT_M[(5 * i + i // 6) % 6]
        if N == 28996 and M == 1280:
            M = 257
        cases.append((v, M, N, (64, 768)[(i // 3 + i // 12) % 2], NT_EPI[(2 * i + i // 9) % 9]))
    return cases


def _nt_run(variant, M, N, Kd, epi, x, w, ops):
    """One vlp_gemm_nt call; returns (y, preact) as guarded outputs."""
    n8 = roundup8(N)
    y = gout(M, N, pad=24)
    pre = gout(M, N, pad=40) if epi in ("gelu_preact", "save_grad") else None
    kw = dict(variant=variant)
    if epi in ("bias", "gelu_preact", "save_grad", "dropout"):
        kw["bias"] = ops["bias"].vec
    if epi == "gelu_preact":
        kw.update(preact=pre.view, act=K.ACT_GELU)
    if epi == "save_grad":
        kw.update(preact=pre.view, act=K.ACT_GELU_SAVE_GRAD)
    if epi in ("residual", "dropout"):
        kw["residual"] = ops["res"].view
    if epi == "residual":
        kw["alpha"] = 0.5
    if epi == "mul_gelu_grad":
        kw.update(mul_src=ops["src"].view, mul_mode=K.MUL_GELU_GRAD)
    if epi == "mul_plain":
        kw.update(mul_src=ops["src"].view, mul_mode=K.MUL_PLAIN)
    if epi == "relu_mask":
        kw.update(mul_src=ops["src"].view, mul_mode=K.MUL_RELU_MASK)
    if epi == "dropout":
        kw.update(dropout_p=0.3, seed=99, rng_stream=5)
    K.gemm_nt(x.view, w.view, y.view, M, N, Kd, **kw)
    assert y.view.stride(0) >= n8 + 8
    return y, pre


@pytest.mark.parametrize("variant,M,N,Kd,epi", _nt_cases())
def test_gemm_nt_ragged(variant, M, N, Kd, epi, gen):
    """Every product variant at a ragged N.  The persistent k-stream kernel (gemm_nt_ps.hip, variants 256 / 264) is NOT run here: it needs
    N % 128 == 0 and NT_N holds no multiple of 128, so a `variant = 264` case checks the launcher's fallback to a ring and nothing else.
    Neither is the lean multiplier instantiation of variants 21 / 29 (N % 16 == 0).  The kernels themselves under guards:
    tests/test_07_step_kernel_contract_gpu.py::test_gemm_nt_persistent_guarded and ::test_gemm_nt_lean_multiplier_guarded."""
    if not (LAB or variant in NT_PRODUCT):
        pytest.skip("investigation variant: needs a -DVLP_LAB_BUILD library")
    n8 = roundup8(N)
    x, w = gin(h16(M, Kd, gen=gen), pad=8), gin(h16(N, Kd, scale=0.05, gen=gen), pad=16)
    ops = {"bias": vin(h16(N, gen=gen)), "res": gin(h16(M, N, gen=gen), pad=8), "src": gin(h16(M, N, gen=gen), pad=16)}
    y, pre = _nt_run(variant, M, N, Kd, epi, x, w, ops)
    resolved = K.gemm_nt_resolved_variant()
    lin = x.view.float() @ w.view.float().t()
    lb = lin + ops["bias"].vec.float()
    bound = 1.5e-3           # fp32 accumulate, one fp16 rounding of the result (test_00)
    if epi == "plain":
        ref = lin
    elif epi == "bias":
        ref = lb
    elif epi == "gelu_preact":
        check_out(pre, lb, 1.5e-3, n8, "preact", zero_band=(N, n8))
        ref = O.gelu(pre.view.float())                     # gelu is applied to the fp16-rounded pre-activation
    elif epi == "save_grad":
        # the stored derivative is gelu'(z16) of the fp16-rounded pre-activation, which this call does not output: take z16 from an
        # ACT_GELU call of the same variant (the same chain, the same rounding), as test_gemm_nt_epilogues does
        z16 = torch.empty(M, n8, device=DEV, dtype=HALF)
        K.gemm_nt(x.view, w.view, torch.empty(M, n8, device=DEV, dtype=HALF), M, N, Kd, bias=ops["bias"].vec, preact=z16, act=K.ACT_GELU, variant=variant)
        assert rel(z16[:, :N].float(), lb) < 1.5e-3
        z = z16[:, :N].float().requires_grad_(True)
        O.gelu(z).sum().backward()
        check_out(pre, z.grad, 1.5e-3, n8, "preact(gelu')", zero_band=(N, n8))
        ref = O.gelu(z.detach())
    elif epi == "residual":
        ref = 0.5 * lin + ops["res"].view.float()
    elif epi == "mul_gelu_grad":
        s32 = ops["src"].view.float().requires_grad_(True)
        O.gelu(s32).sum().backward()
        ref, bound = lin * s32.grad, 2e-3                 # test_gemm_nt_epilogues
    elif epi == "mul_plain":
        ref = lin * ops["src"].view.float()
    elif epi == "relu_mask":
        ref = lin * (ops["src"].view.float() > 0)
    else:
        ref = lb * drop_mult_ref(0.3, 99, 5, range(M), range(N)) + ops["res"].view.float()        # exact mask: element (row m, col n)
    check_out(y, ref, bound, n8, "Y", zero_band=(N, n8))
    G.assert_untouched(x, name="X")
    G.assert_untouched(w, name="W")
    for k, g in ops.items():
        G.assert_untouched(g, name=k)
    if variant in (77, 264):
        # what the launcher does with a wave-pipelined / persistent variant at a ragged N (csrc/gemm_nt.hip).  264: no N of this list is a
        # multiple of 128, so the persistent kernel never runs here -- the launcher must fall back to a ring and say so; this is a test
        # of the fallback, not of gemm_nt_ps.hip (see the docstring).  77: the wave-pipelined kernel carries a ragged N itself and leaves
        # only the erf epilogues to a ring.  Either way the bits are the ring's (same ascending-k fp32 chains)
        ring = 29 if N > 1024 else 27
        erf = epi in ("gelu_preact", "mul_gelu_grad")
        if variant == 264:
            assert N % 128 != 0 and resolved == ring, (N, resolved)
        else:
            assert resolved == (ring if erf else 77), resolved
        y2, pre2 = _nt_run(ring, M, N, Kd, epi, x, w, ops)
        assert K.gemm_nt_resolved_variant() == ring
        assert torch.equal(G.bits(y.view), G.bits(y2.view))
        if pre is not None:
            assert torch.equal(G.bits(pre.view), G.bits(pre2.view))


# =====================================================================================================
# vlp_gemm_nt_splitk
# =====================================================================================================
@pytest.mark.parametrize("M,N,Kd,splits,epi", [(5, 28996, 768, 5, "plain"), (1, 3129, 768, 7, "bias_gelu"), (70, 1001, 768, 5, "bias_res"),
                                                (5, 129, 768, 7, "plain"), (70, 127, 768, 11, "bias_gelu"), (1, 7, 768, 5, "bias_res"),
                                                (70, 1, 192, 2, "plain"), (5, 1001, 64, 3, "bias_gelu")])
def test_gemm_nt_splitk_ragged(M, N, Kd, splits, epi, gen):
    """`splits` that do not divide K / 64 (12 k tiles into 5, 7, 11; 1 into 3), NaN workspace."""
    n8 = roundup8(N)
    x, w = gin(h16(M, Kd, gen=gen)), gin(h16(N, Kd, scale=0.05, gen=gen), pad=16)
    bias, res = vin(h16(N, gen=gen)), gin(h16(M, N, gen=gen))
    ws = nan_ws(K.gemm_nt_splitk_workspace_bytes(M, N, splits))
    y = gout(M, N, pad=24)
    lin = x.view.float() @ w.view.float().t()
    if epi == "plain":
        K.gemm_nt_splitk(x.view, w.view, y.view, M, N, Kd, splits, ws)
        ref, bound = lin, 1.5e-3
    elif epi == "bias_gelu":
        K.gemm_nt_splitk(x.view, w.view, y.view, M, N, Kd, splits, ws, bias=bias.vec, act=K.ACT_GELU)
        z = lin + bias.vec.float()
        ref, bound = z * 0.5 * (1 + torch.erf(z / math.sqrt(2))), 2e-3
    else:
        K.gemm_nt_splitk(x.view, w.view, y.view, M, N, Kd, splits, ws, bias=bias.vec, residual=res.view, alpha=0.5)
        ref, bound = 0.5 * lin + bias.vec.float() + res.view.float(), 2e-3
    check_out(y, ref, bound, n8, "Y", zero_band=(N, n8))
    for g, name in ((x, "X"), (w, "W"), (bias, "bias"), (res, "residual")):
        G.assert_untouched(g, name=name)


# =====================================================================================================
# vlp_gemm_tn, vlp_gemm_tn_grouped, vlp_colsum
# =====================================================================================================
def _tn_operands(M, N, Kd, beta, gen, with_bias=True):
    a, b = gin(h16(M, N, scale=0.3, gen=gen), pad=16), gin(h16(M, Kd, scale=0.3, gen=gen), pad=8)     # NaN in A's padding columns, NaN rows after M
    c0, b0 = h16(N, Kd, gen=gen), h16(N, gen=gen)
    c = gout(N, Kd, pad=8, init=c0 if beta else None)
    bias = vout(N, HALF, init=b0 if beta else None) if with_bias else None           # exactly N elements inside guards
    ref = a.view.float().t() @ b.view.float()
    cs = a.view.float().sum(0)
    if beta:
        ref, cs = ref + c0.float(), cs + b0.float()
    return a, b, c, bias, ref, cs


def _tn_check(a, b, c, bias, ref, cs, beta, Kd):
    check_out(c, ref, 2.5e-3 if beta else 1.5e-3, Kd, "C")          # C rows >= N, columns >= K untouched
    if bias is not None:
        G.assert_written(bias, "logical", "bias_out")
        G.assert_finite(bias.vec, "bias_out")
        # test_gemm_tn's bound for the fused column sums (fp16 result; + one more rounding when it accumulates)
        assert float((bias.vec.float() - cs).abs().max()) < 2e-3 * float(cs.abs().max()) + (2e-2 if beta else 1e-2)
        G.assert_untouched(bias, written="logical", name="bias_out")
    G.assert_untouched(a, name="A")
    G.assert_untouched(b, name="B")


@pytest.mark.parametrize("variant,M,N,Kd,beta,splits", [(0, 63, 1001, 64, 0, 1), (1, 333, 7, 768, 1, 2), (2, 2085, 3129, 128, 0, 0), (3, 65, 28996, 64, 1, 1),
                                                         (4, 1, 1001, 768, 0, 1), (9, 333, 3129, 72, 1, 0), (10, 65, 7, 64, 0, 3), (26, 2085, 1001, 768, 1, 0),
                                                         (2, 1, 7, 64, 1, 1), (10, 63, 28996, 128, 0, 0)])
def test_gemm_tn_ragged(variant, M, N, Kd, beta, splits, gen):
    """The contraction tail (M % 64 != 0: NaN rows after M in A and B) and the ragged N (NaN in A's columns [N, lda))."""
    a, b, c, bias, ref, cs = _tn_operands(M, N, Kd, beta, gen)
    ws = nan_ws(K.gemm_tn_workspace_bytes(M, N, Kd))
    K.gemm_tn(a.view, b.view, c.view, M, N, Kd, beta=beta, workspace=ws, variant=variant, splits=splits, bias_out=bias.vec)
    _tn_check(a, b, c, bias, ref, cs, beta, Kd)


@pytest.mark.parametrize("beta", [0, 1])
def test_gemm_tn_grouped_ragged(beta, gen):
    shapes = [(333, 1001, 64), (65, 7, 768), (2085, 3129, 128), (63, 28996, 64), (1, 1001, 72)]
    ops = [_tn_operands(M, N, Kd, beta, gen, with_bias=(i != 1)) for i, (M, N, Kd) in enumerate(shapes)]
    K.gemm_tn_grouped([(o[0].view, o[1].view, o[2].view, M, N, Kd, beta, o[3].vec if o[3] is not None else None) for o, (M, N, Kd) in zip(ops, shapes)])
    for o, (M, N, Kd) in zip(ops, shapes):
        _tn_check(*o, beta, Kd)


@pytest.mark.parametrize("M,N,beta", [(1, 28996, 0), (63, 1001, 1), (2085, 7, 0), (333, 3129, 1), (4097, 1001, 0)])
def test_colsum_ragged(M, N, beta, gen):
    a = gin(h16(M, N, gen=gen), pad=16)
    o0 = h16(N, gen=gen)
    out = vout(N, HALF, init=o0 if beta else None)
    K.colsum(a.view, out.vec, M, N, beta=beta, workspace=nan_ws(K.colsum_workspace_bytes(M, N)))
    ref = a.view.float().sum(0) + (o0.float() if beta else 0)
    G.assert_written(out, "logical", "out")
    G.assert_finite(out.vec, "out")
    assert float((out.vec.float() - ref).abs().max()) < 1e-3 * float(ref.abs().max()) + 1e-2           # test_colsum
    G.assert_untouched(out, written="logical", name="out")
    G.assert_untouched(a, name="A")


# =====================================================================================================
# attention
# =====================================================================================================
def _pack_masks(mask, B, L):
    Lp = (L + 31) // 32 * 32
    mb = torch.empty(B, L, Lp, device=DEV, dtype=torch.uint8)
    mt = torch.empty(B, Lp, Lp, device=DEV, dtype=torch.uint8)
    K.mask_pack(mask, mb, B, L, Lp, out_t=mt)
    return mb, mt


@pytest.mark.parametrize("B,L,Nv,heads,p", [(1, 17, 8, 2, 0.0), (3, 33, 8, 12, 0.1), (3, 43, 8, 2, 0.0), (1, 123, 100, 12, 0.1), (3, 167, 100, 12, 0.0),
                                             (1, 193, 100, 2, 0.1), (3, 255, 100, 2, 0.1), (1, 256, 100, 12, 0.0), (3, 256, 100, 2, 0.1)])
def test_attention_dense_guarded(B, L, Nv, heads, p, gen):
    """B = 1 and the LAST sequence of B = 3: the key / value tile that runs past the last row of qkv finds NaN there (guard rows), as does
    the dO / ctx tile of the backward; ld_qkv > 3H, ld_ctx > H; lse / delta guarded."""
    H, seed, stream = heads * 64, 7, 11
    mask = attn_mask(B, L, Nv, torch.Generator().manual_seed(5)).to(DEV)
    mb, mt = _pack_masks(mask, B, L)
    qkv = gin(h16(B * L, 3 * H, gen=gen), pad=8)
    ctx = gout(B * L, H, pad=8)
    lse = vout(B * heads * L)
    K.attn_fwd(qkv.view, mb, ctx.view, lse.vec, B, L, heads, 0.125, dropout_p=p, seed=seed, rng_stream=stream)
    mult = drop_mult_ref(p, seed, stream, range(B * heads * L), range(L)).view(B, heads, L, L).double() if p else None
    q64 = qkv.view.contiguous().double().requires_grad_(True)
    ref, _ = attn_ref(q64, mask, B, L, heads, mult)
    check_out(ctx, ref, 2e-3, "logical", "ctx")                     # P and O rounded to fp16 once each (test_attention_fwd_bwd)
    assert rel(ctx.view[(B - 1) * L:].float(), ref[(B - 1) * L:]) < 2e-3, "last sequence"
    x = q64.detach().view(B, L, 3, heads, 64)
    s = (x[:, :, 0].permute(0, 2, 1, 3) @ x[:, :, 1].permute(0, 2, 3, 1)) / 8.0 + (1.0 - mask.double())[:, None] * -10000.0
    G.assert_written(lse, "logical", "lse")
    assert float((lse.vec.view(B, heads, L).double() - torch.logsumexp(s, -1)).abs().max()) < 1e-3
    G.assert_untouched(lse, written="logical", name="lse")
    G.assert_untouched(qkv, name="qkv")
    # backward
    ctx_in = gin(ctx.view.contiguous(), pad=16)
    dctx = gin(h16(B * L, H, gen=gen), pad=24)
    lse_in = vin(lse.vec.clone())
    dqkv = gout(B * L, 3 * H, pad=16)
    delta = vout(B * heads * L)
    K.attn_bwd(qkv.view, mb, mt, ctx_in.view, dctx.view, lse_in.vec, dqkv.view, delta.vec, B, L, heads, 0.125, dropout_p=p, seed=seed, rng_stream=stream)
    ref.backward(dctx.view.double())
    G.assert_written(dqkv, "logical", "dqkv")
    G.assert_finite(dqkv.view, "dqkv")
    last = slice((B - 1) * L, B * L)
    if p:                                                           # test_attention_dropout_exact_mask: the whole dqkv, 5e-3
        assert rel(dqkv.view.float(), q64.grad) < 5e-3
        assert rel(dqkv.view[last].float(), q64.grad[last]) < 5e-3, "last sequence"
    else:                                                           # test_attention_fwd_bwd: dq, dk, dv each, 4e-3
        for i, name in enumerate(("dq", "dk", "dv")):
            a, r = dqkv.view[:, i * H:(i + 1) * H].float(), q64.grad[:, i * H:(i + 1) * H]
            assert rel(a, r) < 4e-3, name
            assert rel(a[last], r[last]) < 4e-3, name + " (last sequence)"
    G.assert_untouched(dqkv, written="logical", name="dqkv")
    G.assert_untouched(delta, written="logical", name="delta")
    for g, name in ((qkv, "qkv"), (ctx_in, "ctx"), (dctx, "dctx"), (lse_in, "lse")):
        G.assert_untouched(g, name=name)


@pytest.mark.parametrize("L,drop", [(167, 0.1), (123, 0.0), (43, 0.1)])
def test_attention_packed_guarded(L, drop):
    """row_off packed rows: the last sequence ends at the last packed row, NaN guard rows follow it.  Truth: the dense launch on plain
    buffers, bit for bit (tests/test_25_varlen_gpu.py::test_attention_packed_rows_equal_dense)."""
    from vlp_amd.input_prep import MaskSpec
    B, A, H, Nv = 3, 12, 768, 30 if L > 60 else 8
    rng = np.random.RandomState(3)
    nb = rng.randint(1, L - Nv - 3, size=B)
    spec = MaskSpec.from_lengths(Nv, nb.tolist(), [True, False, True], device=DEV)
    lens = spec.lens_host
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    Mp = int(off[-1])
    row_off = vin(torch.from_numpy(off).to(DEV), fill=Mp)          # guards: the offset of the NaN guard rows that follow the last packed row
    row_map = torch.empty(Mp, dtype=I32, device=DEV)
    K.rowmap_build(row_off.vec, B, L, row_map)
    Lp = (L + 31) // 32 * 32
    maskb, maskt = torch.empty(B, L, Lp, dtype=torch.uint8, device=DEV), torch.empty(B, Lp, Lp, dtype=torch.uint8, device=DEV)
    K.mask_build(spec.second_st, spec.second_end, spec.is_s2s, maskb, B, L, Lp, out_t=maskt)
    g = torch.Generator(device=DEV).manual_seed(4)
    qkv = (torch.randn(B * L, 3 * H, device=DEV, generator=g) * 0.7).half()
    dctx = (torch.randn(B * L, H, device=DEV, generator=g) * 0.3).half()
    keep = torch.zeros(B * L, dtype=torch.bool, device=DEV)
    keep[row_map.long()] = True
    dctx[~keep] = 0
    ctx0, lse0 = torch.zeros(B * L, H, device=DEV, dtype=HALF), torch.zeros(B, A, L, device=DEV)
    K.attn_fwd(qkv, maskb, ctx0, lse0, B, L, A, 0.125, dropout_p=drop, seed=11, rng_stream=17)
    dq0, dl0 = torch.zeros(B * L, 3 * H, device=DEV, dtype=HALF), torch.zeros(B, A, L, device=DEV)
    K.attn_bwd(qkv, maskb, maskt, ctx0, dctx, lse0, dq0, dl0, B, L, A, 0.125, dropout_p=drop, seed=11, rng_stream=17)
    qkv_p, dctx_p = gin(qkv[row_map.long()], pad=8), gin(dctx[row_map.long()], pad=24)
    ctx1, lse1 = gout(Mp, H, pad=8), vout(B * A * L)
    K.attn_fwd(qkv_p.view, maskb, ctx1.view, lse1.vec, B, L, A, 0.125, dropout_p=drop, seed=11, rng_stream=17, row_off=row_off.vec)
    G.assert_written(ctx1, "logical", "ctx")
    assert torch.equal(G.bits(ctx0[row_map.long()]), G.bits(ctx1.view))
    kept_q = keep.view(B, 1, L).expand(B, A, L)
    assert torch.equal(lse0[kept_q], lse1.vec.view(B, A, L)[kept_q])
    G.assert_untouched(ctx1, written="logical", name="ctx")
    G.assert_untouched(lse1, written="logical", name="lse")
    ctx_in = gin(ctx1.view.contiguous(), pad=16)
    dq1, dl1 = gout(Mp, 3 * H, pad=16), vout(B * A * L)
    K.attn_bwd(qkv_p.view, maskb, maskt, ctx_in.view, dctx_p.view, lse1.vec, dq1.view, dl1.vec, B, L, A, 0.125, dropout_p=drop, seed=11, rng_stream=17,
               row_off=row_off.vec)
    G.assert_written(dq1, "logical", "dqkv")
    assert torch.equal(G.bits(dq0[row_map.long()]), G.bits(dq1.view))
    G.assert_untouched(dq1, written="logical", name="dqkv")
    G.assert_untouched(dl1, written="logical", name="delta")
    for gd, name in ((qkv_p, "qkv"), (ctx_in, "ctx"), (dctx_p, "dctx"), (row_off, "row_off")):
        G.assert_untouched(gd, name=name)


# =====================================================================================================
# LayerNorm
# =====================================================================================================
@pytest.mark.parametrize("M,H,p", [(1, 64, 0.0), (5, 520, 0.2), (257, 768, 0.0), (1, 1032, 0.2), (5, 2048, 0.0), (257, 64, 0.2), (257, 1032, 0.0),
                                    (1, 768, 0.2), (5, 4096, 0.0), (257, 2048, 0.2), (257, 520, 0.0)])
def test_layernorm_guarded(M, H, p, gen):
    """ldx, ldy, lddy, lddx > H (all different), NaN rows after M, mean / rstd / dgamma / dbeta guarded; p > 0: both dropout paths with the
    exact masks; H = 4096 forward only."""
    x = gin(h16(M, H, scale=2.0, gen=gen), pad=8)
    gamma, beta = vin((1 + 0.1 * torch.randn(H, device=DEV, generator=gen)).half()), vin(h16(H, scale=0.1, gen=gen))
    y = gout(M, H, pad=16)
    mean, rstd = vout(M), vout(M)
    K.layernorm_fwd(x.view, gamma.vec, beta.vec, y.view, M, H, mean.vec, rstd.vec, dropout_p=p, seed=3, rng_stream=9)
    mult = drop_mult_ref(p, 3, 9, range(M), range(H)).double()
    x64 = x.view.double().requires_grad_(True)
    g64, b64 = gamma.vec.double().requires_grad_(True), beta.vec.double().requires_grad_(True)
    ref = O.layer_norm(x64, g64, b64) * mult
    check_out(y, ref, 1.5e-3, "logical", "y")
    for g, want, name in ((mean, x64.detach().mean(1), "mean"), (rstd, 1.0 / torch.sqrt(x64.detach().var(1, unbiased=False) + 1e-5), "rstd")):
        G.assert_written(g, "logical", name)
        if name == "mean" and M == 1:
            # one row: the max-normalised metric would divide by that row's own (possibly tiny) mean.  An fp32 mean of H values carries
            # at most H * 2^-24 relative to max|x| (6e-5 at H = 1032 in the worst case, ~1e-7 typical): 1e-5 of max|x| is the same bound
            # as test_layernorm_fwd_wide's on its natural scale
            assert float((g.vec.double() - want).abs().max()) < 1e-5 * float(x64.detach().abs().max()), name
        else:
            assert rel(g.vec, want) < 1e-5, name                   # test_layernorm_fwd_wide
        G.assert_untouched(g, written="logical", name=name)
    for g, name in ((x, "x"), (gamma, "gamma"), (beta, "beta")):
        G.assert_untouched(g, name=name)
    if H > 2048:
        return
    dy = gin(h16(M, H, gen=gen), pad=24)
    mean_in, rstd_in = vin(mean.vec.clone()), vin(rstd.vec.clone())
    dx, dxd = gout(M, H, pad=8), gout(M, H, pad=32) if p else None
    dg, db = vout(H, HALF), vout(H, HALF)
    ws = nan_ws(K.layernorm_bwd_workspace_bytes(H))
    K.layernorm_bwd(dy.view, x.view, gamma.vec, mean_in.vec, rstd_in.vec, dx.view, dg.vec, db.vec, M, H, ws, dx_drop=dxd.view if p else None,
                    dy_drop=(p, 3, 9), out_drop=(0.1 if p else 0.0, 4, 2))
    ref.backward(dy.view.double())
    check_out(dx, x64.grad, 2e-3, "logical", "dx")
    if p:
        check_out(dxd, x64.grad * drop_mult_ref(0.1, 4, 2, range(M), range(H)), 2e-3, "logical", "dx_drop")
    for g, want, name in ((dg, g64.grad, "dgamma"), (db, b64.grad, "dbeta")):
        G.assert_written(g, "logical", name)
        G.assert_finite(g.vec, name)
        assert rel(g.vec.float(), want) < 3e-3, name
        G.assert_untouched(g, written="logical", name=name)
    for g, name in ((x, "x"), (dy, "dy"), (gamma, "gamma"), (mean_in, "mean"), (rstd_in, "rstd")):
        G.assert_untouched(g, name=name)


@pytest.mark.parametrize("M,H", [(4100, 768), (4100, 520)])
def test_layernorm_bwd_rows_per_wave_guarded(M, H, gen):
    """M = 4100 is the smallest M at which some waves of the backward walk two rows and the others one (4096 waves in the grid): the
    next-row prefetch, its rotation into the current row (statistics and LOGICAL row index included) and the tail of the walk run here,
    which no M <= 4096 reaches.  Packed rows (row_map with gaps: the masks are those of the logical rows), both dropouts, every leading
    dimension different and > H, NaN behind row M; bounds of test_layernorm_guarded."""
    rm = torch.arange(M, device=DEV)
    rm = (rm + rm // 100).to(I32)
    row_map = vin(rm, fill=0)
    x = gin(h16(M, H, scale=2.0, gen=gen), pad=8)
    gamma, beta = vin((1 + 0.1 * torch.randn(H, device=DEV, generator=gen)).half()), h16(H, scale=0.1, gen=gen)
    dy = gin(h16(M, H, gen=gen), pad=24)
    x64 = x.view.double().requires_grad_(True)
    g64, b64 = gamma.vec.double().requires_grad_(True), beta.double().requires_grad_(True)
    mult = drop_mult_ref(0.2, 3, 9, rm.tolist(), range(H)).double()
    ref = O.layer_norm(x64, g64, b64) * mult
    ref.backward(dy.view.double())
    xd = x64.detach()
    mean_in, rstd_in = vin(xd.mean(1).float()), vin((1.0 / torch.sqrt(xd.var(1, unbiased=False) + 1e-5)).float())
    dx, dxd = gout(M, H, pad=16), gout(M, H, pad=32)
    dg, db = vout(H, HALF), vout(H, HALF)
    ws = nan_ws(K.layernorm_bwd_workspace_bytes(H))
    K.layernorm_bwd(dy.view, x.view, gamma.vec, mean_in.vec, rstd_in.vec, dx.view, dg.vec, db.vec, M, H, ws, dx_drop=dxd.view,
                    dy_drop=(0.2, 3, 9), out_drop=(0.1, 4, 2), row_map=row_map.vec)
    check_out(dx, x64.grad, 2e-3, "logical", "dx")
    check_out(dxd, x64.grad * drop_mult_ref(0.1, 4, 2, rm.tolist(), range(H)), 2e-3, "logical", "dx_drop")
    for g, want, name in ((dg, g64.grad, "dgamma"), (db, b64.grad, "dbeta")):
        G.assert_written(g, "logical", name)
        G.assert_finite(g.vec, name)
        assert rel(g.vec.float(), want) < 3e-3, name
        G.assert_untouched(g, written="logical", name=name)
    for g, name in ((x, "x"), (dy, "dy"), (gamma, "gamma"), (mean_in, "mean"), (rstd_in, "rstd"), (row_map, "row_map")):
        G.assert_untouched(g, name=name)


@pytest.mark.parametrize("M,H", [(5, 768), (257, 1032)])
def test_layernorm_deferred_reduce_guarded(M, H, gen):
    """defer_reduce leaves dgamma / dbeta bit-untouched; the batched second stage writes exactly [H] of each, accumulating (beta = 1)."""
    n = 2
    slot = K.layernorm_bwd_workspace_bytes(H)
    slots = nan_ws(n * slot)
    dst, keep = [], []
    for i in range(n):
        x = gin(h16(M, H, scale=2.0, gen=gen))
        gamma = vin((1 + 0.1 * torch.randn(H, device=DEV, generator=gen)).half())
        xf = x.view.float()
        mean, var = xf.mean(1), xf.var(1, unbiased=False)
        mean_in, rstd_in = vin(mean), vin(1.0 / torch.sqrt(var + 1e-5))
        dy = gin(h16(M, H, gen=gen), pad=24)
        g0, b0 = h16(H, gen=gen), h16(H, gen=gen)
        dg, db = vout(H, HALF, init=g0), vout(H, HALF, init=b0)
        dx = gout(M, H)
        K.layernorm_bwd(dy.view, x.view, gamma.vec, mean_in.vec, rstd_in.vec, dx.view, dg.vec, db.vec, M, H,
                        slots.view(torch.uint8)[i * slot:(i + 1) * slot], beta=1, defer_reduce=True)
        G.assert_untouched(dg, name="dgamma (deferred)")
        G.assert_untouched(db, name="dbeta (deferred)")
        xh = (xf - mean[:, None]) / torch.sqrt(var + 1e-5)[:, None]
        keep.append((dg, db, g0.float() + (dy.view.float() * xh).sum(0), b0.float() + dy.view.float().sum(0), x, dy, dx))
        dst.append([dg.vec.data_ptr(), db.vec.data_ptr()])
    K.layernorm_bwd_reduce_batched(slots, torch.tensor(dst, dtype=I64, device=DEV), n, M, H, beta=1)
    for dg, db, wg, wb, x, dy, dx in keep:
        for g, want, name in ((dg, wg, "dgamma"), (db, wb, "dbeta")):
            G.assert_finite(g.vec, name)
            assert rel(g.vec.float(), want) < 4e-3, name           # accumulated: test_layernorm_fwd_bwd's beta = 1 bound
            G.assert_untouched(g, written="logical", name=name)
        G.assert_untouched(x, name="x")
        G.assert_untouched(dy, name="dy")
        G.assert_untouched(dx, written="logical", name="dx")


# =====================================================================================================
# losses
# =====================================================================================================
def _ce_inputs(B, P, V, gen, ld_pad=8):
    logits = gin(h16(B * P, V, scale=2.0, gen=gen), pad=ld_pad)                       # NaN in [V, ld)
    lab = torch.randint(0, V, (B * P,), device=DEV, generator=gen)
    lab[0], lab[-1] = 0, V - 1
    if B * P > 2:
        lab[1] = V - 1
    # labels index the columns of their own logits row, and every column of it enters the lse: there is no row or column to reserve as
    # poison for them, so their guards hold the valid label 0 (a stray read stays in bounds; only the numbers would show it).  weights are
    # values, not indices.
    labels = vin(lab, fill=0)
    w = (torch.rand(B * P, device=DEV, generator=gen) < 0.7).long()
    w.view(B, P)[:, 0] = 1
    weights = vin(w, fill=1)
    return logits, labels, weights


def _ls_scalars(ls, V, dtype=torch.float16):
    s, c = smoothing_values(ls, V, dtype)
    sc = torch.tensor([s, c], dtype=dtype, device=DEV)
    xs, xc = (float(v) for v in torch.xlogy(sc, sc))
    return s, c, (V - 2) * s + c, (V - 2) * xs + xc


@pytest.mark.parametrize("B,P,V,ratio", [(16, 3, 28996, 0.3), (1, 1, 28996, 0.0), (5, 2, 1001, 0.2), (4, 3, 17, 0.0), (3, 1, 8, 0.3), (2, 2, 1, 0.0)])
@pytest.mark.parametrize("smoothed", [False, True])
def test_mlm_loss_guarded(B, P, V, ratio, smoothed, gen):
    if smoothed and V <= 2:
        with pytest.raises(RuntimeError):                           # V > 2 is part of the contract: refused, not mis-computed
            f = torch.zeros(B * P, device=DEV)
            K.mlm_loss_ls_fwd(torch.zeros(B * P, 8, device=DEV, dtype=HALF), 8, f.long(), f.long(), f, f, f, f, B, P, V, 0.1, 0.9, 1.0, 0.0)
        return
    rows = B * P
    logits, labels, weights = _ce_inputs(B, P, V, gen)
    ld = logits.ld
    loss, lse, coef, row = vout(1), vout(rows), vout(rows), vout(rows)
    x = logits.view.float().view(B, P, V)
    lab2, w2 = labels.vec.view(B, P), weights.vec.view(B, P)
    if smoothed:
        s, c, q_sum, q_log_q = _ls_scalars(0.1, V)
        K.mlm_loss_ls_fwd(logits.view, ld, labels.vec, weights.vec, loss.vec, lse.vec, coef.vec, row.vec, B, P, V, s, c, q_sum, q_log_q,
                          ignore_index=0, drop_worst_ratio=ratio)
        want = float(smoothed_loss(x, lab2, w2, s, c, ratio, qlogq_dtype=torch.float16))
        gref = smoothed_grad(x, lab2, w2, s, c, ratio, qlogq_dtype=torch.float16) * 128.0
    else:
        K.mlm_loss_fwd(logits.view, ld, labels.vec, weights.vec, loss.vec, lse.vec, coef.vec, row.vec, B, P, V, drop_worst_ratio=ratio)
        x64 = x.double().requires_grad_(True)
        ce = torch.nn.functional.cross_entropy(x64.transpose(1, 2), lab2, reduction="none") if V > 1 else (torch.logsumexp(x64, -1) - x64[..., 0])
        ref = O.loss_mask_and_normalize(ce, w2, ratio)
        (ref * 128.0).backward()
        want, gref = float(ref), x64.grad.view(rows, V)
    for g, name in ((loss, "loss"), (lse, "lse"), (coef, "coef")):
        G.assert_written(g, "logical", name)
        G.assert_finite(g.vec, name)                                # the NaN of [V, ld) must not be part of an lse
        G.assert_untouched(g, written="logical", name=name)
    G.assert_untouched(row, written="logical", name="row_loss")
    assert abs(float(loss.vec) - want) <= 1e-4 * abs(want), (float(loss.vec), want)       # test_mlm_loss
    assert float((lse.vec.double() - torch.logsumexp(x.double().view(rows, V), -1)).abs().max()) < 1e-3
    lse_in, coef_in = vin(lse.vec.clone()), vin(coef.vec.clone())
    gs = vin(torch.full((1,), 128.0, device=DEV))
    dl = gout(rows, V, pad=24)
    if smoothed:
        K.mlm_loss_ls_bwd(logits.view, ld, labels.vec, lse_in.vec, coef_in.vec, gs.vec, dl.view, dl.ld, rows, V, s, c, q_sum, ignore_index=0)
    else:
        K.mlm_loss_bwd(logits.view, ld, labels.vec, lse_in.vec, coef_in.vec, gs.vec, dl.view, dl.ld, rows, V)
    G.assert_written(dl, "rows", "dlogits")                         # the whole row up to ld_dlogits is written: gradient, then zeros
    G.assert_finite(dl.view, "dlogits")
    if float(gref.abs().max()) > 0:
        assert rel(dl.view.float(), gref) < 2e-3
    else:
        assert float(dl.view.float().abs().max()) == 0
    G.assert_zero_band(dl, V, dl.ld, "dlogits")
    G.assert_untouched(dl, written="rows", name="dlogits")
    for g, name in ((logits, "logits"), (labels, "labels"), (weights, "weights"), (lse_in, "lse"), (coef_in, "coef"), (gs, "grad_scale")):
        G.assert_untouched(g, name=name)


@pytest.mark.parametrize("smoothed", [False, True])
@pytest.mark.parametrize("r", [0.05, 0.1, 0.15, 0.2, 0.3, 0.4, 0.6])
def test_mlm_loss_drop_worst_count(r, smoothed, gen):
    """The number of kept samples is Python's int(B * (1 - r)) with the caller's double r, although the ABI carries r as a float
    (csrc/keep_count.h): 1 - float(0.2) is 1.2e-8 short of 0.8, and B = 40 used to keep 31 samples where the reference keeps 32.  All
    weights 1, per-sample losses distinct: the kept set is torch.topk(..., largest=False)'s and the loss is the reference's."""
    P, V, ld = 2, 64, 72
    for B in (5, 10, 40, 50, 60, 64, 80, 100):
        logits = torch.full((B * P, ld), float("nan"), device=DEV, dtype=HALF)
        logits[:, :V] = h16(B * P, V, scale=2.0, gen=gen)
        labels = torch.randint(1, V, (B, P), device=DEV, generator=gen)
        weights = torch.ones(B, P, dtype=I64, device=DEV)
        loss, lse, coef, row = (torch.zeros(n, device=DEV) for n in (1, B * P, B * P, B * P))
        x = logits[:, :V].float().view(B, P, V)
        if smoothed:
            s, c, q_sum, q_log_q = _ls_scalars(0.1, V)
            K.mlm_loss_ls_fwd(logits, ld, labels, weights, loss, lse, coef, row, B, P, V, s, c, q_sum, q_log_q, ignore_index=0, drop_worst_ratio=r)
            want = float(smoothed_loss(x, labels, weights, s, c, r, qlogq_dtype=torch.float16))
        else:
            K.mlm_loss_fwd(logits, ld, labels, weights, loss, lse, coef, row, B, P, V, drop_worst_ratio=r)
            want = float(O.loss_mask_and_normalize(torch.nn.functional.cross_entropy(x.double().transpose(1, 2), labels, reduction="none"), weights, r))
        per_sample = row.view(B, P).sum(-1)
        assert per_sample.unique().numel() == B                     # distinct: the kept set is well defined
        keep_n = int(B * (1 - r))
        kept = (coef.view(B, P) != 0).all(-1)
        assert bool(((coef.view(B, P) != 0).any(-1) == kept).all())
        assert int(kept.sum()) == keep_n, "B = %d, r = %g: %d samples kept, the reference keeps int(B * (1 - r)) = %d" % (B, r, int(kept.sum()), keep_n)
        _, idx = torch.topk(per_sample, keep_n, largest=False)
        want_set = torch.zeros(B, dtype=torch.bool, device=DEV)
        want_set[idx] = True
        assert torch.equal(kept, want_set), "B = %d, r = %g: kept set differs from topk(largest=False)" % (B, r)
        assert abs(float(loss) - want) <= 1e-4 * abs(want), (B, r, float(loss), want)


@pytest.mark.parametrize("R,V", [(48, 28996), (1, 1001), (5, 17), (3, 8), (2, 1)])
def test_token_logprob_guarded(R, V, gen):
    logits, ids, _ = _ce_inputs(R, 1, V, gen)
    logp, lse = vout(R), vout(R)
    K.token_logprob_fwd(logits.view, logits.ld, ids.vec, logp.vec, lse.vec, R, V)
    x64 = logits.view.double().requires_grad_(True)
    lp = torch.log_softmax(x64, -1).gather(1, ids.vec[:, None])[:, 0]
    for g, want, name in ((logp, lp.detach(), "logp"), (lse, torch.logsumexp(x64.detach(), -1), "lse")):
        G.assert_written(g, "logical", name)
        G.assert_finite(g.vec, name)
        assert float((g.vec.double() - want).abs().max()) < 1e-3, name          # lse bound of test_00 (absolute, |lse| ~ 12)
        G.assert_untouched(g, written="logical", name=name)
    grow = vin(torch.randn(R, device=DEV, generator=gen) * 64.0)
    lse_in = vin(lse.vec.clone())
    dl = gout(R, V, pad=24)
    K.token_logprob_bwd(logits.view, logits.ld, ids.vec, lse_in.vec, grow.vec, dl.view, dl.ld, R, V)
    (lp * grow.vec.double()).sum().backward()
    G.assert_written(dl, "rows", "dlogits")
    G.assert_finite(dl.view, "dlogits")
    if V > 1:
        assert rel(dl.view.float(), x64.grad) < 2e-3
    else:
        assert float(dl.view.float().abs().max()) == 0             # one class: the gradient vanishes identically
    G.assert_zero_band(dl, V, dl.ld, "dlogits")
    G.assert_untouched(dl, written="rows", name="dlogits")
    for g, name in ((logits, "logits"), (ids, "ids"), (grow, "g"), (lse_in, "lse")):
        G.assert_untouched(g, name=name)
    # The CE loss and the token log-prob are two policies of one forward and one backward kernel template (csrc/loss.hip): with labels = ids,
    # weights 1, one position per sample and nothing dropped they agree bit for bit -- a - b == -(b - a) and (-c)(o - p) == c(p - o) exactly.
    ones = vin(torch.ones(R, dtype=I64, device=DEV), fill=1)
    loss, lse_ce, coef, row = vout(1), vout(R), vout(R), vout(R)
    K.mlm_loss_fwd(logits.view, logits.ld, ids.vec, ones.vec, loss.vec, lse_ce.vec, coef.vec, row.vec, R, 1, V, drop_worst_ratio=0.0)
    assert torch.equal(G.bits(lse_ce.vec), G.bits(lse.vec)), "lse: mlm_loss_fwd vs token_logprob_fwd"
    assert torch.equal(row.vec, -logp.vec), "row_loss vs -logp"      # by value: one class gives +0 against -0
    one = vin(torch.ones(1, device=DEV))
    neg_coef = vin(-coef.vec)
    dl_ce, dl_tok = gout(R, V, pad=24), gout(R, V, pad=24)
    K.mlm_loss_bwd(logits.view, logits.ld, ids.vec, lse_in.vec, coef.vec, one.vec, dl_ce.view, dl_ce.ld, R, V)
    K.token_logprob_bwd(logits.view, logits.ld, ids.vec, lse_in.vec, neg_coef.vec, dl_tok.view, dl_tok.ld, R, V)
    assert torch.equal(dl_ce.full, dl_tok.full), "dlogits [R, ldd]: mlm_loss_bwd(coef) vs token_logprob_bwd(-coef)"


@pytest.mark.parametrize("B,N", [(7, 3129), (1, 1001), (3, 17), (2, 8), (5, 1)])
def test_bce_loss_guarded(B, N, gen):
    logits = gin(h16(B, N, scale=3.0, gen=gen), pad=8)
    y = gin(torch.rand(B, N, device=DEV, generator=gen), pad=8)
    loss = vout(257)
    K.bce_loss_fwd(logits.view, logits.ld, y.view, y.ld, B, N, loss.vec)
    x64 = logits.view.double().requires_grad_(True)
    ref = torch.nn.functional.binary_cross_entropy_with_logits(x64, y.view.double()) * N
    assert math.isfinite(float(loss.vec[0])) and abs(float(loss.vec[0]) - float(ref)) < 1e-4 * abs(float(ref))
    G.assert_untouched(loss, written="logical", name="loss")
    gs = vin(torch.full((1,), 64.0, device=DEV))
    d = gout(B, N, pad=24)
    K.bce_loss_bwd(logits.view, logits.ld, y.view, y.ld, B, N, gs.vec, d.view, d.ld)
    (ref * 64.0).backward()
    G.assert_written(d, "rows", "dlogits")
    G.assert_finite(d.view, "dlogits")
    assert rel(d.view.float(), x64.grad) < 2e-3
    G.assert_zero_band(d, N, d.ld, "dlogits")                       # "zero for columns >= N"
    G.assert_untouched(d, written="rows", name="dlogits")
    for g, name in ((logits, "logits"), (y, "labels"), (gs, "grad_scale")):
        G.assert_untouched(g, name=name)


@pytest.mark.parametrize("rows,V", [(6, 28996), (1, 1001), (3, 17), (2, 8), (4, 1)])
def test_argmax_topk_sample_guarded(rows, V, gen):
    """The NaN of [V, ld) must never be an argmax, a top-k entry, a sample or part of an lse; the largest logit sits in the LAST valid
    column of row 0 and in column 0 of the last row."""
    t = h16(rows, V, scale=2.0, gen=gen)
    t[0, V - 1] = 30.0
    t[-1, 0] = 31.0 if rows > 1 else t[-1, 0]
    logits = gin(t, pad=8)
    ld = logits.ld
    want_v, want_i = logits.view.float().max(1)
    ids, vals = vout(rows, I64), vout(rows)
    K.argmax_rows(logits.view, ld, rows, V, ids.vec, vals.vec)
    assert torch.equal(ids.vec, want_i) and torch.equal(vals.vec, want_v)
    ida, idb, v2 = vout(rows, I64), vout(rows, I64), vout(rows)
    K.argmax_rows2(logits.view, ld, rows, V, ida.vec, idb.vec, v2.vec)
    assert torch.equal(ida.vec, want_i) and torch.equal(idb.vec, want_i) and torch.equal(v2.vec, want_v)
    for g, name in ((ids, "ids"), (vals, "vals"), (ida, "ids_a"), (idb, "ids_b"), (v2, "vals2")):
        G.assert_untouched(g, written="logical", name=name)
    Kb = min(5, V)
    sc = G.guarded(rows, Kb, ld=Kb, dtype=F32, fill="sentinel", device=DEV)            # [rows, K] contiguous, as the entry point defines it
    oi = G.guarded(rows, Kb, ld=Kb, dtype=I64, fill="sentinel", device=DEV)
    K.logsoftmax_topk(logits.view, ld, rows, V, Kb, sc.view, oi.view)
    ws, wi = torch.topk(torch.log_softmax(logits.view.double(), -1), Kb, dim=-1)
    G.assert_finite(sc.view, "top-k scores")
    assert float((sc.view.double() - ws).abs().max()) < 1e-3
    assert bool(((oi.view >= 0) & (oi.view < V)).all())
    assert torch.equal(oi.view[:, 0], want_i)
    G.assert_untouched(sc, written="logical", name="out_scores")
    G.assert_untouched(oi, written="logical", name="out_ids")
    sid, slp = vout(rows, I64), vout(rows)
    K.sample_rows(logits.view, ld, rows, V, 17, 3, sid.vec, slp.vec)
    assert bool(((sid.vec >= 0) & (sid.vec < V)).all())
    G.assert_finite(slp.vec, "sample logp")
    lsm = torch.log_softmax(logits.view.double(), -1).gather(1, sid.vec[:, None])[:, 0]
    assert float((slp.vec.double() - lsm).abs().max()) < 1e-3
    G.assert_untouched(sid, written="logical", name="sample ids")
    G.assert_untouched(slp, written="logical", name="sample logp")
    G.assert_untouched(logits, name="logits")


# =====================================================================================================
# optimizers and elementwise kernels: small sizes, wave-run edges, past the grid caps
# =====================================================================================================
def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _sumsq_sizes():
    # 8; one element short of / past a 512-element wave run; past the 1024-block cap (csrc/adam.hip SQ_BLOCKS) with a ragged remainder
    return [8, 511, 513, 8 * (1024 * 256 * 2 + 37) + 3]


@pytest.mark.parametrize("n", _sumsq_sizes())
def test_sumsq_sizes_and_accumulate(n, gen):
    g16 = vin(h16(n, scale=3.0, gen=gen))
    part = nan_ws(2048 * 4)
    out = vout(2)
    K.sumsq(g16.vec, n, out.vec, part)
    want = float(g16.vec.double().pow(2).sum())
    assert abs(float(out.vec[0]) - want) < 1e-4 * want and float(out.vec[1]) == 0.0         # test_fused_adam_and_norm: 1e-4 on the norm
    G.assert_untouched(out, written="logical", name="out2")
    # accumulate=True: three ranges (ragged cuts) accumulated == the sum of three plain calls; the flag is sticky (max) and reset by a plain call
    cuts = [0, (n // 3) // 8 * 8, (2 * n // 3) // 8 * 8, n] if n >= 24 else [0, 8]
    plain, acc = [], vout(2, init=torch.zeros(2, device=DEV))
    for i, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
        o = torch.zeros(2, device=DEV)
        K.sumsq(g16.vec[a:b], b - a, o, part)
        plain.append(o.clone())
        K.sumsq(g16.vec[a:b], b - a, acc.vec, part, accumulate=(i > 0))
    tot = plain[0][0]
    for o in plain[1:]:
        tot = tot + o[0]                                            # fp32 adds in launch order: the same chain as the kernel's out2[0] + tot
    assert float(acc.vec[0]) == float(tot) and float(acc.vec[1]) == 0.0
    G.assert_untouched(acc, written="logical", name="out2 (accumulated)")
    G.assert_untouched(g16, name="g16")
    if n >= 24:
        bad = g16.vec.clone()
        bad[cuts[1] + 3] = float("inf")                             # overflow in the SECOND range only
        bad = vin(bad)
        for i, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
            K.sumsq(bad.vec[a:b], b - a, acc.vec, part, accumulate=(i > 0))
        assert float(acc.vec[1]) == 1.0, "overflow flag must be sticky across accumulated ranges"
        K.sumsq(g16.vec[:cuts[1]], cuts[1], acc.vec, part)
        assert float(acc.vec[1]) == 0.0 and float(acc.vec[0]) == float(plain[0][0]), "a plain call resets sum and flag"


@pytest.mark.parametrize("n_kind", ["8", "504", "520", "past_cap"])
def test_fused_adam_sizes(n_kind, gen):
    """n of 8, one vector short of / past a 512-element wave run, and past the grid cap of 2 blocks per CU with a ragged remainder
    (every element compared); then the any_overflow input of vlp_adam_hyper: state bit-untouched."""
    n = {"8": 8, "504": 504, "520": 520, "past_cap": 8 * (2 * _cus() * 256 * 4 + 37)}[n_kind]
    p32, m, v = vout(n, init=torch.randn(n, device=DEV, generator=gen) * 0.02), vout(n, init=torch.rand(n, device=DEV, generator=gen) * 1e-3), \
        vout(n, init=torch.rand(n, device=DEV, generator=gen) * 1e-6)
    g16 = vin((torch.randn(n, device=DEV, generator=gen) * 300).half())
    p16 = vout(n, HALF)
    p0, m0, v0 = p32.vec.clone(), m.vec.clone(), v.vec.clone()
    out2, part, hyper = torch.zeros(2, device=DEV), nan_ws(2048 * 4), vout(3)
    sstate = torch.tensor([1024.0, 0, -1, 2, 1000, 1, 0, 0], device=DEV)
    K.sumsq(g16.vec, n, out2, part)
    K.adam_hyper(out2, None, sstate, 1.0, 3e-5, hyper.vec)
    G.assert_untouched(hyper, written="logical", name="hyper")
    hyper_in = vin(hyper.vec.clone())
    K.fused_adam(p32.vec, m.vec, v.vec, g16.vec, p16.vec, n, hyper_in.vec, decay=0.01)
    rp, rm, rv = _adam_ref(p0, m0, v0, g16.vec, float(hyper.vec[0]), 3e-5)
    # every element, fp32 arithmetic against fp64: test_fused_adam_and_norm's bounds
    assert rel(p32.vec, rp) < 1e-5 and rel(m.vec, rm) < 1e-4 and rel(v.vec, rv) < 1e-4
    assert float(((p32.vec.double() - rp).abs() / (rp.abs() + 1e-3)).max()) < 1e-4          # element-wise, not only against the tensor's scale
    assert torch.equal(p16.vec, p32.vec.half())
    G.assert_written(p16, "logical", "p16")
    for g, name in ((p32, "p32"), (m, "m"), (v, "v"), (p16, "p16")):
        G.assert_untouched(g, written="logical", name=name)
    G.assert_untouched(g16, name="g16")
    G.assert_untouched(hyper_in, name="hyper")
    # any_overflow set by another parameter group while this group's own sumsq2[1] == 0: skip
    for g in (p32, m, v, p16):
        g.seal()
    assert float(out2[1]) == 0.0
    K.adam_hyper(out2, torch.ones(1, device=DEV), sstate, 1.0, 3e-5, hyper.vec)
    assert float(hyper.vec[2]) == 1.0
    K.fused_adam(p32.vec, m.vec, v.vec, g16.vec, p16.vec, n, hyper.vec, decay=0.01)
    for g, name in ((p32, "p32"), (m, "m"), (v, "v"), (p16, "p16")):
        G.assert_untouched(g, name=name + " (skipped step)")


@pytest.mark.parametrize("g_is_f32", [True, False])
def test_bert_adam_segments_and_padded_tail(g_is_f32, gen):
    """Segments of 1, 2 and 3129 elements between ordinary ones, and a padded tail (n > seg_off[ntensors]) that belongs to no tensor: it
    must stay bit-untouched in p32 / m / v / p16."""
    sizes = [768, 1, 2, 3129, 4096 + 5, 8]
    offs = [0]
    for s in sizes:
        offs.append(offs[-1] + s)
    n = offs[-1] + 61                                               # padded tail
    seg = vin(torch.tensor(offs, dtype=I64, device=DEV), fill=offs[-1])       # guards: the start of the padded tail, which must stay bit-untouched
    p0 = torch.randn(n, device=DEV, generator=gen) * 0.02
    g = torch.randn(n, device=DEV, generator=gen) * 0.05
    g[offs[3]:offs[4]] *= 100                                       # one tensor far above the clip threshold
    gk = vin(g if g_is_f32 else g.half())
    p32, m, v, p16 = vout(n, init=p0), vout(n, init=torch.zeros(n, device=DEV)), vout(n, init=torch.zeros(n, device=DEV)), vout(n, HALF)
    norms = nan_ws(4 * K.bert_adam_norms_floats(n, len(sizes)))
    K.bert_adam(p32.vec, m.vec, v.vec, gk.vec, g_is_f32, p16.vec, seg.vec, len(sizes), n, norms, lr=1e-3, decay=0.01)
    rp, rm, rv = p0.cpu().clone(), torch.zeros(n), torch.zeros(n)
    for i in range(len(sizes)):
        sl = slice(offs[i], offs[i + 1])
        O.bert_adam_step(rp[sl], gk.vec.float().cpu()[sl], rm[sl], rv[sl], 0, lr=1e-3, weight_decay=0.01)
    live = offs[-1]
    assert rel(p32.vec[:live].cpu(), rp[:live]) < 1e-5 and rel(m.vec[:live].cpu(), rm[:live]) < 1e-4       # test_bert_adam
    assert rel(v.vec[:live].cpu(), rv[:live]) < 1e-4                                                          # as test_fused_adam_and_norm
    for i in range(len(sizes)):                                     # the tiny segments are not hidden behind the tensor-wide scale
        sl = slice(offs[i], offs[i + 1])
        assert rel(p32.vec[sl].cpu(), rp[sl]) < 1e-5, "segment %d" % i
        assert rel(m.vec[sl].cpu(), rm[sl]) < 1e-4, "segment %d" % i
        assert rel(v.vec[sl].cpu(), rv[sl]) < 1e-4, "segment %d" % i
    assert rel(p16.vec[:live].float().cpu(), p32.vec[:live].cpu()) < 1e-3
    foot = torch.zeros(n, dtype=torch.bool, device=DEV)
    foot[:live] = True
    for gd, name in ((p32, "p32"), (m, "m"), (v, "v"), (p16, "p16")):
        G.assert_untouched(gd, written=foot, name=name + " (padded tail)")
    G.assert_untouched(gk, name="g")
    G.assert_untouched(seg, name="seg_off")


def _gelu_grad64(z):
    z = z.double().requires_grad_(True)
    O.gelu(z).sum().backward()
    return z.grad


@pytest.mark.parametrize("n", [8, 8 * 12345, 8 * (4096 * 256 + 256 * 3 + 37)])
def test_gelu_bwd(n, gen):
    """dz = dy * gelu'(z) against autograd of O.gelu in fp64; bound as for MUL_GELU_GRAD in test_gemm_nt_epilogues (2e-3).  The last size is
    past the launcher's cap of 4096 blocks x 256 threads x 8 elements, with a remainder that is not a multiple of a block."""
    dy, z = vin(h16(n, gen=gen)), vin(h16(n, scale=1.5, gen=gen))
    dz = vout(n, HALF)
    K.gelu_bwd(dy.vec, z.vec, dz.vec, n)
    G.assert_written(dz, "logical", "dz")
    G.assert_finite(dz.vec, "dz")
    assert rel(dz.vec.float(), dy.vec.double() * _gelu_grad64(z.vec)) < 2e-3
    G.assert_untouched(dz, written="logical", name="dz")
    G.assert_untouched(dy, name="dy")
    G.assert_untouched(z, name="z")


def test_relu_dropout_bwd_past_grid_cap(gen):
    """6400 x 2048 (the step's region-feature shape): 1.6 M vectors against the launcher's cap of 4096 blocks x 256 threads, the grid wraps
    inside row 4096.  Every element, exact dropout mask through the mirror of the hash (in row chunks)."""
    rows, cols, p = 6400, 2048, 0.3
    y, dy = vin(torch.relu(h16(rows * cols, gen=gen))), vin(h16(rows * cols, gen=gen))
    dz = vout(rows * cols, HALF)
    K.relu_dropout_bwd(dy.vec, y.vec, dz.vec, rows * cols, cols, drop_p=p, seed=1, rng_stream=2)
    G.assert_written(dz, "logical", "dz")
    got, y2, dy2 = dz.vec.view(rows, cols), y.vec.view(rows, cols), dy.vec.view(rows, cols)
    for r0 in range(0, rows, 800):
        rr = range(r0, r0 + 800)
        ref = dy2[r0:r0 + 800].float() * (y2[r0:r0 + 800] > 0) * drop_mult_ref(p, 1, 2, rr, range(cols))
        assert rel(got[r0:r0 + 800].float(), ref) < 1e-3, "rows %d.." % r0          # test_vqa_mul_and_relu_dropout_bwd
        assert torch.equal(got[r0:r0 + 800] == 0, ref == 0), "rows %d..: keep / drop decisions differ" % r0
    G.assert_untouched(dz, written="logical", name="dz")
    G.assert_untouched(y, name="y")
    G.assert_untouched(dy, name="dy")


@pytest.mark.parametrize("rows,cs,cd,f32,beta", [(1501, 1607, 1663, True, 0), (50, 1664, 1607, False, 0), (50, 1607, 1607, False, 1), (3, 7, 16, True, 0)])
def test_copy2d_guarded(rows, cs, cd, f32, beta, gen):
    """cols_src < cols_dst (zero fill up to cols_dst), > (truncation), fp32 source, accumulation; 1501 x 1663 = 2 496 163 elements is past the
    launcher's cap of 8192 blocks x 256 elements, and the remainder (163 past 9750 blocks) is not a multiple of a block or of a 64-lane wave.
    Every element."""
    src = gin(torch.randn(rows, cs, device=DEV, generator=gen) if f32 else h16(rows, cs, gen=gen), pad=8)
    d0 = h16(rows, cd, gen=gen)
    dst = gout(rows, cd, pad=16, init=d0 if beta else None)
    K.copy2d(src.view, src.ld, f32, dst.view, dst.ld, rows, cs, cd, beta=beta)
    c = min(cs, cd)
    G.assert_written(dst, "logical", "dst")
    G.assert_finite(dst.view, "dst")
    if beta:
        assert rel(dst.view[:, :c].float(), d0[:, :c].float() + src.view[:, :c].float()) < 1e-3
    else:
        assert torch.equal(dst.view[:, :c], src.view[:, :c].half())
        G.assert_zero_band(dst, c, cd, "dst")                        # "columns >= cols_src are 0"
    G.assert_untouched(dst, written="logical", name="dst")
    G.assert_untouched(src, name="src")


# =====================================================================================================
# token-step kernels of the incremental decoder
# =====================================================================================================
@pytest.mark.parametrize("M,N,Kd,act", [(1, 28996, 768, 0), (5, 3129, 768, 2), (70, 1001, 128, 0), (1, 129, 64, 2), (5, 127, 768, 0), (70, 7, 64, 2), (5, 1, 128, 0)])
def test_dec_gemm_ragged(M, N, Kd, act, gen):
    n8 = roundup8(N)
    x, w, b = gin(h16(M, Kd, gen=gen)), gin(h16(N, Kd, scale=0.05, gen=gen), pad=16), vin(h16(N, gen=gen))
    y = gout(M, N, pad=24)
    K.dec_gemm(x.view, w.view, M, N, Kd, y=y.view, bias=b.vec, act=K.ACT_GELU if act else K.ACT_NONE)
    ref = x.view.float() @ w.view.float().t() + b.vec.float()
    if act:
        ref = torch.nn.functional.gelu(ref)
    G.assert_written(y, "logical", "Y")
    G.assert_finite(y.view, "Y")
    assert float((y.view.float() - ref).abs().max()) <= 2e-3 * max(1.0, float(ref.abs().max())) + 2e-3         # test_dec_gemm_plain_and_gelu
    G.assert_zero_band(y, N, n8, "Y")
    G.assert_untouched(y, written=n8, name="Y")
    for g, name in ((x, "X"), (w, "W"), (b, "bias")):
        G.assert_untouched(g, name=name)


def test_dec_gemm_kv_cache_and_ln_prologue_guarded(gen):
    """QKV form: K | V columns go to cache rows [start, start + T) of each sequence, every other cache row stays bit-untouched; with the
    LayerNorm prologue X holds pre-LayerNorm rows and ln_out receives the normalised ones."""
    R, T, H, Lcap, st = 3, 2, 256, 40, 17
    M = R * T
    pre = gin(h16(M, H, scale=2.0, gen=gen) + 0.5)
    w, b = gin(h16(3 * H, H, scale=0.05, gen=gen), pad=16), vin(h16(3 * H, gen=gen))
    ga, be = vin((1 + 0.1 * torch.randn(H, device=DEV, generator=gen)).half()), vin(h16(H, scale=0.1, gen=gen))
    y, xn = gout(M, 3 * H, pad=8), gout(M, H, pad=16)
    cache = G.guarded(R * Lcap, 2 * H, ld=2 * H, dtype=HALF, fill="sentinel", device=DEV)            # [R, Lcap, 2H] contiguous inside guards
    K.dec_gemm(pre.view, w.view, M, 3 * H, H, y=y.view, bias=b.vec, kv_cache=cache.view.view(R, Lcap, 2 * H), kv_col0=H, kv_Lcap=Lcap, kv_T=T, kv_start=st,
               ln_gamma=ga.vec, ln_beta=be.vec, ln_eps=1e-5, ln_out=xn.view)
    refn = torch.nn.functional.layer_norm(pre.view.float(), (H,), ga.vec.float(), be.vec.float(), 1e-5)
    check_out(xn, refn, 1.5e-3, "logical", "ln_out")
    ref = xn.view.float() @ w.view.float().t() + b.vec.float()                                       # the GEMM multiplies the rounded X'
    G.assert_finite(y.view[:, :H], "Y (q part)")
    assert rel(y.view[:, :H].float(), ref[:, :H]) < 1.5e-3
    rows = torch.zeros(R, Lcap, dtype=torch.bool, device=DEV)
    rows[:, st:st + T] = True
    got = cache.view.view(R, Lcap, 2 * H)[:, st:st + T].reshape(M, 2 * H)
    G.assert_finite(got, "K | V cache rows")
    assert rel(got.float(), ref[:, H:]) < 1.5e-3
    G.assert_untouched(cache, written=rows.view(-1, 1).expand(R * Lcap, 2 * H), name="kv_cache")      # rows outside [start, start + T): untouched
    G.assert_untouched(y, written="logical", name="Y")
    for g, name in ((pre, "X"), (w, "W"), (b, "bias"), (ga, "ln_gamma"), (be, "ln_beta")):
        G.assert_untouched(g, name=name)


@pytest.mark.parametrize("M,H,Kd,S", [(1, 768, 768, 4), (5, 256, 512, 2), (70, 1024, 512, 8), (5, 512, 3072, 4)])
def test_dec_split_reduce_ln_guarded(M, H, Kd, S, gen):
    x, w = gin(h16(M, Kd, gen=gen)), gin(h16(H, Kd, scale=0.03, gen=gen), pad=16)
    b, res = vin(h16(H, gen=gen)), gin(h16(M, H, gen=gen), pad=24)
    ga, be = vin((1 + 0.1 * torch.randn(H, device=DEV, generator=gen)).half()), vin(h16(H, scale=0.1, gen=gen))
    slab = torch.full((S, M, H + 8), float("nan"), device=DEV)                                        # ldslab > H
    y = gout(M, H, pad=16)
    K.dec_gemm(x.view, w.view, M, H, Kd, slab=slab, splits=S)
    K.dec_reduce_ln(slab, S, b.vec, res.view, ga.vec, be.vec, y.view, M, H, eps=1e-5)
    pre = (x.view.float() @ w.view.float().t() + b.vec.float() + res.view.float()).half().float()
    ref = torch.nn.functional.layer_norm(pre, (H,), ga.vec.float(), be.vec.float(), 1e-5)
    G.assert_written(y, "logical", "Y")
    G.assert_finite(y.view, "Y")
    err = (y.view.float() - ref).abs()
    assert float(err.max()) <= 6e-3 and float(err.mean()) <= 4e-4                                     # test_dec_split_gemm_plus_reduce_layernorm
    assert bool(torch.isnan(slab[:, :, H:]).all()), "slab padding columns were written"
    G.assert_untouched(y, written="logical", name="Y")
    for g, name in ((x, "X"), (w, "W"), (b, "bias"), (res, "residual"), (ga, "gamma"), (be, "beta")):
        G.assert_untouched(g, name=name)


@pytest.mark.parametrize("B,Lq,Lk,Lcap,heads,n_prefix", [(1, 2, 33, 64, 2, 0), (3, 1, 110, 122, 12, 0), (2, 64, 200, 256, 4, 0), (4, 2, 47, 64, 3, 20)])
def test_attn_decode_guarded(B, Lq, Lk, Lcap, heads, n_prefix, gen):
    """Cache rows >= Lk (stale positions) are NaN, as are the rows after the last sequence's cache; with a shared prefix the rows < n_prefix
    of the per-beam cache are NaN too (they must come from the prefix cache)."""
    H, beams = heads * 64, 2 if n_prefix else 1
    q = gin(h16(B * Lq, 3 * H, scale=0.8, gen=gen), pad=8)
    kv = h16(B, Lcap, 2 * H, scale=0.8, gen=gen)
    kv[:, Lk:] = float("nan")
    full = kv.clone()
    pref = None
    if n_prefix:
        pref = G.guarded((B // beams) * Lcap, 2 * H, ld=2 * H, dtype=HALF, fill="nan", device=DEV)
        pv = pref.view.view(B // beams, Lcap, 2 * H)
        pv[:, :n_prefix] = h16(B // beams, n_prefix, 2 * H, scale=0.8, gen=gen)
        pref.seal()
        full[:, :n_prefix] = pv[:, :n_prefix].repeat_interleave(beams, 0)
        kv[:, :n_prefix] = float("nan")
    cache = G.guarded(B * Lcap, 2 * H, ld=2 * H, dtype=HALF, fill="nan", device=DEV).set(kv.view(B * Lcap, 2 * H))
    cv = cache.view.view(B, Lcap, 2 * H)
    mask = (torch.rand(B, Lq, Lk, device=DEV, generator=gen) < 0.7).long()
    mask[:, :, 0] = 1
    Lkp = (Lk + 31) // 32 * 32
    mb = torch.empty(B, Lq, Lkp, dtype=torch.uint8, device=DEV)
    K.mask_pack_rect(mask, mb, B, Lq, Lk, Lkp)
    ctx = gout(B * Lq, H, pad=8)
    if n_prefix:
        K.attn_decode(q.view, q.ld, Lq, cv, cv[:, :, H:], 2 * H, Lcap, mb, ctx.view, B, Lq, Lk, heads, 0.125, k_prefix=pv, v_prefix=pv[:, :, H:],
                      prefix_rows=Lcap, n_prefix=n_prefix, beams=beams)
    else:
        K.attn_decode(q.view, q.ld, Lq, cv, cv[:, :, H:], 2 * H, Lcap, mb, ctx.view, B, Lq, Lk, heads, 0.125)
    qf = q.view[:, :H].float().view(B, Lq, heads, 64).transpose(1, 2)
    kf = full[:, :Lk, :H].float().view(B, Lk, heads, 64).transpose(1, 2)
    vf = full[:, :Lk, H:].float().view(B, Lk, heads, 64).transpose(1, 2)
    sc = qf @ kf.transpose(-1, -2) * 0.125 + (1.0 - mask[:, None].float()) * -10000.0
    ref = (torch.softmax(sc, dim=-1) @ vf).transpose(1, 2).reshape(B * Lq, H)
    G.assert_written(ctx, "logical", "ctx")
    G.assert_finite(ctx.view, "ctx")
    assert float((ctx.view.float() - ref).abs().max()) < 4e-3                                         # test_attn_decode_vs_torch
    G.assert_untouched(ctx, written="logical", name="ctx")
    G.assert_untouched(q, name="q")
    G.assert_untouched(cache, name="kv cache")
    if pref is not None:
        G.assert_untouched(pref, name="prefix cache")


def test_kv_append_and_gather_guarded(gen):
    B, T, H, Lcap, st = 3, 2, 128, 24, 21                    # the LAST positions of the cache: start + T == Lcap - 1
    qkv = gin(h16(B * T, 3 * H, gen=gen), pad=8)
    cache = G.guarded(B * Lcap, 2 * H, ld=2 * H, dtype=HALF, fill="sentinel", device=DEV)
    K.kv_append(qkv.view, qkv.ld, cache.view.view(B, Lcap, 2 * H), Lcap, B, T, st, H)
    rows = torch.zeros(B, Lcap, dtype=torch.bool, device=DEV)
    rows[:, st:st + T] = True
    assert torch.equal(cache.view.view(B, Lcap, 2 * H)[:, st:st + T].reshape(B * T, 2 * H), qkv.view[:, H:])
    G.assert_untouched(cache, written=rows.view(-1, 1).expand(B * Lcap, 2 * H), name="cache")
    G.assert_untouched(qkv, name="qkv_new")
    # kv_gather: dst[r, pos] = src[idx[r], pos] for pos in [lo, hi); rows with the first and the last valid index
    R, E, lo, hi = 4, 2 * H, 3, 9
    sv = h16(B * Lcap, E, gen=gen)
    sv.view(B, Lcap, E)[1] = float("nan")                     # sequence 1 is used by no real index: the guards of idx point at it
    src = G.guarded(B * Lcap, E, ld=E, dtype=HALF, fill="nan", device=DEV).set(sv)
    dst = G.guarded(R * Lcap, E, ld=E, dtype=HALF, fill="sentinel", device=DEV)
    idx = vin(torch.tensor([B - 1, 0, 0, B - 1], dtype=I64, device=DEV), fill=1)
    K.kv_gather(src.view, Lcap, dst.view, Lcap, idx.vec, R, lo, hi, E)
    want = src.view.view(B, Lcap, E)[idx.vec][:, lo:hi]
    G.assert_finite(want, "gathered rows (truth)")
    assert torch.equal(dst.view.view(R, Lcap, E)[:, lo:hi], want)
    rows = torch.zeros(R, Lcap, dtype=torch.bool, device=DEV)
    rows[:, lo:hi] = True
    G.assert_untouched(dst, written=rows.view(-1, 1).expand(R * Lcap, E), name="dst")
    G.assert_untouched(src, name="src")
    G.assert_untouched(idx, name="idx")


# =====================================================================================================
# data movement
# =====================================================================================================
def test_gather_scatter_pack_unpack_vqa_guarded(gen):
    """Row tables with NaN guard rows before row 0 and after the last row; positions include the first and the last valid index.  Position 5
    of every sample is a NaN row INSIDE the table that no real index uses: the guards of `pos` hold 5 and those of `row_map` hold row
    1 * L + 5 (sample 1 keeps one position only), so a stray read of an index guard is a valid access that poisons the result."""
    B, P, L, H, Nv = 4, 3, 20, 64, 10
    hv0 = h16(B * L, H, gen=gen)
    hv0.view(B, L, H)[:, 5] = float("nan")
    h = gin(hv0, pad=8)
    p = torch.randint(0, L, (B, P), device=DEV, generator=gen)
    p[p == 5] = 6
    p[0, 0], p[-1, -1] = 0, L - 1
    pos = vin(p.view(-1), fill=5)
    out = gout(B * P, H, pad=16)
    K.gather_rows(h.view, h.ld, pos.vec, out.view, out.ld, B, P, L, H)
    ref = torch.gather(h.view.reshape(B, L, H), 1, p.unsqueeze(2).expand(-1, -1, H)).reshape(B * P, H)
    G.assert_written(out, "logical", "out")
    G.assert_finite(out.view, "out")
    assert torch.equal(out.view, ref)
    G.assert_untouched(out, written="logical", name="out")
    G.assert_untouched(h, name="src")
    dh = gout(B * L, H, pad=8, init=torch.zeros(B * L, H, device=DEV, dtype=HALF))
    src = gin(out.view.contiguous(), pad=24)
    K.scatter_add_rows(src.view, src.ld, pos.vec, dh.view, dh.ld, B, P, L, H)
    ref_d = torch.zeros(B, L, H, device=DEV).scatter_add_(1, p.unsqueeze(2).expand(-1, -1, H), src.view.reshape(B, P, H).float())
    G.assert_finite(dh.view, "dst")
    assert rel(dh.view.float(), ref_d.view(B * L, H)) < 2e-3                                          # test_copy2d_transpose_gather_scatter
    G.assert_untouched(dh, written="logical", name="dst")
    G.assert_untouched(src, name="src")
    G.assert_untouched(pos, name="pos")
    # packed rows
    lens = [20, 1, 13, 20]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    Mp = int(off[-1])
    row_off = vin(torch.from_numpy(off).to(DEV), fill=Mp)          # guards: the end offset (an empty sample past the last one)
    row_map = vout(Mp, I32)
    K.rowmap_build(row_off.vec, B, L, row_map.vec)
    want = torch.from_numpy(np.concatenate([b * L + np.arange(n) for b, n in enumerate(lens)]).astype(np.int32)).to(DEV)
    assert torch.equal(row_map.vec, want)
    G.assert_untouched(row_map, written="logical", name="row_map")
    rm = vin(want, fill=1 * L + 5)
    assert not bool((want == 1 * L + 5).any())
    packed = gout(Mp, H, pad=16)
    K.rows_pack(h.view, rm.vec, Mp, packed.view, H)
    assert torch.equal(G.bits(packed.view), G.bits(h.view[want.long()]))                              # bit patterns: the kept position-5 rows are NaN
    G.assert_untouched(packed, written="logical", name="packed")
    back = gout(B * L, H, pad=24)
    K.rows_unpack(packed.view, rm.vec, Mp, back.view, H)
    keep = torch.zeros(B * L, dtype=torch.bool, device=DEV)
    keep[want.long()] = True
    assert torch.equal(G.bits(back.view[keep]), G.bits(h.view[keep]))
    G.assert_untouched(back, written=keep[:, None].expand(B * L, H), name="unpacked")                  # rows no packed row maps to: not touched
    G.assert_untouched(h, name="src")
    G.assert_untouched(rm, name="row_map")
    # VQA fusion reads rows 0 and Nv + 1 of every sample (h is contiguous [B*L, H] by definition of the entry point)
    hc = G.guarded(B * L, H, ld=H, dtype=HALF, fill="nan", device=DEV).set(h.view)
    e = gout(B, H, pad=0) if H % 8 else G.guarded(B, H, ld=H, dtype=HALF, fill="sentinel", device=DEV)
    K.vqa_mul_fwd(hc.view, e.view, B, L, Nv, H)
    hv = hc.view.float().view(B, L, H)
    G.assert_finite(e.view, "vqa out")
    assert rel(e.view.float(), hv[:, 0] * hv[:, Nv + 1]) < 1e-3
    G.assert_untouched(e, written="logical", name="vqa out")
    dout = G.guarded(B, H, ld=H, dtype=HALF, fill="nan", device=DEV).set(h16(B, H, gen=gen))
    dhc = G.guarded(B * L, H, ld=H, dtype=HALF, fill="sentinel", device=DEV).set(torch.zeros(B * L, H, device=DEV, dtype=HALF))
    K.vqa_mul_bwd(hc.view, dout.view, dhc.view, B, L, Nv, H)
    d = dhc.view.float().view(B, L, H)
    assert rel(d[:, 0], dout.view.float() * hv[:, Nv + 1]) < 1e-3 and rel(d[:, Nv + 1], dout.view.float() * hv[:, 0]) < 1e-3
    G.assert_untouched(dhc, written="logical", name="dh")
    G.assert_untouched(hc, name="h")
    G.assert_untouched(dout, name="dout")


@pytest.mark.parametrize("rows,cols", [(300, 200), (1, 7), (63, 65), (5, 3129)])
def test_transpose_guarded(rows, cols, gen):
    rp = (rows + 63) // 64 * 64
    w = gin(h16(rows, cols, gen=gen), pad=8)
    wt = gout(cols, rp, pad=16)
    K.transpose(w.view, w.ld, wt.view, wt.ld, rows, cols, rp)
    assert torch.equal(wt.view[:, :rows], w.view.t())
    G.assert_zero_band(wt, rows, rp, "dst")                       # zero up to rows_pad, nothing beyond it (include/vlp_hip.h)
    G.assert_untouched(wt, written=rp, name="dst")
    G.assert_untouched(w, name="src")
    wb = gout(cols, rp, pad=16)
    K.transpose_batched(K.make_transpose_batch([(w.view, w.ld, wb.view, wb.ld, rows, cols, rp)], DEV))
    assert torch.equal(wb.view[:, :rows], w.view.t())
    G.assert_zero_band(wb, rows, rp, "dst (batched)")
    G.assert_untouched(wb, written=rp, name="dst (batched)")
    G.assert_untouched(w, name="src")


@pytest.mark.parametrize("B,L,Nv", [(3, 43, 8), (1, 30, 0)])
def test_embed_fwd_bwd_guarded(B, L, Nv, gen):
    """Embedding tables with NaN guard rows before row 0 and after the last row, and one NaN row INSIDE each table (word row 7, type row T - 1)
    that no id uses: the guards of input_ids / segment_ids hold exactly those indices, so a stray read of an id guard is a valid access that
    poisons the result.  Ids include the first and the last valid row; Nv = 0 runs without region rows."""
    H, V, T, P = 768, 500, 6, 64
    ids = torch.randint(0, V, (B, L), device=DEV, generator=gen)
    ids[ids == 7] = 8
    ids[0, -1], ids[-1, -2] = 0, V - 1
    seg = torch.randint(0, T - 1, (B, L), device=DEV, generator=gen)
    ids_g, seg_g = vin(ids.view(-1), fill=7), vin(seg.view(-1), fill=T - 1)
    tab = {}
    for name, rows, poison in (("word", V, 7), ("pos", P, None), ("type", T, T - 1)):
        t = h16(rows, H, gen=gen)
        if poison is not None:
            t[poison] = float("nan")
        tab[name] = G.guarded(rows, H, ld=H, dtype=HALF, fill="nan", device=DEV).set(t)
    n_vis = max(B * Nv, 1)
    vis = G.guarded(n_vis, H, ld=H, dtype=HALF, fill="nan", device=DEV).set(torch.relu(h16(n_vis, H, gen=gen)))
    vpe = G.guarded(n_vis, H, ld=H, dtype=HALF, fill="nan", device=DEV).set(torch.relu(h16(n_vis, H, gen=gen)))
    pre = G.guarded(B * L, H, ld=H, dtype=HALF, fill="sentinel", device=DEV)
    K.embed_fwd(ids_g.vec.view(B, L), seg_g.vec.view(B, L), tab["word"].view, tab["pos"].view, tab["type"].view, vis.view if Nv else None,
                vpe.view if Nv else None, pre.view, B, L, Nv, H)
    w64, p64, t64 = (tab[k].view.double().nan_to_num(0.0).requires_grad_(True) for k in ("word", "pos", "type"))
    v64, e64 = vis.view.double().requires_grad_(True), vpe.view.double().requires_grad_(True)
    word = w64[ids]
    posr = p64[torch.arange(L, device=DEV)][None].expand(B, L, H)
    if Nv:
        word = torch.cat([word[:, :1], v64.view(B, Nv, H), word[:, Nv + 1:]], 1)
        posr = torch.cat([posr[:, :1], e64.view(B, Nv, H), posr[:, Nv + 1:]], 1)
    ref = word + posr + t64[seg]
    check_out(pre, ref.reshape(B * L, H), 1e-3, "logical", "pre")                                     # test_embed_fwd_bwd
    for g, name in ((ids_g, "input_ids"), (seg_g, "segment_ids"), (vis, "vis_h"), (vpe, "vispe_h")) + tuple((tab[k], k) for k in tab):
        G.assert_untouched(g, name=name)
    # backward: += into the three tables (zero before), region-row gradients out
    dpre = G.guarded(B * L, H, ld=H, dtype=HALF, fill="nan", device=DEV).set(h16(B * L, H, gen=gen))
    dw, dp_, dt = (G.guarded(r, H, ld=H, dtype=HALF, fill="sentinel", device=DEV).set(torch.zeros(r, H, device=DEV, dtype=HALF)) for r in (V, P, T))
    dv, dvp = (G.guarded(n_vis, H, ld=H, dtype=HALF, fill="sentinel", device=DEV) for _ in range(2))
    acc = nan_ws(4 * K.embed_bwd_workspace_floats(B, L, Nv, H))
    K.embed_bwd(dpre.view, ids_g.vec.view(B, L), seg_g.vec.view(B, L), vis.view if Nv else None, vpe.view if Nv else None, dw.view, dp_.view, dt.view,
                dv.view if Nv else None, dvp.view if Nv else None, acc, B, L, Nv, H, V, T)
    ref.backward(dpre.view.double().view(B, L, H))
    for g, want, name in ((dw, w64.grad, "d_word_emb"), (dp_, p64.grad, "d_pos_emb"), (dt, t64.grad, "d_type_emb")):
        check_out(g, want, 3e-3, "logical", name)                                                    # test_embed_fwd_bwd
    if Nv:
        check_out(dv, v64.grad * (v64.detach() > 0), 1e-3, "logical", "d_vis_h")
        check_out(dvp, e64.grad * (e64.detach() > 0), 1e-3, "logical", "d_vispe_h")
    else:
        G.assert_untouched(dv, name="d_vis_h (Nv = 0)")
        G.assert_untouched(dvp, name="d_vispe_h (Nv = 0)")
    for g, name in ((dpre, "dpre"), (ids_g, "input_ids"), (seg_g, "segment_ids"), (vis, "vis_h"), (vpe, "vispe_h")):
        G.assert_untouched(g, name=name)
