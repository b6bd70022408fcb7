"""GPU contract tests of the kernels the padding-free training step runs and tests/test_05_kernel_contract_gpu.py does not reach.

The packed step runs every encoder GEMM at a row count M' = sum of the kept lengths, a different value each step (7 000 .. 10 688 at
B = 64).  test_05's N list holds no multiple of 128 and no multiple of 16, so it never launches the persistent k-stream kernel
(gemm_nt_ps.hip: the QKV forward of every packed step with M' >= 6144) nor the lean multiplier instantiation of the 256x256 ring (the
FFN-down dgrad of every step), and the pretext / region-mask / mask-build / box-encoding kernels were only ever run at the workload's own
shapes on exact-size buffers.  Same method as test_05, same helpers: every operand from tests/guard_util.py (leading dimensions larger
than the width where the entry point has one, NaN in every byte a kernel must not read, a sentinel in every byte of an output), and per call
  (a) the result against an fp32 / fp64 torch restatement with the bound test_00 / test_50 use for that op,
  (b) the promised zero band,
  (c) every byte outside the write footprint, and every input, bit-untouched,
  (d) a finite result although everything around the operands is NaN.
Each test prints the largest error it saw ("[err] ..."; run with -s); nothing is asserted on those lines.
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from vlp_amd import _lib as K          # noqa: E402
from oracle import loader_oracle as LO  # noqa: E402   (checker only)
from oracle import vlp_oracle as O      # noqa: E402   (checker only)

from tests import guard_util as G                                              # noqa: E402
from tests.guard_util import roundup8                                          # noqa: E402
from tests.hard_inputs import pretext_sim_window                               # noqa: E402
from tests.kernel_util import DEV, drop_mult_ref, h16, rel                     # noqa: E402
from tests.test_05_kernel_contract_gpu import check_out, gin, gout, vin, vout  # noqa: E402

HALF, F32, I64, I32, U8 = torch.float16, torch.float32, torch.int64, torch.int32, torch.uint8


@pytest.fixture
def gen():
    g = torch.Generator(device=DEV)
    g.manual_seed(8765)
    return g


def flat(rows, cols, dtype=HALF, fill="nan"):
    """Guarded [rows, cols] tensor for the entry points that take no leading dimension (ld = cols): guard rows only."""
    return G.guarded(rows, cols, ld=cols, dtype=dtype, fill=fill, device=DEV)


def note(what, value):
    print("[err] %s: %.3e" % (what, value))


def cdiv(a, b):
    return (a + b - 1) // b


def gelu_grad64(z):
    z = z.double().requires_grad_(True)
    O.gelu(z).sum().backward()
    return z.grad


# =====================================================================================================
# A. persistent k-stream GEMM (gemm_nt_ps.hip, variants 256 / 264) under guards
# =====================================================================================================
# (M, N, K, VLP_NT_PS_GRID, epilogue, alpha, tiles per run).  The kernel walks 256 x 128 tiles, n fastest; the launcher gives every
# workgroup per = cdiv(tiles, cap) consecutive tiles and launches cdiv(tiles, per) workgroups (gemm_nt_ps.hip, vlp_gemm_nt_ps_launch), so
# the last column is a function of the others and is asserted, not assumed.  What the list covers:
#   epilogues       bias, plain (no bias), save-grad GeLU (Y and preact), MUL_PLAIN; alpha = 0.5 once
#   N               128, 256, 384, 640;   K / 64 = 9 (the smallest eligible K) and K = 768
#   last row tile   1 row (M = 1, M = 257), 255 rows (M = 255, 511), a cut inside a 64-row wave tile and a 16-row block (M = 321: 65 rows,
#                   M = 575: 63 rows, M = 833: 65 rows)
#   runs            1 tile, 2 tiles, >= 3 tiles; ragged last run (4, 4, 2); a run that crosses from one X row panel to the next (M = 257,
#                   N = 384, one workgroup: tiles 0..2 of panel 0, then 3..5 of panel 1; also the 4, 4, 2 and 3 x 5 cases)
#   +8 remap (264)  grids of 5, 9 and 10 workgroups (gridDim % 8 != 0 below and above 8), and 1, 2, 3
PS_CASES = [
    (1, 128, 576, 1, "bias", 1.0, (1,)),
    (257, 384, 768, 1, "sg", 1.0, (6,)),
    (255, 256, 576, 2, "plain", 1.0, (1, 1)),
    (321, 640, 768, 3, "mul", 1.0, (4, 4, 2)),
    (575, 640, 576, 5, "bias", 0.5, (3, 3, 3, 3, 3)),
    (575, 384, 768, 9, "sg", 1.0, (1,) * 9),
    (511, 256, 576, 2, "mul", 1.0, (2, 2)),
    (257, 128, 768, 100, "plain", 1.0, (1, 1)),
    (833, 640, 576, 11, "mul", 1.0, (2,) * 10),
]


def _ps_run(variant, M, N, Kd, epi, alpha, x, w, bias, src):
    """One vlp_gemm_nt call into fresh guarded outputs; ldy = N + 24, ldp = N + 40, ldm = N + 16 (all different)."""
    y = gout(M, N, pad=24)
    pre = gout(M, N, pad=40) if epi == "sg" else None
    kw = dict(variant=variant, alpha=alpha)
    if epi in ("bias", "sg"):
        kw["bias"] = bias.vec
    if epi == "sg":
        kw.update(preact=pre.view, act=K.ACT_GELU_SAVE_GRAD)
    if epi == "mul":
        kw.update(mul_src=src.view, mul_mode=K.MUL_PLAIN)
    K.gemm_nt(x.view, w.view, y.view, M, N, Kd, **kw)
    return y, pre, K.gemm_nt_resolved_variant()


@pytest.mark.parametrize("M,N,Kd,cap,epi,alpha,runs", PS_CASES)
def test_gemm_nt_persistent_guarded(M, N, Kd, cap, epi, alpha, runs, gen, monkeypatch):
    """The kernel defers a tile's stores behind the next tile's k loop, clamps its X rows at M - 1 and requests a tile's multiplier rows
    during that tile's last k tile: a store or an unclamped load past M lands in the guard rows here.  Per case and variant: the launcher
    ran the variant it was asked for (no silent fallback), (a)..(d) against the fp64 product, the bits of the ring (27 / 29) run under the
    same guards, and three launches that agree bit for bit, guards included."""
    tiles = cdiv(M, 256) * (N // 128)
    per = cdiv(tiles, cap)
    grid = cdiv(tiles, per)
    assert tuple(min(per, tiles - i * per) for i in range(grid)) == runs, "the case list describes another run structure"
    assert N % 128 == 0 and Kd // 64 > 8                            # vlp_gemm_nt_ps_eligible
    monkeypatch.setenv("VLP_NT_PS_GRID", str(cap))
    x, w = gin(h16(M, Kd, gen=gen), pad=8), gin(h16(N, Kd, scale=0.05, gen=gen), pad=16)
    bias, src = vin(h16(N, scale=0.5, gen=gen)), gin(h16(M, N, gen=gen), pad=16)
    lin = alpha * (x.view.double() @ w.view.double().t())
    want_pre = None
    if epi == "bias":
        want = lin + bias.vec.double()
    elif epi == "plain":
        want = lin
    elif epi == "mul":
        want = lin * src.view.double()
    else:
        # the stored derivative and Y are gelu'(z16) / gelu(z16) of the fp16-rounded pre-activation, which this call does not output: z16
        # comes from an ACT_GELU call on the ring (the same chain, the same rounding), as in test_05 / test_gemm_nt_epilogues
        z16 = torch.empty(M, N, device=DEV, dtype=HALF)
        K.gemm_nt(x.view, w.view, torch.empty(M, N, device=DEV, dtype=HALF), M, N, Kd, bias=bias.vec, preact=z16, act=K.ACT_GELU, variant=27)
        e = rel(z16.float(), lin + bias.vec.double())
        note("ps z16 vs fp64 (M=%d N=%d K=%d)" % (M, N, Kd), e)
        assert e < 1.5e-3
        want, want_pre = O.gelu(z16.double()), gelu_grad64(z16)
    ring = 29 if N > 1024 else 27
    y_ring, pre_ring, rv = _ps_run(ring, M, N, Kd, epi, alpha, x, w, bias, src)
    assert rv == ring
    check_out(y_ring, want, 1.5e-3, "logical", "Y (ring)")
    worst = 0.0
    for variant in (256, 264):
        first = None
        for it in range(3):
            y, pre, rv = _ps_run(variant, M, N, Kd, epi, alpha, x, w, bias, src)
            assert rv == variant, "variant %d fell back to %d" % (variant, rv)
            tag = "variant %d run %d" % (variant, it)
            check_out(y, want, 1.5e-3, "logical", "Y, " + tag)       # fp32 accumulate, one fp16 rounding of the result (test_00)
            worst = max(worst, rel(y.view.float(), want))
            assert torch.equal(G.bits(y.view), G.bits(y_ring.view)), "Y differs from the ring, " + tag
            if pre is not None:
                check_out(pre, want_pre, 1.5e-3, "logical", "preact(gelu'), " + tag)
                worst = max(worst, rel(pre.view.float(), want_pre))
                assert torch.equal(G.bits(pre.view), G.bits(pre_ring.view)), "stored derivative differs from the ring, " + tag
            if first is None:
                first = (y, pre)
            else:
                assert torch.equal(G.bits(y.buf), G.bits(first[0].buf)), "Y: run 0 and " + tag + " differ"
                assert pre is None or torch.equal(G.bits(pre.buf), G.bits(first[1].buf)), "preact: run 0 and " + tag + " differ"
    note("ps %s M=%d N=%d K=%d cap=%d" % (epi, M, N, Kd, cap), worst)
    for g, name in ((x, "X"), (w, "W"), (bias, "bias"), (src, "mul_src")):
        G.assert_untouched(g, name=name)


# =====================================================================================================
# B. lean multiplier epilogue of the 256 x 256 ring under guards
# =====================================================================================================
# The launcher does not report which instantiation of variants 21 / 29 ran.  gemm_nt.hip (vlp_gemm_nt, case 5) picks
# gemm_nt_kernel<3, 256, 256, false, 2, 1> -- the lean epilogue: multiplier rows loaded as two 8-wide vectors per row block, clamped at
# M - 1, no shared epilogue -- exactly when
#     (variant & 7) == 5 && (variant & 16),  mul_mode == VLP_MUL_PLAIN,  N % 16 == 0,
#     no activation, no preact, no residual, no dropout (a bias is allowed),  ldm % 8 == 0 and mul_src 16-byte aligned (the ABI's own rule),
#     and the process did not hold VLP_NT_LEAN_EPI=0 at its first variant-21 / 29 launch.
# Every case below meets it.  A change of that condition in gemm_nt.hip has to be mirrored here, or these cases silently test the shared
# epilogue a second time.  VLP_NT_LEAN_EPI is read ONCE per process into a function-local static (gemm_nt.hip), so no test can switch it:
# what the environment held when this module was imported is what decides, and with "0" there the cases fail instead of passing on the
# shared epilogue.
# (variant, M, N, K): N in {16, 272, 768} x M in {1, 255, 257, 575}; either variant and either K at every N and at every M
LEAN_CASES = [
    (29, 1, 16, 64), (21, 255, 16, 64), (29, 257, 16, 768), (21, 575, 16, 768),
    (21, 1, 272, 768), (29, 255, 272, 768), (21, 257, 272, 64), (29, 575, 272, 64),
    (29, 1, 768, 64), (21, 255, 768, 64), (29, 257, 768, 768), (21, 575, 768, 768),
]
LEAN_ENV_AT_IMPORT = os.environ.get("VLP_NT_LEAN_EPI")


@pytest.mark.parametrize("variant,M,N,Kd", LEAN_CASES)
def test_gemm_nt_lean_multiplier_guarded(variant, M, N, Kd, gen):
    assert not (LEAN_ENV_AT_IMPORT or "").startswith("0"), "VLP_NT_LEAN_EPI=0: the launcher runs the shared epilogue, the lean one is not under test"
    assert (variant & 7) == 5 and (variant & 16) and N % 16 == 0
    x, w = gin(h16(M, Kd, gen=gen), pad=8), gin(h16(N, Kd, scale=0.05, gen=gen), pad=16)
    src = gin(h16(M, N, gen=gen), pad=16)
    want = (x.view.double() @ w.view.double().t()) * src.view.double()

    def run(v):
        y = gout(M, N, pad=24)
        K.gemm_nt(x.view, w.view, y.view, M, N, Kd, mul_src=src.view, mul_mode=K.MUL_PLAIN, variant=v)
        assert K.gemm_nt_resolved_variant() == v
        check_out(y, want, 1.5e-3, "logical", "Y (variant %d)" % v)                  # test_gemm_nt_epilogues' MUL_PLAIN bound
        return y

    y = run(variant)
    y27 = run(27)                                                    # 256 x 128 ring: the shared epilogue (nt_epilogue8)
    assert torch.equal(G.bits(y.view), G.bits(y27.view)), "lean epilogue and shared epilogue differ"
    note("lean v=%d M=%d N=%d K=%d" % (variant, M, N, Kd), rel(y.view.float(), want))
    for g, name in ((x, "X"), (w, "W"), (src, "mul_src")):
        G.assert_untouched(g, name=name)


# =====================================================================================================
# C. what the dispatcher picks at packed row counts
# =====================================================================================================
# (call site, N, K, epilogue as vlp_amd/engine.py passes it there, resolved variants the contract tests cover for that site).
#   264       test_gemm_nt_persistent_guarded above (bias epilogue)
#   29 / 77   test_05::test_gemm_nt_ragged runs both kernels under guards with each of these epilogues (bias, residual, dropout,
#             save-grad, MUL_PLAIN) -- at ragged N only (no multiple of 8 among them) and never with row_map; 29 + MUL_PLAIN at
#             N % 16 == 0 is in test_gemm_nt_lean_multiplier_guarded above
# "Covered" therefore means: this kernel, this epilogue, inside guard bands, somewhere.  The combinations of the forward sites
# themselves -- 77 + bias + residual + dropout + row_map at N = 768, 29 + save-grad at N = 3072 -- run only here, on exact-size buffers.
# A change of vlp_amd/tuned_gfx950.json or tuning.nt_heuristic that moves a site onto another kernel fails here, not in training.
DISPATCH_SITES = [
    ("qkv fwd", 2304, 768, "bias", {264, 29}),
    ("attention output fwd", 768, 768, "bias_res_drop", {77}),
    ("ffn up fwd", 3072, 768, "save_grad", {29}),
    ("ffn down fwd", 768, 3072, "bias_res_drop", {77}),
    ("ffn down dgrad", 3072, 768, "mul_plain", {29}),
    ("ffn up dgrad", 768, 3072, "residual", {77}),
    ("attention output dgrad", 768, 768, "plain", {77}),
    ("qkv dgrad", 768, 2304, "residual", {77}),
]


@pytest.mark.parametrize("Mp", [6144, 7937, 8311, 10687])
def test_gemm_nt_packed_dispatch(Mp, gen, monkeypatch):
    """tuning.nt_variant(M', N, K) for every encoder GEMM of a packed step, run with the epilogue of its call site: the launcher ran a
    variant of the covered set, the bits are the ring's, and the first 256 and the last 257 rows (the ragged last row tile) agree with
    the fp64 product (1.5e-3, test_00); every element is finite (the outputs start as NaN)."""
    from vlp_amd import tuning
    for name in ("VLP_NT_VARIANT", "VLP_NT_RULES", "VLP_NT_OVERRIDE", "VLP_NT_PS_GRID"):
        monkeypatch.delenv(name, raising=False)
    p, seed = 0.1, 41
    xs = {Kd: h16(Mp, Kd, gen=gen) for Kd in (768, 2304, 3072)}
    ar = torch.arange(Mp, device=DEV)
    row_map = (ar + 3 * (ar // 97)).to(I32)                          # packed row -> dense row: increasing, with gaps
    sub = torch.cat([ar[:256], ar[Mp - 257:]])
    picked = []
    for site, (name, N, Kd, epi, covered) in enumerate(DISPATCH_SITES):
        x = xs[Kd]
        w, bias = h16(N, Kd, scale=0.05, gen=gen), h16(N, gen=gen)
        res = h16(Mp, N, gen=gen) if epi in ("bias_res_drop", "residual") else None
        src = h16(Mp, N, gen=gen) if epi == "mul_plain" else None
        kw = {}
        if epi in ("bias", "bias_res_drop", "save_grad"):
            kw["bias"] = bias
        if epi == "bias_res_drop":
            kw.update(residual=res, dropout_p=p, seed=seed, rng_stream=16 * site + 2, row_map=row_map)
        if epi == "residual":
            kw["residual"] = res
        if epi == "mul_plain":
            kw.update(mul_src=src, mul_mode=K.MUL_PLAIN)

        def run(v):
            y = torch.full((Mp, N), float("nan"), device=DEV, dtype=HALF)
            pre = torch.full((Mp, N), float("nan"), device=DEV, dtype=HALF) if epi == "save_grad" else None
            if pre is not None:
                K.gemm_nt(x, w, y, Mp, N, Kd, preact=pre, act=K.ACT_GELU_SAVE_GRAD, variant=v, **kw)
            else:
                K.gemm_nt(x, w, y, Mp, N, Kd, variant=v, **kw)
            return y, pre, K.gemm_nt_resolved_variant()

        v = tuning.nt_variant(Mp, N, Kd)
        y, pre, resolved = run(v)
        picked.append(resolved)
        assert resolved in covered, "%s at M' = %d: nt_variant gave %d, the launcher ran %d; the contract tests cover %s there" % (
            name, Mp, v, resolved, sorted(covered))
        ring = 29 if N > 1024 else 27
        y2, pre2, rv = run(ring)
        assert rv == ring
        assert bool(torch.isfinite(y).all()), name
        assert torch.equal(G.bits(y), G.bits(y2)), "%s at M' = %d: variant %d differs from ring %d" % (name, Mp, resolved, ring)
        lin = x[sub].double() @ w.double().t()
        if epi == "save_grad":
            assert bool(torch.isfinite(pre).all()), name
            assert torch.equal(G.bits(pre), G.bits(pre2)), "%s at M' = %d: stored derivative differs from the ring" % (name, Mp)
            z16 = torch.empty(Mp, N, device=DEV, dtype=HALF)
            K.gemm_nt(x, w, torch.empty(Mp, N, device=DEV, dtype=HALF), Mp, N, Kd, bias=bias, preact=z16, act=K.ACT_GELU, variant=ring)
            z = z16[sub]
            assert rel(z.float(), lin + bias.double()) < 1.5e-3, name
            e = max(rel(y[sub].float(), O.gelu(z.double())), rel(pre[sub].float(), gelu_grad64(z)))
        else:
            if epi == "bias":
                want = lin + bias.double()
            elif epi == "bias_res_drop":
                mult = drop_mult_ref(p, seed, 16 * site + 2, row_map[sub].long(), range(N)).double()
                want = (lin + bias.double()) * mult + res[sub].double()
            elif epi == "residual":
                want = lin + res[sub].double()
            elif epi == "mul_plain":
                want = lin * src[sub].double()
            else:
                want = lin
            e = rel(y[sub].float(), want)
        note("dispatch %s M'=%d variant %d" % (name, Mp, resolved), e)
        assert e < 1.5e-3, "%s at M' = %d (variant %d): rel err %.3e" % (name, Mp, resolved, e)
    print("[dispatch] M' = %d: %s" % (Mp, picked))


# =====================================================================================================
# D. pretext loss, region mask, mask build, box encoding
# =====================================================================================================
def _masked_positions(B, Nv, Pm, spare):
    """[B, Pm] distinct positions in 1..Nv (include/vlp_hip.h), never `spare`; sample 0 holds the last position and, from Pm = 2 on, the
    first usable one."""
    cand = [q for q in range(1, Nv + 1) if q != spare]
    assert len(cand) >= Pm
    out = []
    for b in range(B):
        if b == 0 and Pm >= 1:
            inner = cand[1:-1]
            perm = torch.randperm(len(inner), generator=torch.Generator().manual_seed(100)).tolist()
            row = [cand[-1]] + [inner[i] for i in perm[:max(Pm - 2, 0)]] + ([cand[0]] if Pm >= 2 else [])
        else:
            perm = torch.randperm(len(cand), generator=torch.Generator().manual_seed(100 + b)).tolist()
            row = [cand[i] for i in perm[:Pm]]
        assert len(row) == Pm and len(set(row)) == Pm
        out.append(row)
    return torch.tensor(out, dtype=I64, device=DEV).view(B, Pm)


# Pm = 64 with Nv = 64 masks every region; H = 520 gives 65 eight-column chunks, one past the 64-lane stride of the forward
@pytest.mark.parametrize("B,Nv,Pm,H,p", [(1, 3, 1, 64, 0.0), (3, 3, 1, 768, 0.1), (3, 4, 2, 520, 0.0), (1, 20, 5, 768, 0.1), (3, 20, 5, 64, 0.0),
                                          (1, 65, 63, 520, 0.1), (3, 65, 63, 768, 0.0), (1, 64, 64, 768, 0.1), (3, 64, 64, 520, 0.0)])
def test_pretext_guarded(B, Nv, Pm, H, p, gen):
    """vlp_pretext_fwd / vlp_pretext_bwd with the references and bounds of test_00::test_pretext_fwd_bwd.  vis_masked_pos is a guarded int64
    input whose guards hold a valid position (2) that no sample masks and whose region row is NaN in vis_h and vispe_h (where every region
    is masked there is no such row: the guards then hold position 1, a stray read stays in bounds and shows in the numbers only).

    The rounding-flip allowance, restated per shape from the reference's own similarity matrix: the kernel sums each H-long dot product in
    fp32 -- 8 ceil(H / 512) fused multiply-adds per lane and a 6-level wave reduction, that many roundings of 2^-24 against
    sum |a_k v_k| at the most (tests/hard_inputs.py::pretext_sim_window; tests/test_hard_inputs_cpu.py shows on the CPU that the kernel's
    summation order never flips an entry outside that window and that the window holds a few percent of the entries) -- and rounds the
    sum to fp16.  An entry whose fp64 value lies that close to an fp16 rounding boundary may round either way
    (one fp16 ulp of that entry, which moves the softmax row it belongs to); every other entry cannot.  At Pm = 63 / 64 most ROWS hold such
    an entry (a few percent of the entries, 40 .. 90 % of the rows: tests/test_hard_inputs_cpu.py), so the window alone would exempt
    most of `probs`; the number of rows that actually moved is bounded as well.  Rules: every entry within test_00's 1.2 ulp + 1e-6; a
    row off by more than 1e-6 must hold an entry inside the window; at most min(entries inside the window, 4) rows are off by more than
    1e-6, the same cap of four flips as the loss term (test_00's 4 ulp / (B Pm), one ulp / (B Pm) per entry inside the window, never
    more than four); and test_00's "fewer than 2 % of the entries off by more than 1e-6" wherever one flipped row fits inside 2 %
    (B Pm > 50).  At Pm = 1 everything is exact: probs 1, loss 0, +0 gradients."""
    seed, s_vis, s_vpe = 77, 1001, 1002
    rows, cols = list(range(B * Nv)), list(range(H))
    mv, mp = drop_mult_ref(p, seed, s_vis, rows, cols), drop_mult_ref(p, seed, s_vpe, rows, cols)
    vis0 = (torch.relu(h16(B * Nv, H, scale=0.15, gen=gen)).float() * mv).half()                    # post-ReLU, post-dropout forward outputs
    vpe0 = (torch.relu(h16(B * Nv, H, scale=0.15, gen=gen)).float() * mp).half()
    spare = 2 if Nv > Pm else None
    if spare is not None:
        vis0.view(B, Nv, H)[:, spare - 1] = float("nan")
        vpe0.view(B, Nv, H)[:, spare - 1] = float("nan")
    vis, vpe = flat(B * Nv, H).set(vis0), flat(B * Nv, H).set(vpe0)
    pooled = flat(B, H).set(torch.tanh(h16(B, H, gen=gen).float() * 0.3).half())
    vmp = _masked_positions(B, Nv, Pm, spare)
    pos = vin(vmp.view(-1), fill=spare if spare is not None else 1)
    probs, sample, loss = vout(B * Pm * Pm), vout(B), vout(1)
    K.pretext_fwd(vis.view, vpe.view, pooled.view, pos.vec.view(B, Pm), probs.vec, sample.vec, loss.vec, B, Nv, Pm, H)
    for g, name in ((probs, "probs"), (sample, "sample_loss"), (loss, "loss")):
        G.assert_written(g, "logical", name)
        G.assert_finite(g.vec, name)
        G.assert_untouched(g, written="logical", name=name)
    # forward reference: fp64 sums over the same rounding points (A and sim rounded to fp16)
    idx = (vmp - 1).unsqueeze(-1).expand(-1, -1, H)
    Vm = torch.gather(vis.view.double().view(B, Nv, H), 1, idx)
    A = (torch.gather(vpe.view.float().view(B, Nv, H), 1, idx) + pooled.view.float().unsqueeze(1)).half().double()
    assert bool(torch.isfinite(Vm).all()) and bool(torch.isfinite(A).all())
    s64, amb = pretext_sim_window(A, Vm, H)                         # amb [B, Pm, Pm]: may round either way (tests/hard_inputs.py)
    sim = s64.half().double()
    ulp = float(sim.abs().max()) * 2.0 ** -10
    ls = torch.log_softmax(sim, dim=-1)
    ref_sample = torch.stack([-ls[b].diag().mean() for b in range(B)])
    ref_loss = float(ref_sample.mean())
    got_p = probs.vec.view(B, Pm, Pm)
    pd = (got_p.double() - torch.softmax(sim, -1)).abs()
    amb_row = amb.any(-1)
    note("pretext loss |got - ref| (B=%d Pm=%d H=%d, %d ambiguous sim entries)" % (B, Pm, H, int(amb.sum())), abs(float(loss.vec) - ref_loss))
    note("pretext probs max |got - ref|", float(pd.max()))
    print("[pretext] rows of probs off by more than 1e-6: %d of %d (%d hold an entry near a rounding boundary)" % (
        int((pd.amax(-1) > 1e-6).sum()), B * Pm, int(amb_row.sum())))
    if Pm == 1:
        assert float(loss.vec) == 0.0 and bool((sample.vec == 0).all()) and bool((probs.vec == 1).all())
    else:
        assert abs(float(loss.vec) - ref_loss) <= 2e-6 * abs(ref_loss) + min(int(amb.sum()), 4) * ulp / (B * Pm), (float(loss.vec), ref_loss, ulp)
        for b in range(B):
            lim = 2e-6 * abs(float(ref_sample[b])) + min(int(amb[b].sum()), 4) * ulp / Pm
            assert abs(float(sample.vec[b]) - float(ref_sample[b])) <= lim, (b, float(sample.vec[b]), float(ref_sample[b]))
        assert float(pd.max()) <= 1.2 * ulp + 1e-6, (float(pd.max()), ulp)
        off_row = pd.amax(-1) > 1e-6                                 # [B, Pm]: rows of probs that a flipped sim entry moved
        assert not bool((off_row & ~amb_row).any()), "a row of probs without an entry near a rounding boundary is off by %.3e" % float(pd[off_row & ~amb_row].max())
        assert int(off_row.sum()) <= min(int(amb.sum()), 4), "%d rows of probs are off by more than 1e-6; %d sim entries may flip, 4 are admitted" % (
            int(off_row.sum()), int(amb.sum()))
        if B * Pm > 50:                                              # one flipped row (Pm of B Pm^2 entries) fits inside test_00's 2 %: its rule as it stands
            assert float((pd > 1e-6).double().mean()) < 0.02
        assert float((got_p.sum(-1) - 1).abs().max()) < 1e-5
    for g, name in ((vis, "vis_h"), (vpe, "vispe_h"), (pooled, "pooled"), (pos, "vis_masked_pos")):
        G.assert_untouched(g, name=name)
    # backward: the closed form on the kernel's own probabilities (isolates the backward kernel from forward flips), as test_00
    gs = 4096.0
    probs_in, gscale = vin(probs.vec.clone()), vin(torch.full((1,), gs, device=DEV))
    d_vis, d_vpe, dpool = flat(B * Nv, H, fill="sentinel"), flat(B * Nv, H, fill="sentinel"), flat(B, H, fill="sentinel")
    K.pretext_bwd(vis.view, vpe.view, pooled.view, pos.vec.view(B, Pm), probs_in.vec, gscale.vec, d_vis.view, d_vpe.view, dpool.view, B, Nv, Pm, H,
                  drop_p=p, seed=seed, vis_stream=s_vis, vispe_stream=s_vpe)
    masked = torch.zeros(B, Nv, dtype=torch.bool, device=DEV)
    masked.scatter_(1, vmp - 1, True)
    masked = masked.view(-1)
    foot = masked[:, None].expand(B * Nv, H)                        # the write footprint of d_vis_h / d_vispe_h: exactly the masked rows
    for g, name in ((d_vis, "d_vis_h"), (d_vpe, "d_vispe_h")):
        G.assert_written(g, foot, name)
        G.assert_finite(g.view[masked], name)
        G.assert_untouched(g, written=foot, name=name)
    G.assert_written(dpool, "logical", "d_pooled_pre")
    G.assert_finite(dpool.view, "d_pooled_pre")
    G.assert_untouched(dpool, written="logical", name="d_pooled_pre")
    if Pm == 1:
        assert bool((G.bits(d_vis.view[masked]) == 0).all()) and bool((G.bits(d_vpe.view[masked]) == 0).all()) and bool((G.bits(dpool.view) == 0).all())
    else:
        dsim = (got_p.double() - torch.eye(Pm, device=DEV, dtype=torch.double)) * (gs / (B * Pm))
        dA, dV = dsim @ Vm, dsim.transpose(1, 2) @ A
        full_v = torch.zeros(B, Nv, H, device=DEV, dtype=torch.double).scatter_(1, idx, dV).view(B * Nv, H)
        full_e = torch.zeros(B, Nv, H, device=DEV, dtype=torch.double).scatter_(1, idx, dA).view(B * Nv, H)
        want_v = (full_v * (vis.view.float() > 0) * mv)[masked]
        want_e = (full_e * (vpe.view.float() > 0) * mp)[masked]
        want_pool = dA.sum(1) * (1.0 - pooled.view.double() ** 2)
        errs = (rel(d_vis.view[masked].float(), want_v), rel(d_vpe.view[masked].float(), want_e), rel(dpool.view.float(), want_pool))
        note("pretext bwd d_vis / d_vispe / d_pooled (B=%d Pm=%d H=%d)" % (B, Pm, H), max(errs))
        assert errs[0] < 1e-3 and errs[1] < 1e-3 and errs[2] < 1e-3, errs                             # fp16 output rounding only (test_00)
    for g, name in ((vis, "vis_h"), (vpe, "vispe_h"), (pooled, "pooled"), (pos, "vis_masked_pos"), (probs_in, "probs"), (gscale, "gscale")):
        G.assert_untouched(g, name=name)


# (B, L, Nv, Pm, caption lengths): len_b = -1 is an empty second segment (st = en = Nv + 2), len_b = L - Nv - 3 one that fills the row
# (en = L); the last case has 16 * 167 * 192 + 16 * 192 * 192 = 1 102 848 elements, past the launcher's 4096 blocks x 256 threads, so the
# grid-stride loop of vlp_mask_build takes a second trip
MASK_CASES = [(1, 5, 1, 1, [-1]), (1, 5, 1, 0, [1]), (1, 32, 8, 3, [21]), (1, 32, 29, 0, [-1]), (1, 33, 8, 8, [22]), (1, 33, 30, 7, [0]),
              (1, 256, 100, 25, [153]), (1, 256, 100, 0, [-1]), (16, 167, 100, 25, None)]


@pytest.mark.parametrize("s2s", [True, False])
@pytest.mark.parametrize("B,L,Nv,Pm,len_b", MASK_CASES)
def test_region_mask_and_mask_build_guarded(B, L, Nv, Pm, len_b, s2s):
    """vlp_region_mask_build + vlp_mask_build, with and without region_mask, bit for bit against vlp_mask_pack of the dense mask of the
    loader (as test_50) and, for `out`, against the dense mask itself.  The length vectors are guarded int32 whose guards hold st = en = 0:
    read in place of a real sample they give an all-masked row (a real row always attends column 0).  The guards of vis_masked_pos hold a
    valid position that no sample masks: read, it sets a byte of the region mask that must stay 0."""
    rng = np.random.RandomState(L + B)
    if len_b is None:
        len_b = rng.randint(0, L - Nv - 2, size=B).tolist()
        len_b[0], len_b[1], len_b[-1] = -1, L - Nv - 3, L - Nv - 3
    modes = [s2s if B == 1 else bool((b % 3 == 0) == s2s) for b in range(B)]
    st = torch.tensor([Nv + 2] * B, dtype=I32, device=DEV)
    en = torch.tensor([Nv + n + 3 for n in len_b], dtype=I32, device=DEV)
    assert int(en.max()) <= L and int((en - st).min()) >= 0
    st_g, en_g, s2s_g = vin(st, fill=0), vin(en, fill=0), vin(torch.tensor(modes, device=DEV).to(I32), fill=1)
    spare = 2 if Nv > Pm else None                                   # a position (region 1) that no sample masks
    vmp = _masked_positions(B, Nv, Pm, spare).cpu()
    pos = vin(vmp.view(-1).to(DEV) if Pm else torch.ones(1, dtype=I64, device=DEV), fill=spare if spare is not None else 1)
    rmask = vout(B * Nv, U8)
    K.region_mask_build(pos.vec, rmask.vec, B, Pm, Nv)
    want_r = torch.zeros(B, Nv, dtype=U8)
    if Pm:
        want_r.scatter_(1, vmp - 1, 1)
    assert torch.equal(rmask.vec.cpu().view(B, Nv), want_r)
    G.assert_untouched(rmask, written="logical", name="region mask")
    G.assert_untouched(pos, name="vis_masked_pos")
    rmask_in = vin(rmask.vec.clone(), fill=1)                       # guards: "masked", so a stray read blocks a column that must attend
    Lp = (L + 31) // 32 * 32
    for with_regions in (False, True):
        dense = torch.from_numpy(np.stack([LO.attention_mask(Nv, int(n), L, "s2s" if m else "bi") for n, m in zip(len_b, modes)]))
        if with_regions:
            for b in range(B):
                dense[b][:, vmp[b]] = 0
        dense = dense.to(DEV)
        ref, ref_t = torch.empty(B, L, Lp, dtype=U8, device=DEV), torch.empty(B, Lp, Lp, dtype=U8, device=DEV)
        K.mask_pack(dense, ref, B, L, Lp, out_t=ref_t)
        out, out_t = vout(B * L * Lp, U8), vout(B * Lp * Lp, U8)
        if with_regions:
            K.mask_build(st_g.vec, en_g.vec, s2s_g.vec, out.vec.view(B, L, Lp), B, L, Lp, out_t=out_t.vec.view(B, Lp, Lp), region_mask=rmask_in.vec, Nv=Nv)
        else:
            K.mask_build(st_g.vec, en_g.vec, s2s_g.vec, out.vec.view(B, L, Lp), B, L, Lp, out_t=out_t.vec.view(B, Lp, Lp))
        tag = " (region_mask)" if with_regions else ""
        assert torch.equal(out.vec.view(B, L, Lp), ref), "out" + tag
        assert torch.equal(out_t.vec.view(B, Lp, Lp), ref_t), "out_t" + tag
        direct = torch.cat([dense.to(U8), torch.full((B, L, Lp - L), 2, dtype=U8, device=DEV)], -1)
        assert torch.equal(out.vec.view(B, L, Lp), direct), "out vs the dense mask" + tag
        G.assert_untouched(out, written="logical", name="out" + tag)
        G.assert_untouched(out_t, written="logical", name="out_t" + tag)
        for g, name in ((st_g, "second_st"), (en_g, "second_end"), (s2s_g, "is_s2s"), (rmask_in, "region_mask")):
            G.assert_untouched(g, name=name)


# (B, Nv, n_cls, class input is f32, pad_to - roundup8(6 + n_cls)); B * Nv = 1, 195, 65 are no multiple of the 4 rows of a block
@pytest.mark.parametrize("B,Nv,n_cls,f32,extra", [(1, 1, 1, False, 0), (3, 36, 63, True, 8), (2, 64, 64, False, 0), (3, 65, 65, True, 16),
                                                   (1, 100, 1601, False, 56), (1, 65, 2048, True, 0), (1, 36, 1601, True, 0), (3, 65, 1, False, 8)])
def test_vis_pe_prep_guarded(B, Nv, n_cls, f32, extra, gen):
    """vlp_vis_pe_prep against oracle/loader_oracle.vis_pe_prepare (float64) on the values the kernel is given, test_50's bound
    5.5e-4 |want| + 1e-4 (fp32 arithmetic and one fp16 rounding).  ld_cls > n_cls with NaN in the padding, NaN around the boxes,
    ld_out > pad_to; columns [6 + n_cls, pad_to) exactly zero, [pad_to, ld_out) untouched.  Degenerate rows (Nv >= 3): region 0 a zero-area
    box, region 1 a box with x2 < x1 (the area clamps to 0), region 2 a constant class row (variance 0: exactly 0 wanted)."""
    rows = B * Nv
    pad_to = roundup8(6 + n_cls) + extra
    xy = torch.rand(B, Nv, 4, device=DEV, generator=gen) * torch.tensor([300.0, 200.0, 300.0, 200.0], device=DEV)
    box = torch.cat([xy[..., :2], xy[..., :2] + xy[..., 2:] + 1.0, torch.zeros(B, Nv, 1, device=DEV),
                     torch.rand(B, Nv, 1, device=DEV, generator=gen)], -1)                      # x1, y1, x2 > x1, y2 > y1, -, confidence
    cls = torch.softmax(3.0 * torch.randn(rows, n_cls, device=DEV, generator=gen), -1)
    if Nv >= 3:
        box[:, 0, 2] = box[:, 0, 0]
        box[:, 1, 2] = box[:, 1, 0] - 7.0
        cls.view(B, Nv, n_cls)[:, 2] = 0.25
    cls = cls if f32 else cls.half()
    bbox = vin(box.reshape(-1))
    cls_g = gin(cls, pad=8)
    out = gout(rows, pad_to, pad=8)
    assert cls_g.ld > n_cls and out.ld > pad_to
    K.vis_pe_prep(bbox.vec.view(B, Nv, 6), cls_g.view, out.view, B, Nv, n_cls, pad_to)
    G.assert_written(out, "logical", "out")
    G.assert_finite(out.view, "out")
    got = out.view.double().cpu().numpy().reshape(B, Nv, pad_to)
    bb, cc = box.double().cpu().numpy(), cls_g.view.double().cpu().numpy().reshape(B, Nv, n_cls)
    worst = 0.0
    for b in range(B):
        want = LO.vis_pe_prepare(bb[b], cc[b])
        if Nv >= 3:
            assert np.all(want[2, 6:] == 0)
        err = np.abs(got[b, :, :6 + n_cls] - want)
        worst = max(worst, float((err - 5.5e-4 * np.abs(want)).max()))
        assert np.all(err <= 5.5e-4 * np.abs(want) + 1e-4), (b, float(err.max()))
    note("vis_pe_prep max(|got - want| - 5.5e-4 |want|), bound 1e-4 (B=%d Nv=%d n_cls=%d)" % (B, Nv, n_cls), worst)
    G.assert_zero_band(out, 6 + n_cls, pad_to, "out")
    G.assert_untouched(out, written="logical", name="out")
    G.assert_untouched(bbox, name="bbox")
    G.assert_untouched(cls_g, name="cls")
