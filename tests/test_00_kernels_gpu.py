"""GPU parity tests of every HIP kernel, called THROUGH THE C ABI (vlp_amd._lib -> libvlp_hip.so), against
fp32/fp64 torch restatements of the same op (the path is floating point; tolerances are written next to
each check).  Run on the MI355X box:  python -m pytest tests -m gpu -x -q
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from vlp_amd import _lib as K          # noqa: E402
from oracle import vlp_oracle as O      # noqa: E402   (checker only)

from tests.kernel_util import DEV, LAB, NT_PRODUCT, drop_mult_ref, h16, nt_variants, rel     # noqa: E402,F401   (shared with test_05 / test_06)
from tests.kernel_util import attn_mask as _mask, attn_ref as _attn_ref                      # noqa: E402


@pytest.fixture
def gen():
    g = torch.Generator(device=DEV)
    g.manual_seed(1234)
    return g


# =====================================================================================================
# NT GEMM
# =====================================================================================================
@pytest.mark.parametrize("variant", [0, 1, 2, 3, 4, 5, 9, 10, 12, 13])
@pytest.mark.parametrize("M,N,K", [(128, 128, 64), (300, 256, 128), (1000, 768, 768), (77, 1000, 192), (256, 2304, 768)])
def test_gemm_nt_plain(variant, M, N, K, gen):
    Kd = K
    from vlp_amd import _lib as K   # the parametrize name shadows the module alias inside this test
    x, w = h16(M, Kd, gen=gen), h16(N, Kd, scale=0.05, gen=gen)
    ldy = (N + 7) // 8 * 8
    y = torch.full((M, ldy), 7.0, device=DEV, dtype=torch.half)
    K.gemm_nt(x, w, y, M, N, Kd, variant=variant)
    ref = x.float() @ w.float().t()
    # fp32 accumulate, one fp16 rounding of the result: 2^-11 relative + accumulation-order noise
    assert rel(y[:, :N].float(), ref) < 1.5e-3, "variant %d" % variant
    if ldy > N:
        assert float(y[:, N:].abs().max()) == 0.0        # padding columns are written as zero


@pytest.mark.parametrize("variant", nt_variants([6, 7, 14, 15, 22, 23, 54, 17, 19, 27, 21, 29, 53, 61, 64, 65, 66, 67, 68, 69, 70, 71, 72, 73, 77, 78, 192, 193, 194, 201, 202]))
@pytest.mark.parametrize("M,N,K", [(300, 256, 128), (1000, 768, 768), (77, 1000, 192), (256, 2304, 768), (515, 520, 1664),
                                   (10688, 768, 3072), (10688, 2304, 768)])
def test_gemm_nt_phased(variant, M, N, K, gen):
    """Phased 256-row kernels (gemm_nt_ph.hip: counted-vmcnt LDS-DMA pipeline with two staggered wave groups) and the ring kernels of
    gemm_nt.hip (17 / 19 / 21, +8 XCD order), and the wave-pipelined family of gemm_nt_wp.hip (64 + cfg, +8 XCD order).  Repeated launches
    on the same inputs must be bit-identical (a race between DMA and fragment reads would show up as run-to-run differences)."""
    Kd = K
    from vlp_amd import _lib as K
    x, w = h16(M, Kd, gen=gen), h16(N, Kd, scale=0.05, gen=gen)
    ldy = (N + 7) // 8 * 8
    ref = x.float() @ w.float().t()
    first = None
    for it in range(4):
        y = torch.full((M, ldy), 7.0, device=DEV, dtype=torch.half)
        K.gemm_nt(x, w, y, M, N, Kd, variant=variant)
        assert rel(y[:, :N].float(), ref) < 1.5e-3, "variant %d run %d" % (variant, it)
        if first is None:
            first = y.clone()
        else:
            assert torch.equal(first, y), "variant %d: run %d differs from run 0" % (variant, it)
    if variant < 64 and variant & 7 in (6, 7):
        with pytest.raises(RuntimeError):
            K.gemm_nt(x[:, :64], w[:, :64], y, M, N, 64, ldx=Kd, ldw=Kd, variant=variant)       # K < 128 is refused, not mis-computed
    else:                                       # ring variants (17, 19, 27): a single k tile works too (clamped refills)
        y1 = torch.zeros(M, ldy, device=DEV, dtype=torch.half)
        K.gemm_nt(x[:, :64], w[:, :64], y1, M, N, 64, ldx=Kd, ldw=Kd, variant=variant)
        assert rel(y1[:, :N].float(), x[:, :64].float() @ w[:, :64].float().t()) < 1.5e-3


def test_gemm_nt_variant_identity(gen):
    """the full-size report lists the SAME 16-digit logits error under every forced variant, including the
    32x32x16-MFMA family.  Two questions, answered here on one GEMM of the step (10 688 x 768 x 3072):
      (a) does a forced variant reach the kernel it names?  vlp_gemm_nt_resolved_variant() returns what the launcher ran after its
          fallbacks -- asserted for the rings (27, 29), the wave-pipelined kernels (73, 77) and the fallback cases;
      (b) are the fp16 outputs of the 16x16x32 chains (rings) and the 32x32x16 chains (wave-pipelined) bit-identical?  Both walk k in
          ascending order and accumulate in fp32; whether one 16x16x32 MFMA rounds like two 32x32x16 steps is a property of the matrix
          pipe.  The outcome is recorded in gpurun_out/nt_variant_identity.json and asserted to be what round 4 measured
          (see DESIGN.md section 4)."""
    import json
    import os
    M, N, Kd = 10688, 768, 3072
    x, w = h16(M, Kd, gen=gen), h16(N, Kd, scale=0.05, gen=gen)
    out, resolved = {}, {}
    for v in (27, 29, 13, 73, 77, 69):
        y = torch.full((M, N), 7.0, device=DEV, dtype=torch.half)
        K.gemm_nt(x, w, y, M, N, Kd, variant=v)
        resolved[v] = K.gemm_nt_resolved_variant()
        out[v] = y
        assert resolved[v] == v, (v, resolved[v])                      # plain epilogue: nothing falls back
    # a wave-pipelined variant with an erf epilogue has no instantiation: the launcher must say that it ran a ring instead
    y = torch.empty(M, N, device=DEV, dtype=torch.half)
    K.gemm_nt(x, w, y, M, N, Kd, act=K.ACT_GELU, variant=77)
    assert K.gemm_nt_resolved_variant() == 27
    K.gemm_nt(x, w, y, M, N, Kd, act=K.ACT_GELU_SAVE_GRAD, preact=torch.empty_like(y), variant=77)
    assert K.gemm_nt_resolved_variant() == 77
    same = {"%d_vs_%d" % (a, b): bool(torch.equal(out[a], out[b])) for a, b in ((27, 29), (27, 13), (73, 77), (77, 69), (27, 77), (29, 73))}
    ulp = {k: float((out[int(k.split("_")[0])].float() - out[int(k.split("_")[2])].float()).abs().max()) for k in same}
    os.makedirs("gpurun_out", exist_ok=True)
    with open("gpurun_out/nt_variant_identity.json", "w") as f:
        json.dump({"shape": [M, N, Kd], "resolved": {str(k): v for k, v in resolved.items()}, "bit_identical": same, "max_abs_diff": ulp}, f, indent=1)
    # within an MFMA family the chain per output element does not depend on the tile shape
    assert same["27_vs_29"] and same["27_vs_13"] and same["73_vs_77"] and same["77_vs_69"], same
    # across the families: measured in round 4 (profiles/r04_nt_variant_identity.json)
    if NT_FAMILIES_BIT_IDENTICAL is not None:
        assert same["27_vs_77"] == NT_FAMILIES_BIT_IDENTICAL and same["29_vs_73"] == NT_FAMILIES_BIT_IDENTICAL, (same, ulp)


@pytest.mark.parametrize("M,N,K,cap", [(1000, 512, 640, 5), (1000, 512, 640, 0), (700, 384, 1024, 2), (2085, 2304, 768, 7), (10688, 3072, 768, 0), (10688, 2304, 768, 0),
                                         (10688, 768, 3072, 0), (10688, 3072, 768, 100)])
@pytest.mark.parametrize("epi", ["bias", "plain", "sg", "mul"])
def test_gemm_nt_persistent_stream(M, N, K, cap, epi, gen, monkeypatch):
    """gemm_nt_ps.hip (variant 256 / 264): one workgroup per CU walks a run of 256x128 tiles as one k stream and stores a finished tile in
    slices behind the next tile's k tiles.  Its three epilogues must be BIT-identical to the ring kernels' (same MFMA chain, same epilogue
    arithmetic), whatever the run length (`VLP_NT_PS_GRID` caps the workgroups of the launch: runs of 1 .. 17 tiles, ragged last run,
    ragged last row tile), and repeated launches must agree (deferred stores + LDS-DMA ring share the vmcnt counter)."""
    Kd = K
    from vlp_amd import _lib as K
    if cap:
        monkeypatch.setenv("VLP_NT_PS_GRID", str(cap))
    else:
        monkeypatch.delenv("VLP_NT_PS_GRID", raising=False)
    x, w = h16(M, Kd, gen=gen), h16(N, Kd, scale=0.05, gen=gen)
    kw = {}
    if epi in ("bias", "sg"):
        kw["bias"] = h16(N, scale=0.5, gen=gen)
    if epi == "mul":
        kw.update(mul_src=h16(M, N, gen=gen), mul_mode=K.MUL_PLAIN)

    def run(variant):
        y = torch.full((M, N), 7.0, device=DEV, dtype=torch.half)
        pre = torch.full((M, N), 5.0, device=DEV, dtype=torch.half) if epi == "sg" else None
        if epi == "sg":
            K.gemm_nt(x, w, y, M, N, Kd, act=K.ACT_GELU_SAVE_GRAD, preact=pre, variant=variant, **kw)
        else:
            K.gemm_nt(x, w, y, M, N, Kd, variant=variant, **kw)
        return y, pre, K.gemm_nt_resolved_variant()

    y_ref, pre_ref, rv = run(29 if N > 1024 else 27)
    for variant in (256, 264):
        first = None
        for it in range(3):
            y, pre, rv = run(variant)
            assert rv == variant, (variant, rv)
            assert torch.equal(y, y_ref), "variant %d run %d: Y differs from the ring (max abs %g)" % (variant, it, float((y.float() - y_ref.float()).abs().max()))
            if epi == "sg":
                assert torch.equal(pre, pre_ref), "variant %d run %d: stored derivative differs" % (variant, it)
    z = x.float() @ w.float().t()
    if "bias" in kw:
        z = z + kw["bias"].float()
    if epi == "sg":
        z = torch.nn.functional.gelu(z.half().float())
    if epi == "mul":
        z = z * kw["mul_src"].float()
    assert rel(y_ref.float(), z) < 2e-3


def test_gemm_nt_persistent_stream_fallbacks(gen):
    """What the persistent kernel does not carry runs on a ring, and the launcher says so."""
    M, N, Kd = 600, 256, 640
    x, w = h16(M, Kd, gen=gen), h16(N, Kd, scale=0.05, gen=gen)
    y = torch.empty(M, N, device=DEV, dtype=torch.half)
    K.gemm_nt(x, w, y, M, N, Kd, variant=264, residual=h16(M, N, gen=gen))
    assert K.gemm_nt_resolved_variant() == 27
    K.gemm_nt(x, w, y, M, N, Kd, variant=264, act=K.ACT_GELU)
    assert K.gemm_nt_resolved_variant() == 27
    K.gemm_nt(x, w, y, M, N, Kd, variant=264, dropout_p=0.1, seed=3)
    assert K.gemm_nt_resolved_variant() == 27
    K.gemm_nt(x[:, :512], w[:, :512], y, M, N, 512, ldx=Kd, ldw=Kd, variant=264)          # 8 k tiles: no room for the eight store slices
    assert K.gemm_nt_resolved_variant() == 27
    y2 = torch.empty(M, 1000, device=DEV, dtype=torch.half)
    K.gemm_nt(x, h16(1000, Kd, scale=0.05, gen=gen), y2, M, 1000, Kd, variant=264)        # N % 128 != 0
    assert K.gemm_nt_resolved_variant() == 27
    K.gemm_nt(x, w, y, M, N, Kd, variant=264)
    assert K.gemm_nt_resolved_variant() == 264


NT_FAMILIES_BIT_IDENTICAL = True      # measured in round 4 (profiles/r04_nt_variant_identity.json): one 16x16x32 MFMA rounds like two 32x32x16 k16 steps


@pytest.mark.parametrize("M,N,K,splits", [(128, 768, 3072, 8), (128, 2304, 768, 4), (640, 768, 768, 3), (77, 1000, 192, 2), (320, 3072, 768, 12),
                                            (128, 768, 768, 64)])
def test_gemm_nt_splitk(M, N, K, splits, gen):
    """Split-K NT GEMM for the decoder's skinny shapes: plain result, fused epilogues after the slice reduction, determinism."""
    Kd = K
    from vlp_amd import _lib as K
    x, w = h16(M, Kd, gen=gen), h16(N, Kd, scale=0.05, gen=gen)
    ldy = (N + 7) // 8 * 8
    ws = torch.full((K.gemm_nt_splitk_workspace_bytes(M, N, splits) // 4,), float("nan"), device=DEV)     # stale scratch must not matter
    ref = x.float() @ w.float().t()
    y = torch.full((M, ldy), 7.0, device=DEV, dtype=torch.half)
    K.gemm_nt_splitk(x, w, y, M, N, Kd, splits, ws)
    assert rel(y[:, :N].float(), ref) < 1.5e-3
    if ldy > N:
        assert float(y[:, N:].abs().max()) == 0.0
    y2 = torch.empty_like(y)
    K.gemm_nt_splitk(x, w, y2, M, N, Kd, splits, ws)
    assert torch.equal(y, y2)
    bias, res = h16(N, gen=gen), h16(M, ldy, gen=gen)
    K.gemm_nt_splitk(x, w, y, M, N, Kd, splits, ws, bias=bias, act=K.ACT_GELU)
    lin = ref + bias.float()
    assert rel(y[:, :N].float(), lin * 0.5 * (1 + torch.erf(lin / math.sqrt(2)))) < 2e-3
    K.gemm_nt_splitk(x, w, y, M, N, Kd, splits, ws, bias=bias, residual=res, alpha=0.5)
    assert rel(y[:, :N].float(), 0.5 * ref + bias.float() + res[:, :N].float()) < 2e-3
    with pytest.raises(RuntimeError):
        K.gemm_nt_splitk(x, w, y, M, N, Kd, splits, ws[:16])                # workspace too small is refused


@pytest.mark.parametrize("variant", nt_variants([0, 1, 2, 3, 64, 65, 66, 67, 68, 69, 70, 71, 192, 193, 194]))
def test_gemm_nt_asymmetric_identity(variant):
    """A = I against an asymmetric B catches swapped row/col in the MFMA C-layout handling."""
    M = N = Kd = 128
    x = torch.eye(M, Kd, device=DEV).half()
    w = (torch.arange(N, device=DEV)[:, None] * 0.01 + torch.arange(Kd, device=DEV)[None, :] * 1.0).half()
    y = torch.zeros(M, N, device=DEV, dtype=torch.half)
    K.gemm_nt(x, w, y, M, N, Kd, variant=variant)
    assert torch.equal(y, w.t().contiguous())


@pytest.mark.parametrize("variant", nt_variants([0, 1, 2, 3, 5, 6, 7, 19, 27, 29, 61, 64, 65, 66, 67, 68, 69, 70, 71, 73, 77, 192, 193, 194]))
def test_gemm_nt_epilogues(variant, gen):
    M, N, Kd = 200, 384, 256
    x, w = h16(M, Kd, gen=gen), h16(N, Kd, scale=0.06, gen=gen)
    bias, res = h16(N, gen=gen), h16(M, N, gen=gen)
    lin = x.float() @ w.float().t() + bias.float()
    # bias + gelu (+ pre-activation output)
    y = torch.empty(M, N, device=DEV, dtype=torch.half)
    z = torch.empty(M, N, device=DEV, dtype=torch.half)
    K.gemm_nt(x, w, y, M, N, Kd, bias=bias, preact=z, act=K.ACT_GELU, variant=variant)
    assert rel(z.float(), lin) < 1.5e-3
    assert rel(y.float(), O.gelu(z.float())) < 1.5e-3          # gelu is applied to the fp16-rounded pre-activation
    # relu, tanh
    K.gemm_nt(x, w, y, M, N, Kd, bias=bias, act=K.ACT_RELU, variant=variant)
    assert rel(y.float(), torch.relu(lin)) < 1.5e-3
    K.gemm_nt(x, w, y, M, N, Kd, bias=bias, act=K.ACT_TANH, variant=variant)
    assert rel(y.float(), torch.tanh(lin)) < 1.5e-3
    # bias + residual, alpha
    K.gemm_nt(x, w, y, M, N, Kd, bias=bias, residual=res, alpha=0.5, variant=variant)
    assert rel(y.float(), 0.5 * (x.float() @ w.float().t()) + bias.float() + res.float()) < 1.5e-3
    # multiplier epilogues (dgrad through gelu / relu)
    src = h16(M, N, gen=gen)
    K.gemm_nt(x, w, y, M, N, Kd, mul_src=src, mul_mode=K.MUL_GELU_GRAD, variant=variant)
    s32 = src.float().requires_grad_(True)
    O.gelu(s32).sum().backward()
    assert rel(y.float(), (x.float() @ w.float().t()) * s32.grad) < 2e-3
    K.gemm_nt(x, w, y, M, N, Kd, mul_src=src, mul_mode=K.MUL_RELU_MASK, variant=variant)
    assert rel(y.float(), (x.float() @ w.float().t()) * (src.float() > 0)) < 1.5e-3
    # dropout + residual: exact mask from the python mirror of the hash; element = (row m, col n)
    p, seed, stream = 0.3, 99, 5
    K.gemm_nt(x, w, y, M, N, Kd, bias=bias, residual=res, dropout_p=p, seed=seed, rng_stream=stream, variant=variant)
    mult = drop_mult_ref(p, seed, stream, range(M), range(N))
    assert rel(y.float(), lin * mult + res.float()) < 1.5e-3
    frac = float((mult == 0).float().mean())
    assert abs(frac - p) < 0.01
    # gelu with the derivative saved for backward: y = gelu(z16), `preact` <- gelu'(z16) (z16 = fp16-rounded pre-activation);
    # the dgrad side then multiplies by the stored derivative (MUL_PLAIN)
    gp = torch.empty(M, N, device=DEV, dtype=torch.half)
    # (the phased kernels 6 / 7 do not instantiate the save-grad epilogue; vlp_gemm_nt runs those calls on the ring kernels)
    K.gemm_nt(x, w, y, M, N, Kd, bias=bias, preact=gp, act=K.ACT_GELU_SAVE_GRAD, variant=variant)
    z32 = z.float().requires_grad_(True)                    # z from the ACT_GELU call above: the same fp16-rounded pre-activation
    O.gelu(z32).sum().backward()
    assert rel(y.float(), O.gelu(z.float())) < 1.5e-3
    assert rel(gp.float(), z32.grad) < 1.5e-3
    K.gemm_nt(x, w, y, M, N, Kd, mul_src=gp, mul_mode=K.MUL_PLAIN, variant=variant)
    assert rel(y.float(), (x.float() @ w.float().t()) * gp.float()) < 1.5e-3


def test_c_only_consumer_two_host_threads(tmp_path):
    """tests/c_abi_smoke.c: a C program (no Python, no torch) links libvlp_hip.so through include/vlp_hip.h and drives vlp_gemm_nt +
    vlp_layernorm_fwd from TWO host threads, each on its own stream, checking the results against plain C arithmetic (SURVEY.md 8b
    threading contract; first calls race on the launchers' once-per-device state)."""
    import os
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if shutil.which("gcc") is None:
        pytest.skip("needs gcc")
    exe = os.path.join(str(tmp_path), "c_abi_smoke")
    libdir = os.path.join(root, "vlp_amd")
    r = subprocess.run(["gcc", "-O2", "-std=c11", "-D__HIP_PLATFORM_AMD__", "-D_GNU_SOURCE", "-I", os.path.join(root, "include"), "-I", "/opt/rocm/include",
                        os.path.join(root, "tests", "c_abi_smoke.c"), "-o", exe, "-L", libdir, "-lvlp_hip", "-L", "/opt/rocm/lib", "-lamdhip64", "-lpthread",
                        "-lm", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "c_abi_smoke ok" in r.stdout, (r.stdout, r.stderr)


def test_gemm_nt_rejects_bad_args():
    x = torch.zeros(8, 100, device=DEV, dtype=torch.half)
    with pytest.raises(RuntimeError, match="multiple of 64"):
        K.gemm_nt(x, x, x, 8, 8, 100)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        K.gemm_nt(x.cpu(), x, x, 8, 8, 64)


# =====================================================================================================
# TN GEMM (wgrad), colsum
# =====================================================================================================
@pytest.mark.parametrize("variant", [0, 1, 9, 2, 10, 26, 3, 4])
@pytest.mark.parametrize("M,N,K,splits", [(64, 128, 128, 1), (1000, 256, 384, 1), (1000, 256, 384, 4), (192, 1000, 768, 1),
                                          (2000, 768, 768, 0), (333, 72, 64, 2)])
def test_gemm_tn(variant, M, N, K, splits, gen):
    Kd = K
    from vlp_amd import _lib as K
    a, b = h16(M, (N + 7) // 8 * 8, scale=0.3, gen=gen), h16(M, Kd, scale=0.3, gen=gen)
    c = h16(N, Kd, gen=gen)
    ws = torch.empty(K_ws(M, N, Kd), device=DEV, dtype=torch.uint8)
    ref = a[:, :N].float().t() @ b.float()
    K.gemm_tn(a, b, c, M, N, Kd, beta=0, workspace=ws, variant=variant, splits=splits)
    assert rel(c.float(), ref) < 1.5e-3, "variant %d" % variant
    K.gemm_tn(a, b, c, M, N, Kd, beta=1, workspace=ws, variant=variant, splits=splits)
    assert rel(c.float(), 2 * ref) < 2.5e-3
    # fused bias gradient (column sums of A)
    bias = h16(N, gen=gen)
    b0 = bias.clone()
    K.gemm_tn(a, b, c, M, N, Kd, beta=0, workspace=ws, variant=variant, splits=splits, bias_out=bias)
    cs = a[:, :N].float().sum(0)
    assert float((bias.float() - cs).abs().max()) < 2e-3 * float(cs.abs().max()) + 1e-2
    assert rel(c.float(), ref) < 1.5e-3
    b0_before = b0.float().clone()
    K.gemm_tn(a, b, c, M, N, Kd, beta=1, workspace=ws, variant=variant, splits=splits, bias_out=b0)
    # beta = 1 accumulates into the bias gradient as well: previous value + column sums (one more fp16 rounding)
    want = b0_before + cs
    assert float((b0.float() - want).abs().max()) < 2e-3 * float(want.abs().max()) + 2e-2
    assert rel(c.float(), 2 * ref) < 2.5e-3


def K_ws(M, N, Kd):
    return K.gemm_tn_workspace_bytes(M, N, Kd)


def test_gemm_tn_grouped(gen):
    """vlp_gemm_tn_grouped: several wgrads in one grid, every workgroup walking its problem's whole contraction (no split-M slabs).
    Shapes: ragged N / K / M (tile tails, zero-filled last stage), beta = 0 and 1, fused bias gradients, a problem without bias;
    repeated launches are bit-identical and equal to the single-problem kernel with splits = 1 (same accumulation order)."""
    shapes = [(1000, 256, 384), (1000, 768, 768), (777, 72, 64), (1000, 1000, 128), (2048 + 37, 2304, 768)]
    probs, refs, cs = [], [], []
    for i, (M, N, Kd) in enumerate(shapes):
        a, b = h16(M, (N + 7) // 8 * 8, scale=0.3, gen=gen), h16(M, Kd, scale=0.3, gen=gen)
        c = h16(N, Kd, gen=gen)
        bias = h16(N, gen=gen) if i != 2 else None
        probs.append([a, b, c, M, N, Kd, 0, bias])
        refs.append(a[:, :N].float().t() @ b.float())
        cs.append(a[:, :N].float().sum(0))
    K.gemm_tn_grouped([tuple(q) for q in probs])
    first = [q[2].clone() for q in probs]
    for q, ref, col in zip(probs, refs, cs):
        assert rel(q[2].float(), ref) < 1.5e-3
        if q[7] is not None:
            assert float((q[7].float() - col).abs().max()) < 2e-3 * float(col.abs().max()) + 1e-2
    # single-problem kernel, no split: identical bits
    for q, f in zip(probs, first):
        a, b, c, M, N, Kd, _, _ = q
        c1 = torch.empty_like(c)
        ws = torch.empty(K_ws(M, N, Kd), device=DEV, dtype=torch.uint8)
        K.gemm_tn(a, b, c1, M, N, Kd, beta=0, workspace=ws, variant=2, splits=1)
        assert torch.equal(c1, f)
    # beta = 1 accumulates (weights and biases); run twice from the same start -> same bits
    outs = []
    for rep in range(2):
        for q, f in zip(probs, first):
            q[2].copy_(f)
            q[6] = 1
        K.gemm_tn_grouped([tuple(q) for q in probs])
        outs.append([q[2].clone() for q in probs])
    for x, y, ref in zip(outs[0], outs[1], refs):
        assert torch.equal(x, y)
        assert rel(x.float(), 2 * ref) < 2.5e-3
    with pytest.raises(RuntimeError, match="1..8"):
        K.gemm_tn_grouped([tuple(probs[0])] * 9)


@pytest.mark.skipif(not LAB, reason="investigation variant: needs a -DVLP_LAB_BUILD library")
@pytest.mark.parametrize("M", [10688, 1000, 64 * 14 + 5])
def test_gemm_tn_grouped_stream_k(M, gen, monkeypatch):
    """Stream-K form of the grouped launch (VLP_TN_GROUP_MODE=5, gemm_tn_grouped_sk_kernel): six tiles are dealt to seven workgroups in equal
    runs of contraction stages, every tile is cut once and its two fp32 chains meet through the workspace.  Against the plain grouped
    launch: equal up to the fp32 summation order (two chains instead of one), bias gradients included; repeated launches bit-identical
    (the hand-off is deterministic); beta = 1 accumulates; without a workspace, or with a tile count that is not a multiple of 6, the
    launcher runs the plain form (bit-identical to it)."""
    shapes = [(256, 384), (768, 768), (384, 128)]           # 6 + 36 + 3 = 45 tiles -> pad with a fourth problem to a multiple of 6
    shapes.append((384, 128))                                # 48 tiles = 8 groups, 56 workgroups
    def make():
        probs = []
        g2 = torch.Generator(device=DEV); g2.manual_seed(99)
        for i, (N, Kd) in enumerate(shapes):
            a, b = h16(M, N, scale=0.3, gen=g2), h16(M, Kd, scale=0.3, gen=g2)
            probs.append([a, b, h16(N, Kd, gen=g2), M, N, Kd, 0, h16(N, gen=g2) if i != 2 else None])
        return probs
    tiles = sum((N // 128) * (Kd // 128) for N, Kd in shapes)
    assert tiles % 6 == 0
    wsk = torch.empty(K.gemm_tn_grouped_workspace_bytes(tiles), device=DEV, dtype=torch.uint8)
    monkeypatch.setenv("VLP_TN_GROUP_MODE", "0")
    plain = make()
    K.gemm_tn_grouped([tuple(q) for q in plain])
    monkeypatch.setenv("VLP_TN_GROUP_MODE", "5")
    runs = []
    for rep in range(3):
        sk = make()
        wsk.fill_(0xFF if rep == 1 else 0)                   # stale partials / flags from another launch must not matter
        K.gemm_tn_grouped([tuple(q) for q in sk], workspace=wsk)
        runs.append(sk)
    for q0, q1, q2, qp in zip(runs[0], runs[1], runs[2], plain):
        assert torch.equal(q0[2], q1[2]) and torch.equal(q0[2], q2[2])
        ref = q0[0].float().t() @ q0[1].float()
        assert rel(q0[2].float(), ref) < 1.5e-3
        assert rel(q0[2].float(), qp[2].float()) < 1.5e-3
        if q0[7] is not None:
            assert torch.equal(q0[7], q1[7])
            col = q0[0].float().sum(0)
            assert float((q0[7].float() - col).abs().max()) < 2e-3 * float(col.abs().max()) + 1e-2
    if M >= 64 * 14:
        assert any(not torch.equal(q0[2], qp[2]) for q0, qp in zip(runs[0], plain)), "two chains per tile should differ from one chain in the last bit somewhere"
    # beta = 1
    acc = make()
    for q, q0 in zip(acc, runs[0]):
        q[2].copy_(q0[2]); q[6] = 1
        if q[7] is not None:
            q[7].copy_(q0[7])
    K.gemm_tn_grouped([tuple(q) for q in acc], workspace=wsk)
    for q, q0 in zip(acc, runs[0]):
        assert rel(q[2].float(), 2 * q0[2].float()) < 2e-3
    # fallbacks: no workspace / tile count not a multiple of 6 -> the plain kernel, bit for bit
    nows = make()
    K.gemm_tn_grouped([tuple(q) for q in nows])
    odd = make()[:3]
    K.gemm_tn_grouped([tuple(q) for q in odd], workspace=wsk)
    for q, qp in zip(nows, plain):
        assert torch.equal(q[2], qp[2])
    for q, qp in zip(odd, plain):
        assert torch.equal(q[2], qp[2])


@pytest.mark.parametrize("variant", [0, 1, 2, 3, 4])
def test_gemm_tn_asymmetric(variant):
    """dY = I-like selector against an asymmetric X: dW[n,k] must equal X[n,k] for n < M."""
    M, N, Kd = 128, 128, 128
    a = torch.eye(M, N, device=DEV).half()
    b = (torch.arange(M, device=DEV)[:, None] * 1.0 + torch.arange(Kd, device=DEV)[None, :] * 0.01).half()
    c = torch.zeros(N, Kd, device=DEV, dtype=torch.half)
    ws = torch.empty(K_ws(M, N, Kd), device=DEV, dtype=torch.uint8)
    K.gemm_tn(a, b, c, M, N, Kd, workspace=ws, variant=variant, splits=1)
    assert torch.equal(c, b)


@pytest.mark.parametrize("M,N", [(10, 64), (1000, 768), (4097, 1000), (192, 28996)])
def test_colsum(M, N, gen):
    lda = (N + 7) // 8 * 8
    a = h16(M, lda, gen=gen)
    out = h16(N, gen=gen)
    out0 = out.clone()
    ws = torch.empty(K.colsum_workspace_bytes(M, N), device=DEV, dtype=torch.uint8)
    K.colsum(a, out, M, N, beta=0, workspace=ws)
    ref = a[:, :N].float().sum(0)
    assert float((out.float() - ref).abs().max()) < 1e-3 * float(ref.abs().max()) + 1e-2
    prev = out0.float().clone()
    K.colsum(a, out0, M, N, beta=1, workspace=ws)
    want = prev + ref                          # beta = 1: previous value + column sums
    assert float((out0.float() - want).abs().max()) < 1e-3 * float(want.abs().max()) + 1e-2


# =====================================================================================================
# attention
# =====================================================================================================
@pytest.mark.parametrize("B,L,Nv,heads", [(2, 43, 8, 2), (3, 123, 100, 12), (2, 167, 100, 12), (1, 256, 100, 4), (2, 64, 20, 1)])
def test_attention_fwd_bwd(B, L, Nv, heads, gen):
    gc = torch.Generator().manual_seed(5)
    H = heads * 64
    qkv = h16(B * L, 3 * H, scale=1.0, gen=gen)
    mask = _mask(B, L, Nv, gc).to(DEV)
    Lp = (L + 31) // 32 * 32
    mb = torch.empty(B, L, Lp, device=DEV, dtype=torch.uint8)
    mt = torch.empty(B, Lp, Lp, device=DEV, dtype=torch.uint8)
    K.mask_pack(mask, mb, B, L, Lp, out_t=mt)
    assert torch.equal(mb[:, :, :L].long(), mask) and (Lp == L or int(mb[:, :, L:].min()) == 2)
    ctx = torch.zeros(B * L, H, device=DEV, dtype=torch.half)
    lse = torch.zeros(B, heads, L, device=DEV)
    K.attn_fwd(qkv, mb, ctx, lse, B, L, heads, 0.125)
    q64 = qkv.double().requires_grad_(True)
    ref, p = _attn_ref(q64, mask, B, L, heads)
    # P and O are rounded to fp16 once each: ~1e-3 relative to max|O|
    assert rel(ctx.float(), ref) < 2e-3
    x = qkv.double().view(B, L, 3, heads, 64)
    s = (x[:, :, 0].permute(0, 2, 1, 3) @ x[:, :, 1].permute(0, 2, 3, 1)) / 8.0 + (1.0 - mask.double())[:, None] * -10000.0
    assert float((lse.double() - torch.logsumexp(s, -1)).abs().max()) < 1e-3
    # backward
    dctx = h16(B * L, H, gen=gen)
    dqkv = torch.zeros(B * L, 3 * H, device=DEV, dtype=torch.half)
    delta = torch.zeros(B, heads, L, device=DEV)
    K.attn_bwd(qkv, mb, mt, ctx, dctx, lse, dqkv, delta, B, L, heads, 0.125)
    ref.backward(dctx.double())
    g = q64.grad
    for i, name in enumerate(("dq", "dk", "dv")):
        a = dqkv.view(B * L, 3, H)[:, i].float()
        r = g.view(B * L, 3, H)[:, i]
        assert rel(a, r) < 4e-3, name
    # dead-block skipping (blocks whose probabilities are exactly zero under the mask) must not change a single bit, with and
    # without dropout: the same calls with VLP_ATTN_SKIP=0 (read at every launch)
    import os
    for pdrop in (0.0, 0.2):
        outs = []
        for flag in ("1", "0"):
            os.environ["VLP_ATTN_SKIP"] = flag
            try:
                c2, l2 = torch.zeros_like(ctx), torch.zeros_like(lse)
                d2, dl2 = torch.zeros_like(dqkv), torch.zeros_like(delta)
                K.attn_fwd(qkv, mb, c2, l2, B, L, heads, 0.125, dropout_p=pdrop, seed=11, rng_stream=3)
                K.attn_bwd(qkv, mb, mt, c2, dctx, l2, d2, dl2, B, L, heads, 0.125, dropout_p=pdrop, seed=11, rng_stream=3)
                outs.append((c2, l2, d2, dl2))
            finally:
                os.environ.pop("VLP_ATTN_SKIP", None)
        for x, y in zip(*outs):
            assert torch.equal(x, y)
    # the one-kernel backward (default) against the two-kernel form it replaces (VLP_ATTN_BWD=split): dV is accumulated in the same
    # orientation and order from the same probabilities -> bit-identical; dK and dQ see delta = rowsum(dO * O) summed in another lane
    # order, and dQ comes from dS^T blocks produced by the key-owner orientation: equal up to fp16 rounding
    for pdrop in (0.0, 0.2):
        outs = []
        if not LAB:             # the two-kernel / exchange-tile forms are investigation kernels (-DVLP_LAB_BUILD); the product library says so
            os.environ["VLP_ATTN_BWD"] = "split"
            try:
                with pytest.raises(RuntimeError, match="VLP_LAB_BUILD"):
                    K.attn_bwd(qkv, mb, mt, ctx, dctx, lse, torch.zeros_like(dqkv), torch.zeros_like(delta), B, L, heads, 0.125)
            finally:
                os.environ.pop("VLP_ATTN_BWD", None)
        for mode in (("one", "split", "xch") if LAB else ("one", "one", "one")):         # default (whole dS^T in LDS at L <= 192) | two kernels | exchange-tile form
            os.environ["VLP_ATTN_BWD"] = mode
            try:
                c2, l2 = torch.zeros_like(ctx), torch.zeros_like(lse)
                d2, dl2 = torch.zeros_like(dqkv), torch.zeros_like(delta)
                K.attn_fwd(qkv, mb, c2, l2, B, L, heads, 0.125, dropout_p=pdrop, seed=11, rng_stream=3)
                K.attn_bwd(qkv, mb, mt, c2, dctx, l2, d2, dl2, B, L, heads, 0.125, dropout_p=pdrop, seed=11, rng_stream=3)
                outs.append(d2.view(B * L, 3, H))
            finally:
                os.environ.pop("VLP_ATTN_BWD", None)
        assert torch.equal(outs[0][:, 2], outs[1][:, 2])                                   # dV: same probabilities, same order
        assert rel(outs[0][:, 1].float(), outs[1][:, 1].float()) < 2e-3                     # dK: delta is summed in another lane order
        assert rel(outs[0][:, 0].float(), outs[1][:, 0].float()) < 2e-3
        assert torch.equal(outs[0], outs[2])                                                # the two one-kernel forms: same chains everywhere
        # the default kernel is PERSISTENT (one workgroup per CU walks several (batch, head) items, the next item's Q / dO prefetched into
        # registers): with 5 workgroups every one of them walks several items here; one workgroup per item (grid 0) must give the same bits
        for cap in ("5", "0"):
            os.environ["VLP_ATTN_BWD_GRID"] = cap
            try:
                c2, l2 = torch.zeros_like(ctx), torch.zeros_like(lse)
                d2, dl2 = torch.zeros_like(dqkv), torch.zeros_like(delta)
                K.attn_fwd(qkv, mb, c2, l2, B, L, heads, 0.125, dropout_p=pdrop, seed=11, rng_stream=3)
                K.attn_bwd(qkv, mb, mt, c2, dctx, l2, d2, dl2, B, L, heads, 0.125, dropout_p=pdrop, seed=11, rng_stream=3)
                assert torch.equal(d2.view(B * L, 3, H), outs[0]), cap
            finally:
                os.environ.pop("VLP_ATTN_BWD_GRID", None)


def test_attention_dropout_exact_mask(gen):
    B, L, Nv, heads, p, seed, stream = 2, 123, 100, 3, 0.25, 7, 11
    H = heads * 64
    gc = torch.Generator().manual_seed(6)
    qkv = h16(B * L, 3 * H, gen=gen)
    mask = _mask(B, L, Nv, gc).to(DEV)
    Lp = (L + 31) // 32 * 32
    mb = torch.empty(B, L, Lp, device=DEV, dtype=torch.uint8)
    mt = torch.empty(B, Lp, Lp, device=DEV, dtype=torch.uint8)
    K.mask_pack(mask, mb, B, L, Lp, out_t=mt)
    ctx = torch.zeros(B * L, H, device=DEV, dtype=torch.half)
    lse = torch.zeros(B, heads, L, device=DEV)
    K.attn_fwd(qkv, mb, ctx, lse, B, L, heads, 0.125, dropout_p=p, seed=seed, rng_stream=stream)
    # element = (row (b*heads + h)*L + q, col key)
    mult = drop_mult_ref(p, seed, stream, range(B * heads * L), range(L)).view(B, heads, L, L).double()
    q64 = qkv.double().requires_grad_(True)
    ref, _ = _attn_ref(q64, mask, B, L, heads, mult)
    assert rel(ctx.float(), ref) < 2e-3
    dctx = h16(B * L, H, gen=gen)
    dqkv = torch.zeros(B * L, 3 * H, device=DEV, dtype=torch.half)
    delta = torch.zeros(B, heads, L, device=DEV)
    K.attn_bwd(qkv, mb, mt, ctx, dctx, lse, dqkv, delta, B, L, heads, 0.125, dropout_p=p, seed=seed, rng_stream=stream)
    ref.backward(dctx.double())
    assert rel(dqkv.float(), q64.grad) < 5e-3


@pytest.mark.parametrize("L,Nv", [(167, 100), (50, 30), (100, 36), (223, 100)])
def test_attention_forward_dropout_decisions(L, Nv, gen):
    """EVERY keep / drop decision of the forward, not a tolerance: V is one-hot over a window of 64 keys (zero elsewhere), so the context row
    of a query IS its dropped, normalised probability row over that window -- an entry is exactly 0 iff it was dropped (attended
    probabilities are >> the fp16 underflow).  Compared with the Python mirror of the hash (16-bit half < threshold = dropped)."""
    B, heads, p, seed, stream = 3, 2, 0.25, 21, 5
    H = heads * 64
    gc = torch.Generator().manual_seed(8)
    mask = _mask(B, L, Nv, gc).to(DEV)
    Lp = (L + 31) // 32 * 32
    mb = torch.empty(B, L, Lp, device=DEV, dtype=torch.uint8)
    K.mask_pack(mask, mb, B, L, Lp)
    keep_ref = drop_mult_ref(p, seed, stream, range(B * heads * L), range(L)).view(B, heads, L, L) > 0
    qkv = h16(B * L, 3 * H, scale=0.25, gen=gen)               # small scores: attended probabilities stay near 1 / (attended keys)
    checked = 0
    for k0 in range(0, L, 64):
        kw = min(64, L - k0)
        v = torch.zeros(B, L, heads, 64, device=DEV, dtype=torch.half)
        for j in range(kw):
            v[:, k0 + j, :, j] = 1.0
        qkv.view(B, L, 3, heads, 64)[:, :, 2] = v
        ctx = torch.zeros(B * L, H, device=DEV, dtype=torch.half)
        lse = torch.zeros(B, heads, L, device=DEV)
        K.attn_fwd(qkv, mb, ctx, lse, B, L, heads, 0.125, dropout_p=p, seed=seed, rng_stream=stream)
        got = ctx.view(B, L, heads, 64).permute(0, 2, 1, 3)[..., :kw] != 0            # [B, heads, q, key in window]
        # attended keys carry a probability; a query row with NO attended key (padding rows) is uniform over all L keys, as in the reference
        rowlive = (mask != 0).any(-1)                                                  # [B, L]
        att = ((mask[:, :, k0:k0 + kw] != 0) | ~rowlive[:, :, None])[:, None].expand(B, heads, L, kw)
        want = keep_ref[..., k0:k0 + kw] & att
        assert torch.equal(got, want), "window at key %d: %d decisions differ" % (k0, int((got != want).sum()))       # (masked keys of a live row: exactly 0)
        checked += int(att.sum())
    assert checked > B * heads * L * 8


@pytest.mark.parametrize("L,Nv", [(167, 100), (50, 30), (100, 36)])
def test_attention_backward_dropout_decisions(L, Nv, gen):
    """The backward recomputes the forward's dropout: with dO one-hot over a window of 64 queries, dV[key, j] = Pd[query q0 + j, key], so the
    zero pattern of dV is the backward's keep / drop decision per (query, key) -- compared with the mirror of the hash, exactly."""
    B, heads, p, seed, stream = 2, 2, 0.25, 33, 2
    H = heads * 64
    gc = torch.Generator().manual_seed(9)
    mask = _mask(B, L, Nv, gc).to(DEV)
    Lp = (L + 31) // 32 * 32
    mb = torch.empty(B, L, Lp, device=DEV, dtype=torch.uint8)
    mt = torch.empty(B, Lp, Lp, device=DEV, dtype=torch.uint8)
    K.mask_pack(mask, mb, B, L, Lp, out_t=mt)
    keep_ref = drop_mult_ref(p, seed, stream, range(B * heads * L), range(L)).view(B, heads, L, L) > 0
    qkv = h16(B * L, 3 * H, scale=0.25, gen=gen)
    ctx = torch.zeros(B * L, H, device=DEV, dtype=torch.half)
    lse = torch.zeros(B, heads, L, device=DEV)
    K.attn_fwd(qkv, mb, ctx, lse, B, L, heads, 0.125, dropout_p=p, seed=seed, rng_stream=stream)
    rowlive = (mask != 0).any(-1)
    carries = ((mask != 0) | ~rowlive[:, :, None])[:, None].expand(B, heads, L, L)      # (query, key) pairs with a non-zero probability
    for q0 in range(0, L, 64):
        qw = min(64, L - q0)
        dctx = torch.zeros(B, L, heads, 64, device=DEV, dtype=torch.half)
        for j in range(qw):
            dctx[:, q0 + j, :, j] = 1.0
        dqkv = torch.zeros(B * L, 3 * H, device=DEV, dtype=torch.half)
        delta = torch.zeros(B, heads, L, device=DEV)
        K.attn_bwd(qkv, mb, mt, ctx, dctx.view(B * L, H), lse, dqkv, delta, B, L, heads, 0.125, dropout_p=p, seed=seed, rng_stream=stream)
        dv = dqkv.view(B, L, 3, heads, 64)[:, :, 2]                                      # [B, key, heads, j]
        got = (dv != 0).permute(0, 2, 3, 1)[:, :, :qw]                                   # [B, heads, query q0 + j, key]
        want = (keep_ref & carries)[:, :, q0:q0 + qw]
        assert torch.equal(got, want), "query window at %d: %d decisions differ" % (q0, int((got != want).sum()))


# =====================================================================================================
# layernorm
# =====================================================================================================
@pytest.mark.parametrize("M,H", [(5, 768), (1000, 768), (300, 2048), (64, 64), (129, 1032), (77, 520)])
def test_layernorm_fwd_bwd(M, H, gen):
    x, gamma, beta = h16(M, H, scale=2.0, gen=gen), (1 + 0.1 * torch.randn(H, device=DEV, generator=gen)).half(), h16(H, scale=0.1, gen=gen)
    y = torch.empty_like(x)
    mean, rstd = torch.empty(M, device=DEV), torch.empty(M, device=DEV)
    K.layernorm_fwd(x, gamma, beta, y, M, H, mean, rstd)
    x64 = x.double().requires_grad_(True)
    g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    ref = O.layer_norm(x64, g64, b64)
    assert rel(y.float(), ref) < 1.5e-3
    dy = h16(M, H, gen=gen)
    dx, dg, db = torch.empty_like(x), torch.zeros(H, device=DEV, dtype=torch.half), torch.zeros(H, device=DEV, dtype=torch.half)
    ws = torch.empty(K.layernorm_bwd_workspace_bytes(H), device=DEV, dtype=torch.uint8)
    K.layernorm_bwd(dy, x, gamma, mean, rstd, dx, dg, db, M, H, ws)
    ref.backward(dy.double())
    assert rel(dx.float(), x64.grad) < 2e-3
    assert rel(dg.float(), g64.grad) < 3e-3 and rel(db.float(), b64.grad) < 3e-3
    K.layernorm_bwd(dy, x, gamma, mean, rstd, dx, dg, db, M, H, ws, beta=1)
    assert rel(dg.float(), 2 * g64.grad) < 4e-3


@pytest.mark.parametrize("M,H", [(33, 4096), (10, 2056)])
def test_layernorm_fwd_wide(M, H, gen):
    """forward only: H up to 4096 (16 four-column pieces per lane); the backward stops at 2048"""
    x, gamma, beta = h16(M, H, scale=2.0, gen=gen), (1 + 0.1 * torch.randn(H, device=DEV, generator=gen)).half(), h16(H, scale=0.1, gen=gen)
    y = torch.empty_like(x)
    mean, rstd = torch.empty(M, device=DEV), torch.empty(M, device=DEV)
    K.layernorm_fwd(x, gamma, beta, y, M, H, mean, rstd)
    ref = O.layer_norm(x.double(), gamma.double(), beta.double())
    assert rel(y.float(), ref) < 1.5e-3
    assert rel(mean, x.double().mean(1)) < 1e-5


@pytest.mark.parametrize("M,H", [(1000, 768), (37, 768), (4000, 1024)])
def test_layernorm_bwd_deferred_batched_reduce(M, H, gen):
    """defer_reduce leaves dgamma / dbeta untouched and the per-block partials in the caller's slot; ONE batched launch then writes
    every LayerNorm's dgamma / dbeta -- bit-identical to the immediate second stage (same summation order), beta = 0 and 1."""
    n = 3
    slot = K.layernorm_bwd_workspace_bytes(H)
    slots = torch.empty(n * slot, device=DEV, dtype=torch.uint8)
    ws = torch.empty(slot, device=DEV, dtype=torch.uint8)
    want, dst, keep = [], [], []
    for i in range(n):
        x, gamma = h16(M, H, scale=2.0, gen=gen), (1 + 0.1 * torch.randn(H, device=DEV, generator=gen)).half()
        y = torch.empty_like(x)
        mean, rstd = torch.empty(M, device=DEV), torch.empty(M, device=DEV)
        K.layernorm_fwd(x, gamma, torch.zeros(H, device=DEV).half(), y, M, H, mean, rstd)
        dy = h16(M, H, gen=gen)
        dx0, dx1 = torch.empty_like(x), torch.empty_like(x)
        g0, b0 = h16(H, gen=gen), h16(H, gen=gen)                 # pre-existing gradient content (beta = 1 accumulates onto it)
        g1, b1 = g0.clone(), b0.clone()
        for beta, gg, bb in ((1, g0, b0),):
            K.layernorm_bwd(dy, x, gamma, mean, rstd, dx0, gg, bb, M, H, ws, beta=beta)
        K.layernorm_bwd(dy, x, gamma, mean, rstd, dx1, g1, b1, M, H, slots[i * slot:(i + 1) * slot], beta=1, defer_reduce=True)
        assert torch.equal(dx0, dx1)
        assert not torch.equal(g1, g0)                            # untouched so far
        want.append((g0, b0))
        dst.append([g1.data_ptr(), b1.data_ptr()])
        keep.append((g1, b1))
    table = torch.tensor(dst, dtype=torch.int64, device=DEV)
    K.layernorm_bwd_reduce_batched(slots, table, n, M, H, beta=1)
    for (g0, b0), (g1, b1) in zip(want, keep):
        assert torch.equal(g0, g1) and torch.equal(b0, b1)


def test_layernorm_dropout_paths(gen):
    M, H, p = 257, 768, 0.2
    x, gamma, beta = h16(M, H, gen=gen), torch.ones(H, device=DEV).half(), torch.zeros(H, device=DEV).half()
    y = torch.empty_like(x)
    mean, rstd = torch.empty(M, device=DEV), torch.empty(M, device=DEV)
    K.layernorm_fwd(x, gamma, beta, y, M, H, mean, rstd, dropout_p=p, seed=3, rng_stream=9)
    mult = drop_mult_ref(p, 3, 9, range(M), range(H))
    ref = O.layer_norm(x.float(), gamma.float(), beta.float())
    assert rel(y.float(), ref * mult) < 1.5e-3
    # backward: incoming dy passes through the same mask; second output = dx * (another mask)
    dy = h16(M, H, gen=gen)
    dx, dxd = torch.empty_like(x), torch.empty_like(x)
    dg, db = torch.zeros(H, device=DEV, dtype=torch.half), torch.zeros(H, device=DEV, dtype=torch.half)
    ws = torch.empty(K.layernorm_bwd_workspace_bytes(H), device=DEV, dtype=torch.uint8)
    K.layernorm_bwd(dy, x, gamma, mean, rstd, dx, dg, db, M, H, ws, dx_drop=dxd, dy_drop=(p, 3, 9), out_drop=(0.1, 4, 2))
    x64 = x.double().requires_grad_(True)
    (O.layer_norm(x64, gamma.double(), beta.double()) * mult.double()).backward(dy.double())
    assert rel(dx.float(), x64.grad) < 2e-3
    assert rel(dxd.float(), x64.grad * drop_mult_ref(0.1, 4, 2, range(M), range(H))) < 2e-3


# =====================================================================================================
# embeddings / data movement
# =====================================================================================================
def test_embed_fwd_bwd(gen):
    B, L, Nv, H, V, T, P = 3, 43, 8, 768, 500, 6, 64
    ids = torch.randint(0, V, (B, L), device=DEV, generator=gen)
    ids[0, -3:] = 0
    seg = torch.randint(0, T, (B, L), device=DEV, generator=gen)
    word, pos, typ = h16(V, H, gen=gen), h16(P, H, gen=gen), h16(T, H, gen=gen)
    vis, vpe = torch.relu(h16(B * Nv, H, gen=gen)), torch.relu(h16(B * Nv, H, gen=gen))
    pre = torch.empty(B * L, H, device=DEV, dtype=torch.half)
    K.embed_fwd(ids, seg, word, pos, typ, vis, vpe, pre, B, L, Nv, H)
    p = {"bert.embeddings.word_embeddings.weight": word.double().requires_grad_(True),
         "bert.embeddings.position_embeddings.weight": pos.double().requires_grad_(True),
         "bert.embeddings.token_type_embeddings.weight": typ.double().requires_grad_(True),
         "bert.embeddings.LayerNorm.weight": torch.ones(H, device=DEV).double(), "bert.embeddings.LayerNorm.bias": torch.zeros(H, device=DEV).double()}
    v64, vp64 = vis.double().view(B, Nv, H).requires_grad_(True), vpe.double().view(B, Nv, H).requires_grad_(True)
    # the oracle's arange for position ids lives on the CPU: build it on the device here
    _, ref_pre = O.embeddings(p, v64, vp64, ids, seg, Nv, position_ids=torch.arange(L, device=DEV).unsqueeze(0).expand(B, L))
    assert rel(pre.float(), ref_pre.reshape(B * L, H)) < 1e-3
    dpre = h16(B * L, H, gen=gen)
    dpre.view(B, L, H)[0, -3:] = 0      # padding rows carry exactly zero gradient
    dw, dp_, dt = torch.zeros_like(word), torch.zeros_like(pos), torch.zeros_like(typ)
    dv, dvp = torch.empty_like(vis), torch.empty_like(vpe)
    acc = torch.empty(K.embed_bwd_workspace_floats(B, L, Nv, H), device=DEV)
    K.embed_bwd(dpre, ids, seg, vis, vpe, dw, dp_, dt, dv, dvp, acc, B, L, Nv, H, V, T)
    ref_pre.backward(dpre.double().view(B, L, H))
    assert rel(dw.float(), p["bert.embeddings.word_embeddings.weight"].grad) < 3e-3
    assert rel(dp_.float(), p["bert.embeddings.position_embeddings.weight"].grad) < 3e-3
    assert rel(dt.float(), p["bert.embeddings.token_type_embeddings.weight"].grad) < 3e-3
    # region rows: gradient gated by (y > 0) (ReLU'; no dropout here)
    assert rel(dv.float(), (v64.grad * (v64 > 0)).reshape(B * Nv, H)) < 1e-3
    assert rel(dvp.float(), (vp64.grad * (vp64 > 0)).reshape(B * Nv, H)) < 1e-3


@pytest.mark.parametrize("B,L,Nv,V", [(8, 150, 100, 3), (64, 167, 100, 40), (2, 30, 0, 5)])
def test_embed_word_grad_long_chains_deterministic(B, L, Nv, V, gen):
    """Word-embedding gradient with heavily repeated ids (chains of hundreds of rows, as the [PAD] rows of a real batch): fixed-order
    fp32 sums by one owner per id -- matches an fp64 index_add to fp16 rounding, adds onto what the buffer holds, and is bitwise
    reproducible."""
    H, T = 768, 6
    ids = torch.randint(0, V, (B, L), device=DEV, generator=gen)
    seg = torch.zeros(B, L, dtype=torch.long, device=DEV)
    dpre = h16(B * L, H, gen=gen)
    vis = vpe = torch.relu(h16(max(B * Nv, 1), H, gen=gen))
    base = h16(V, H, scale=0.5, gen=gen)
    outs = []
    for rep in range(2):
        dw, dp_, dt = base.clone(), torch.zeros(256, H, device=DEV, dtype=torch.half), torch.zeros(T, H, device=DEV, dtype=torch.half)
        dv, dvp = torch.empty_like(vis), torch.empty_like(vpe)
        acc = torch.full((K.embed_bwd_workspace_floats(B, L, Nv, H),), float("nan"), device=DEV)      # scratch content must not matter
        K.embed_bwd(dpre, ids, seg, vis if Nv else None, vpe if Nv else None, dw, dp_, dt, dv if Nv else None, dvp if Nv else None, acc,
                    B, L, Nv, H, V, T)
        outs.append(dw)
    assert torch.equal(outs[0], outs[1])
    tok = torch.ones(L, dtype=torch.bool, device=DEV)
    tok[1:Nv + 1] = False
    ref = base.double().index_add(0, ids[:, tok].reshape(-1), dpre.view(B, L, H)[:, tok].reshape(-1, H).double())
    err = (outs[0].double() - ref).abs()
    assert float((err / (ref.abs() + 1.0)).max()) < 1e-3, float(err.max())


def test_copy2d_transpose_gather_scatter(gen):
    src = torch.randn(50, 1607, device=DEV, generator=gen)
    dst = torch.full((50, 1664), 9.0, device=DEV, dtype=torch.half)
    K.copy2d(src, 1607, True, dst, 1664, 50, 1607, 1664)
    assert torch.equal(dst[:, :1607], src.half()) and float(dst[:, 1607:].abs().max()) == 0
    s16 = src.half()
    K.copy2d(s16, 1607, False, dst, 1664, 50, 1607, 1664, beta=1)
    assert rel(dst[:, :1607].float(), 2 * src) < 1e-3
    w = h16(300, 200, gen=gen)
    wt = torch.full((200, 320), 5.0, device=DEV, dtype=torch.half)
    K.transpose(w, 200, wt, 320, 300, 200, 320)
    assert torch.equal(wt[:, :300], w.t()) and float(wt[:, 300:].abs().max()) == 0
    # batched form: several shapes (ragged, padded) in one launch
    mats = [h16(300, 200, gen=gen), h16(768, 2304, gen=gen), h16(1000, 64, gen=gen), h16(5, 3129 + 7, gen=gen)[:, :3128]]
    items, outs = [], []
    for m_ in mats:
        r_, c_ = m_.shape
        rp = (r_ + 63) // 64 * 64
        o_ = torch.full((c_, rp), 3.0, device=DEV, dtype=torch.half)
        items.append((m_, m_.stride(0), o_, rp, r_, c_, rp))
        outs.append(o_)
    K.transpose_batched(K.make_transpose_batch(items, DEV))
    for m_, o_ in zip(mats, outs):
        assert torch.equal(o_[:, :m_.shape[0]], m_.t()) and float(o_[:, m_.shape[0]:].abs().max() if o_.shape[1] > m_.shape[0] else 0) == 0
    B, P, L, H = 4, 3, 20, 64
    h = h16(B * L, H, gen=gen)
    pos = torch.randint(0, L, (B, P), device=DEV, generator=gen)
    out = torch.empty(B * P, H, device=DEV, dtype=torch.half)
    K.gather_rows(h, H, pos, out, H, B, P, L, H)
    ref = torch.gather(h.view(B, L, H), 1, pos.unsqueeze(2).expand(-1, -1, H)).reshape(B * P, H)
    assert torch.equal(out, ref)
    dh = torch.zeros(B * L, H, device=DEV, dtype=torch.half)
    K.scatter_add_rows(out, H, pos, dh, H, B, P, L, H)
    ref_d = torch.zeros(B, L, H, device=DEV).scatter_add_(1, pos.unsqueeze(2).expand(-1, -1, H), out.view(B, P, H).float())
    assert rel(dh.float(), ref_d.view(B * L, H)) < 2e-3


def test_vqa_mul_and_relu_dropout_bwd(gen):
    B, L, Nv, H = 5, 30, 10, 768
    h = h16(B * L, H, gen=gen)
    out = torch.empty(B, H, device=DEV, dtype=torch.half)
    K.vqa_mul_fwd(h, out, B, L, Nv, H)
    hv = h.view(B, L, H).float()
    assert rel(out.float(), hv[:, 0] * hv[:, Nv + 1]) < 1e-3
    dout = h16(B, H, gen=gen)
    dh = torch.zeros(B * L, H, device=DEV, dtype=torch.half)
    K.vqa_mul_bwd(h, dout, dh, B, L, Nv, H)
    d = dh.view(B, L, H).float()
    assert rel(d[:, 0], dout.float() * hv[:, Nv + 1]) < 1e-3 and rel(d[:, Nv + 1], dout.float() * hv[:, 0]) < 1e-3
    assert float(d[:, 1:Nv + 1].abs().max()) == 0
    y, dy = torch.relu(h16(40, 768, gen=gen)), h16(40, 768, gen=gen)
    dz = torch.empty_like(y)
    K.relu_dropout_bwd(dy, y, dz, y.numel(), 768, drop_p=0.3, seed=1, rng_stream=2)
    ref = dy.float() * (y > 0) * drop_mult_ref(0.3, 1, 2, range(40), range(768))
    assert rel(dz.float(), ref) < 1e-3


# =====================================================================================================
# losses
# =====================================================================================================
@pytest.mark.parametrize("ratio", [0.0, 0.3])
def test_mlm_loss(ratio, gen):
    B, P, V = 16, 3, 28996
    ld = (V + 63) // 64 * 64
    logits = torch.zeros(B * P, ld, device=DEV, dtype=torch.half)
    logits[:, :V] = h16(B * P, V, scale=2.0, gen=gen)
    labels = torch.randint(0, V, (B, P), device=DEV, generator=gen)
    weights = (torch.rand(B, P, device=DEV, generator=gen) < 0.7).long()
    weights[:, 0] = 1
    loss, lse, coef, row = torch.zeros(1, device=DEV), torch.zeros(B * P, device=DEV), torch.zeros(B * P, device=DEV), torch.zeros(B * P, device=DEV)
    K.mlm_loss_fwd(logits, ld, labels, weights, loss, lse, coef, row, B, P, V, drop_worst_ratio=ratio)
    x = logits[:, :V].float().view(B, P, V).requires_grad_(True)
    ce = torch.nn.functional.cross_entropy(x.transpose(1, 2), labels, reduction="none")
    ref = O.loss_mask_and_normalize(ce, weights, ratio)
    assert abs(float(loss) - float(ref)) < 1e-4 * abs(float(ref))
    gs = torch.full((1,), 128.0, device=DEV)
    dl = torch.full((B * P, ld), 3.0, device=DEV, dtype=torch.half)
    K.mlm_loss_bwd(logits, ld, labels, lse, coef, gs, dl, ld, B * P, V)
    (ref * 128.0).backward()
    assert rel(dl[:, :V].float(), x.grad.view(B * P, V)) < 2e-3
    assert float(dl[:, V:].abs().max()) == 0


def test_bce_loss(gen):
    B, N, ld = 7, 3129, 3136
    logits = torch.zeros(B, ld, device=DEV, dtype=torch.half)
    logits[:, :N] = h16(B, N, scale=3.0, gen=gen)
    y = torch.rand(B, N, device=DEV, generator=gen)
    loss = torch.zeros(257, device=DEV)
    K.bce_loss_fwd(logits, ld, y, N, B, N, loss)
    x = logits[:, :N].float().requires_grad_(True)
    ref = torch.nn.functional.binary_cross_entropy_with_logits(x, y) * N
    assert abs(float(loss[0]) - float(ref)) < 1e-4 * abs(float(ref))
    gs = torch.full((1,), 64.0, device=DEV)
    d = torch.full((B, ld), 2.0, device=DEV, dtype=torch.half)
    K.bce_loss_bwd(logits, ld, y, N, B, N, gs, d, ld)
    (ref * 64.0).backward()
    assert rel(d[:, :N].float(), x.grad) < 2e-3 and float(d[:, N:].abs().max()) == 0


# =====================================================================================================
# optimizers
# =====================================================================================================
def test_fused_adam_and_norm(gen):
    n = 8 * 12345
    p32 = torch.randn(n, device=DEV, generator=gen) * 0.02
    g16 = (torch.randn(n, device=DEV, generator=gen) * 300).half()      # "scaled" gradients
    m, v = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    p16 = torch.empty(n, device=DEV, dtype=torch.half)
    out2, part, hyper = torch.zeros(2, device=DEV), torch.zeros(2048, device=DEV), torch.zeros(3, device=DEV)
    scale = 1024.0
    sstate = torch.tensor([scale, 0, -1, 2, 1000, 1, 0, 0], device=DEV, dtype=torch.float32)
    rp, rm, rv = p32.cpu().clone(), m.cpu().clone(), v.cpu().clone()
    for step in range(2):
        K.sumsq(g16, n, out2, part)
        K.adam_hyper(out2, None, sstate, 1.0, 3e-5, hyper)
        K.fused_adam(p32, m, v, g16, p16, n, hyper, decay=0.01)
        norm = float(g16.float().norm())
        assert abs(math.sqrt(float(out2[0])) - norm) < 1e-4 * norm and float(out2[1]) == 0
        O.fused_adam_step(rp, g16.cpu(), rm, rv, lr=3e-5, grad_norm_scaled=norm, scale=scale, weight_decay=0.01)
    assert rel(p32.cpu(), rp) < 1e-5 and rel(m.cpu(), rm) < 1e-4 and rel(v.cpu(), rv) < 1e-4
    # the fp16 model copy is exactly half(master), as apex writes it: a resumed run rebuilds it from the master bit for bit
    assert torch.equal(p16, p32.half())
    # overflow: state must stay untouched and the flag must be raised
    g_bad = g16.clone()
    g_bad[777] = float("inf")
    before = p32.clone()
    K.sumsq(g_bad, n, out2, part)
    K.adam_hyper(out2, None, sstate, 1.0, 3e-5, hyper)
    K.fused_adam(p32, m, v, g_bad, p16, n, hyper)
    assert float(out2[1]) == 1.0 and float(hyper[2]) == 1.0 and torch.equal(before, p32)
    # device-side loss-scale bookkeeping vs the oracle's restatement of apex
    ls = O.LossScaler(dynamic=True, init_scale=scale, scale_window=3)
    sstate = torch.tensor([scale, 0, -1, 2, 3, 1, 0, 0], device=DEV, dtype=torch.float32)
    for ovf in (0, 0, 0, 1, 0, 0, 0, 0, 1, 1, 0):
        K.loss_scale_update(sstate, torch.tensor([float(ovf)], device=DEV))
        ls.update(bool(ovf))
        assert float(sstate[0]) == ls.cur_scale and int(sstate[1]) == ls.cur_iter and int(sstate[2]) == ls.last_overflow_iter


@pytest.mark.parametrize("g_is_f32", [True, False])
def test_bert_adam(g_is_f32, gen):
    sizes = [768 * 64, 768, 3072, 5000, 8, 28996]
    offs = [0]
    for s in sizes:
        offs.append(offs[-1] + s)
    n = offs[-1]
    seg = torch.tensor(offs, device=DEV, dtype=torch.int64)
    p32 = torch.randn(n, device=DEV, generator=gen) * 0.02
    g = torch.randn(n, device=DEV, generator=gen) * 0.05
    g[offs[1]:offs[2]] *= 100          # one tensor far above the clip threshold
    gk = g if g_is_f32 else g.half()
    m, v = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    norms = torch.full((K.bert_adam_norms_floats(n, len(sizes)),), float("nan"), device=DEV)     # stale scratch must not matter
    with pytest.raises(RuntimeError, match="norms"):
        K.bert_adam(p32, m, v, gk, g_is_f32, None, seg, len(sizes), n, norms[:len(sizes)], lr=1e-3)          # ABI-1 sized scratch is refused
    p16 = torch.empty(n, device=DEV, dtype=torch.half)
    rp = p32.cpu().clone()
    rm, rv = torch.zeros(n), torch.zeros(n)
    p0, m0, v0 = p32.clone(), m.clone(), v.clone()
    for step in range(2):
        lr = 1e-3 * O.warmup_linear((step + 1) / 20, 0.1)
        K.bert_adam(p32, m, v, gk, g_is_f32, p16, seg, len(sizes), n, norms, lr=lr, decay=0.01)
        for i in range(len(sizes)):
            sl = slice(offs[i], offs[i + 1])
            O.bert_adam_step(rp[sl], gk.float().cpu()[sl], rm[sl], rv[sl], 0, lr=lr, weight_decay=0.01)
    assert rel(p32.cpu(), rp) < 1e-5 and rel(m.cpu(), rm) < 1e-4
    assert rel(p16.float().cpu(), p32.cpu()) < 1e-3
    # per-tensor squared norms (clip decisions) against torch, and bitwise repeatability of the whole update (no atomics)
    want = torch.stack([gk.float()[offs[i]:offs[i + 1]].double().pow(2).sum() for i in range(len(sizes))]).float()
    assert rel(norms[:len(sizes)].cpu(), want.cpu()) < 1e-5
    runs = []
    for rep in range(3):
        a, b, c = p0.clone(), m0.clone(), v0.clone()
        nn_ = torch.zeros_like(norms)
        for step in range(2):
            K.bert_adam(a, b, c, gk, g_is_f32, None, seg, len(sizes), n, nn_, lr=1e-3, decay=0.01)
        runs.append((a, b, c, nn_[:len(sizes)].clone()))
    for r in runs[1:]:
        assert all(torch.equal(x, y) for x, y in zip(runs[0], r))


# =====================================================================================================
# mask_image_regions / vis_pretext_loss kernels (modeling.py:1049-1056, 1113-1131)
# =====================================================================================================
@pytest.mark.parametrize("B,Nv,Pm,H,p", [(3, 100, 25, 768, 0.0), (2, 100, 25, 768, 0.1), (2, 20, 5, 256, 0.1), (1, 100, 50, 768, 0.0)])
def test_pretext_fwd_bwd(B, Nv, Pm, H, p, gen):
    """vlp_pretext_fwd / vlp_pretext_bwd against the oracle's vis_pretext_loss under torch autograd (fp32 on the same fp16 inputs;
    A = vispe + pooled and the similarity matrix are rounded to fp16 in both, as the reference's half tensors are).  With p > 0 the
    gradient passes through the projections' ReLU + dropout exactly like vlp_embed_bwd does for the unmasked rows: checked against
    the python mirror of the dropout hash; rows that are not masked must stay untouched."""
    seed, s_vis, s_vpe = 77, 1001, 1002
    vis = torch.relu(h16(B * Nv, H, scale=0.15, gen=gen))
    vpe = torch.relu(h16(B * Nv, H, scale=0.15, gen=gen))
    rows, cols = list(range(B * Nv)), list(range(H))
    mv, mp = drop_mult_ref(p, seed, s_vis, rows, cols), drop_mult_ref(p, seed, s_vpe, rows, cols)
    vis, vpe = (vis.float() * mv).half(), (vpe.float() * mp).half()                 # post-ReLU, post-dropout forward outputs
    pooled = torch.tanh(h16(B, H, gen=gen).float() * 0.3).half()
    vmp = torch.stack([torch.randperm(Nv, generator=torch.Generator().manual_seed(10 + b))[:Pm] + 1 for b in range(B)]).to(DEV)
    probs = torch.empty(B, Pm, Pm, device=DEV)
    sample, loss = torch.empty(B, device=DEV), torch.empty(1, device=DEV)
    K.pretext_fwd(vis, vpe, pooled, vmp, probs, sample, loss, B, Nv, Pm, H)
    # forward reference: fp64 sums over the same rounding points (A and sim rounded to fp16, :1124, :1126).  The kernel sums in fp32, so
    # a similarity that lands within ~1e-6 relative of an fp16 rounding boundary may round the other way (1 fp16 ulp of that entry):
    # the bounds below admit a handful of such flips, nothing more
    idx = (vmp - 1).unsqueeze(-1).expand(-1, -1, H)
    Vm = torch.gather(vis.double().view(B, Nv, H), 1, idx)
    A = (torch.gather(vpe.float().view(B, Nv, H), 1, idx) + pooled.float().unsqueeze(1)).half().double()
    sim = (A @ Vm.transpose(1, 2)).half().double()
    ulp = float(sim.abs().max()) * 2.0 ** -10
    ls = torch.log_softmax(sim, dim=-1)
    ref_loss = torch.stack([-ls[b].diag().mean() for b in range(B)]).mean()
    assert abs(float(loss) - float(ref_loss)) <= 2e-6 * abs(float(ref_loss)) + 4 * ulp / (B * Pm), (float(loss), float(ref_loss), ulp)
    pd = (probs.double() - torch.softmax(sim, -1)).abs()
    assert float(pd.max()) <= 1.2 * ulp + 1e-6 and float((pd > 1e-6).double().mean()) < 0.02, (float(pd.max()), ulp)
    assert float((probs.sum(-1) - 1).abs().max()) < 1e-5
    # backward reference: the closed form on the kernel's own probabilities (isolates the backward kernel from forward flips)
    g = 4096.0
    dsim = (probs.double() - torch.eye(Pm, device=DEV, dtype=torch.double)) * (g / (B * Pm))
    dA, dV = dsim @ Vm, dsim.transpose(1, 2) @ A
    d_vis = torch.full((B * Nv, H), 3.0, device=DEV, dtype=torch.half)
    d_vpe = torch.full((B * Nv, H), 3.0, device=DEV, dtype=torch.half)
    dpool = torch.empty(B, H, device=DEV, dtype=torch.half)
    K.pretext_bwd(vis, vpe, pooled, vmp, probs, torch.full((1,), g, device=DEV), d_vis, d_vpe, dpool, B, Nv, Pm, H, drop_p=p, seed=seed,
                  vis_stream=s_vis, vispe_stream=s_vpe)
    masked = torch.zeros(B, Nv, dtype=torch.bool, device=DEV)
    masked.scatter_(1, vmp - 1, True)
    masked = masked.view(-1)
    assert float((d_vis[~masked].float() - 3.0).abs().max()) == 0.0 and float((d_vpe[~masked].float() - 3.0).abs().max()) == 0.0
    full_v = torch.zeros(B, Nv, H, device=DEV, dtype=torch.double).scatter_(1, idx, dV).view(B * Nv, H)
    full_e = torch.zeros(B, Nv, H, device=DEV, dtype=torch.double).scatter_(1, idx, dA).view(B * Nv, H)
    want_v = (full_v * (vis.float() > 0) * mv)[masked]
    want_e = (full_e * (vpe.float() > 0) * mp)[masked]
    assert rel(d_vis[masked].float(), want_v) < 1e-3                                # fp16 output rounding only
    assert rel(d_vpe[masked].float(), want_e) < 1e-3
    want_pool = dA.sum(1) * (1.0 - pooled.double() ** 2)
    assert rel(dpool.float(), want_pool) < 1e-3
    # and the closed form IS the gradient: torch autograd of the oracle's loss (fp32, straight-through fp16 roundings) agrees
    v32 = vis.float().view(B, Nv, H).clone().requires_grad_(True)
    e32 = vpe.float().view(B, Nv, H).clone().requires_grad_(True)
    q32 = pooled.float().clone().requires_grad_(True)
    A32 = torch.gather(e32, 1, idx) + q32.unsqueeze(1)
    A32 = A32 + (A32.half().float() - A32).detach()
    s32 = A32 @ torch.gather(v32, 1, idx).transpose(1, 2)
    s32 = s32 + (s32.half().float() - s32).detach()
    l32 = torch.log_softmax(s32, dim=-1)
    (torch.stack([-l32[b].diag().mean() for b in range(B)]).mean() * g).backward()
    assert rel((v32.grad.view(B * Nv, H) * (vis.float() > 0) * mv)[masked], want_v) < 0.1 * (1 + 20 * ulp)      # loose: forward flips allowed
    assert rel(q32.grad * (1.0 - pooled.float() ** 2), want_pool) < 0.1 * (1 + 20 * ulp)
    # bitwise reproducible
    d2, e2, p2 = torch.empty_like(d_vis), torch.empty_like(d_vpe), torch.empty_like(dpool)
    K.pretext_bwd(vis, vpe, pooled, vmp, probs, torch.full((1,), g, device=DEV), d2, e2, p2, B, Nv, Pm, H, drop_p=p, seed=seed,
                  vis_stream=s_vis, vispe_stream=s_vpe)
    assert torch.equal(d2[masked], d_vis[masked]) and torch.equal(e2[masked], d_vpe[masked]) and torch.equal(p2, dpool)
    with pytest.raises(RuntimeError):
        K.pretext_fwd(vis, vpe, pooled, vmp, probs, sample, loss, B, Nv, 65, H)       # more masked regions than a wave has lanes: refused


def test_device_guard_multi_device_path():
    """under torchrun every rank sees all 8 GPUs, so every launch goes through the multi-device branch of the entry
    guard.  A 1-GPU box cannot switch devices, but it can run that branch: VLP_FAKE_DEVICE_COUNT=2 makes the guard resolve the owner of
    every operand and compare it with hipGetDevice().  Checked in a child process (the count is read once): results are correct, the
    driver is asked once per ALLOCATION and not once per launch (the owner cache), the caller's current device is what it was, and a
    host pointer is still refused."""
    import os
    import subprocess
    import sys
    code = r"""
import ctypes, torch
from vlp_amd import _lib as K
dev = torch.device('cuda:0')
x = torch.randn(256, 128, device=dev).half(); w = torch.randn(128, 128, device=dev).half(); y = torch.empty(256, 128, device=dev, dtype=torch.half)
for _ in range(200):
    K.gemm_nt(x, w, y, 256, 128, 128)
torch.cuda.synchronize()
assert float((y.float() - x.float() @ w.float().t()).abs().max()) < 0.25
lk, q = ctypes.c_ulonglong(), ctypes.c_ulonglong()
K.load().vlp_debug_device_lookup_stats(ctypes.byref(lk), ctypes.byref(q))
assert lk.value >= 200 and q.value <= 8, (lk.value, q.value)
assert torch.cuda.current_device() == 0
host = torch.zeros(256, 128, dtype=torch.half).pin_memory()
a = K.GemmNtArgs(host.data_ptr(), 128, w.data_ptr(), 128, y.data_ptr(), 128, None, None, 0, None, 0, None, 0, 256, 128, 128, 0, 0, 1.0, 0.0, 0, 0, 0)
rc = K.load().vlp_gemm_nt(ctypes.byref(a), None)
assert rc != 0 and b'host memory' in K.load().vlp_last_error_string(), (rc, K.load().vlp_last_error_string())
print('GUARD_OK', lk.value, q.value)
"""
    env = dict(os.environ, VLP_FAKE_DEVICE_COUNT="2")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=root, timeout=300)
    assert "GUARD_OK" in r.stdout, r.stdout + r.stderr
