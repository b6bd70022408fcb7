"""The figures that tests/test_06_kernel_hard_values_gpu.py quotes beside its bounds, asserted: fp32 restatements of the ops with the
kernels' documented rounding points (tests/hard_inputs.py) against fp64 on exactly the hard inputs of test_06.  The bounds of test_06 are
the existing ones of test_00, or twice a figure pinned here; none is read off a kernel.  Needs neither a GPU nor the built library."""
import torch

from oracle import vlp_oracle as O
from tests.hard_inputs import (attn_hard_qkv, attn_mask, attn_ref, attn_restatement_fp32, ce_hard_rows, ce_rows_restatement_fp32,
                               layernorm_restatement_fp32, ln_hard_rows, pretext_sim_restatement_fp32, pretext_sim_window, rel)

# what test_06 allows is 2 x these (attention), measured with this restatement on these inputs; the assertions below leave 5 % for another
# BLAS summing in another order
ATTN_MEASURED = {"ctx": 4.38e-4, "lse_low_head": 6.63e-4, "lse_other_heads": 2.80e-5, "dq": 1.52e-3, "dk": 1.15e-3, "dv": 4.40e-4}


def test_layernorm_two_pass_is_inside_the_bound_and_single_pass_is_not():
    for H in (768, 1032):
        x, kind = ln_hard_rows(257, H)
        g = torch.Generator().manual_seed(1)
        gamma, beta = (1 + 0.1 * torch.randn(H, generator=g)).half(), (0.1 * torch.randn(H, generator=g)).half()
        ref = O.layer_norm(x.double(), gamma.double(), beta.double())
        y2, mean, rstd = layernorm_restatement_fp32(x, gamma, beta)
        y1, _, _ = layernorm_restatement_fp32(x, gamma, beta, two_pass=False)
        want_rstd = 1.0 / torch.sqrt(x.double().var(1, unbiased=False) + 1e-5)
        absmean = x.double().abs().mean(1)
        for kd in range(5):
            m = kind == kd
            assert rel(y2[m].float(), ref[m]) < 5e-4, (H, kd)                     # test_06 allows 1.5e-3: a factor 3 in hand
            assert rel(rstd[m], want_rstd[m]) < 1e-6, (H, kd)                      # test_06 allows 1e-5
            assert bool(((mean[m].double() - x[m].double().mean(1)).abs() <= absmean[m] * 2.0 ** -23 * 16).all()), (H, kd)
        for kd in (1, 2):                                                          # the offset rows separate the two by an order of magnitude
            m = kind == kd
            assert rel(y1[m].float(), ref[m]) > 1.5e-2, (H, kd)


def test_cross_entropy_rows_restatement():
    xs, lab = ce_hard_rows(28996)
    lse, row = ce_rows_restatement_fp32(xs, lab)
    row64 = torch.logsumexp(xs.double(), -1) - xs.double().gather(1, lab[:, None])[:, 0]
    assert abs(float(row64[0]) - 1.2e5) < 1 and float(row64[2]) > 1.3e5 and float(row64[3]) > 1e4
    assert float(((row.double() - row64).abs() / row64.abs()).max()) < 1e-6          # test_06 allows 1e-4
    assert float(((lse.double() - torch.logsumexp(xs.double(), -1)).abs() / torch.logsumexp(xs.double(), -1).abs().clamp_min(1.0)).max()) < 1e-6


def test_attention_restatement_figures():
    B, L, heads, Nv, low = 2, 167, 12, 100, 3
    H = heads * 64
    qkv = attn_hard_qkv(B, L, heads, low)
    mask = attn_mask(B, L, Nv, torch.Generator().manual_seed(5))
    dctx = torch.randn(B * L, H, generator=torch.Generator().manual_seed(14)).half()
    ctx, lse, dqkv = attn_restatement_fp32(qkv, mask, dctx, B, L, heads)
    q64 = qkv.double().requires_grad_(True)
    ref, _ = attn_ref(q64, mask, B, L, heads)
    ref.backward(dctx.double())
    x = qkv.double().view(B, L, 3, heads, 64)
    s = (x[:, :, 0].permute(0, 2, 1, 3) @ x[:, :, 1].permute(0, 2, 3, 1)) / 8.0 + (1.0 - mask.double())[:, None] * -10000.0
    assert float(s[:, low].max()) < -2000
    d = (lse.double() - torch.logsumexp(s, -1)).abs()
    got = {"ctx": rel(ctx.float(), ref.detach()), "lse_low_head": float(d[:, low].max()),
           "lse_other_heads": float(d[:, [h for h in range(heads) if h != low]].max())}
    for i, n in enumerate(("dq", "dk", "dv")):
        got[n] = rel(dqkv[:, i * H:(i + 1) * H].float(), q64.grad[:, i * H:(i + 1) * H])
    for k, v in ATTN_MEASURED.items():
        assert got[k] <= 1.05 * v, (k, got[k], v)
        assert got[k] >= 0.5 * v, (k, got[k], v)             # and the quoted figure is not an overstatement that would loosen test_06


def test_pretext_sim_rounding_window():
    """tests/test_07_step_kernel_contract_gpu.py::test_pretext_guarded lets an entry of the fp16 similarity matrix round either way only
    inside pretext_sim_window's window.  Here the kernel's own summation order in fp32 (pretext_sim_restatement_fp32) against fp64 on
    inputs drawn like the test's: a differing entry always lies inside the window and is one fp16 ulp off.  The window is a worst-case
    bound: it holds a few percent of the ENTRIES, but at Pm = 63 / 64 that is an entry in 40 .. 90 % of the ROWS, so the window does not by
    itself pin most rows of `probs`.  That is why test_pretext_guarded also caps the number of rows that moved at four: the summation
    order of the kernel flips no more than that here (none on these inputs)."""
    for H, Pm, rows_lo, rows_hi in ((64, 63, 0.2, 0.6), (520, 63, 0.7, 1.0), (768, 64, 0.5, 0.9)):
        g = torch.Generator().manual_seed(21 + H)
        V = torch.relu(0.15 * torch.randn(Pm, H, generator=g)).half()
        A = (torch.relu(0.15 * torch.randn(Pm, H, generator=g)).half().float() + torch.tanh(0.3 * torch.randn(H, generator=g)).half().float()).half()
        s64, amb = pretext_sim_window(A, V, H)
        got, want = pretext_sim_restatement_fp32(A, V), s64.half()
        flips = got != want
        assert not bool((flips & ~amb).any()), (H, Pm, int((flips & ~amb).sum()))
        assert bool(((got.double() - want.double()).abs() <= want.double().abs() * 2.0 ** -10).all()), (H, Pm)
        assert int(flips.any(-1).sum()) <= 4, (H, Pm, int(flips.any(-1).sum()))          # rows that moved: inside test_pretext_guarded's cap
        assert float(amb.double().mean()) < 0.05, (H, Pm, float(amb.double().mean()))     # entries inside the window
        row_frac = float(amb.any(-1).double().mean())                                     # rows holding one: most of them (measured 0.40, 0.90, 0.69)
        assert rows_lo <= row_frac <= rows_hi, (H, Pm, row_frac)
