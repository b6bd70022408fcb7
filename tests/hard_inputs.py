"""Library-free helpers of the kernel tests: the error metric, the attention masks and fp64 restatement, and the hard inputs of
tests/test_06_kernel_hard_values_gpu.py with fp32 restatements of the ops at the kernels' documented rounding points.  Nothing here loads
libvlp_hip.so, so tests/test_hard_inputs_cpu.py can measure the restatements against fp64 on any machine: the figures test_06 quotes beside
its bounds are asserted there."""
import torch


def rel(a, b):
    """max(max-normalised error, relative L2 error): the first bounds the worst element against the tensor's scale, the second is not
    blind to errors spread over the many small elements."""
    a, b = a.detach().double(), b.detach().double()
    d = a - b
    return max(float(d.abs().max() / (b.abs().max() + 1e-30)), float(d.norm() / (b.norm() + 1e-30)))


# ---- attention: random s2s / bi masks of the loader, and the fp64 restatement of the fused kernel ---------
def attn_mask(B, L, Nv, gen_cpu):
    from vlp_amd import synthetic as S
    m = torch.zeros(B, L, L, dtype=torch.long)
    for b in range(B):
        n_b = int(torch.randint(1, L - Nv - 2, (1,), generator=gen_cpu))
        m[b] = S.build_attention_mask(L, Nv, n_b, "s2s" if b % 2 == 0 else "bi")
    return m


def attn_ref(qkv, mask, B, L, heads, mult=None):
    H = heads * 64
    x = qkv.double().view(B, L, 3, heads, 64)
    q, k, v = (x[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    s = q @ k.transpose(-1, -2) / 8.0 + (1.0 - mask.double().to(qkv.device))[:, None] * -10000.0
    p = torch.softmax(s, -1)
    pd = p if mult is None else p * mult
    return (pd @ v).permute(0, 2, 1, 3).reshape(B * L, H), p


# ---- hard inputs (tests/test_06_kernel_hard_values_gpu.py) ---------------------------------------------------------------------
def ln_hard_rows(M, H, device="cpu", seed=11):
    """[M, H] fp16 rows that punish a LayerNorm shortcut, and a [M] int64 tag per row: 0 = constant row (every third row: variance exactly
    0; the constants are small multiples of 1.5, whose fp32 sums are exact), 1 = 300 + 0.5 randn, 2 = -2000 + 4 randn, 3 = unit noise with
    two outlier channels (+900, -450: the shape of a real BERT residual stream), 4 = one row of +-65504."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, H, generator=g)
    kind = torch.zeros(M, dtype=torch.int64)
    for i in range(M):
        if i % 3 == 0:
            x[i] = 1.5 * ((i // 3) % 7 - 3)
        elif i % 3 == 1:
            kind[i] = 1 + (i // 3) % 2
            x[i] = 300 + 0.5 * x[i] if kind[i] == 1 else -2000 + 4 * x[i]
        else:
            kind[i] = 3
            x[i, 5 % H], x[i, 77 % H] = 900.0, -450.0
    last = M - 1 if (M - 1) % 3 else M - 2
    kind[last] = 4
    x[last] = 65504.0 * (1 - 2 * (torch.arange(H) % 2)).float()
    return x.half().to(device), kind.to(device)


def ce_hard_rows(V, device="cpu", seed=12):
    """[8, V] fp16 logits and [8] labels: row 0 = -60000 everywhere except +60000 at one id, label elsewhere (loss 1.2e5); row 1 = all logits
    equal (lse = x + log V); row 2 = -65504 / +65504 alternating, label on a -65504 column; row 3 = 3000 * randn with the label at its argmin;
    rows 4 .. 7 ordinary (2 * randn)."""
    g = torch.Generator().manual_seed(seed)
    x = 2.0 * torch.randn(8, V, generator=g)
    lab = torch.randint(1, V, (8,), generator=g)
    x[0] = -60000.0
    x[0, V // 3] = 60000.0
    lab[0] = V // 3 + 7
    x[1] = 3.5
    x[2] = 65504.0 * (1 - 2 * (torch.arange(V) % 2)).float()
    lab[2] = 1
    x[3] = 3000.0 * torch.randn(V, generator=g)
    x = x.half()
    lab[3] = int(x[3].float().argmin())
    if int(lab[3]) == 0:                      # keep label 0 (the smoothed loss's ignore_index) out of the hard rows
        x[3, 0], x[3, 1] = x[3, 1].clone(), x[3, 0].clone()
        lab[3] = 1
    return x.to(device), lab.to(device)


def attn_hard_qkv(B, L, heads, low_head, device="cpu", seed=13):
    """[B*L, 3H] fp16 at scale 4 (scores of standard deviation ~16: near-one-hot probability rows); in head `low_head` q = 17 + 0.25 randn and
    k = -17 + 0.25 randn, so every score of that head is about -2300: only max subtraction over the attended keys carries it."""
    g = torch.Generator().manual_seed(seed)
    H = heads * 64
    x = (4.0 * torch.randn(B * L, 3, heads, 64, generator=g))
    x[:, 0, low_head] = 17.0 + 0.25 * torch.randn(B * L, 64, generator=g)
    x[:, 1, low_head] = -17.0 + 0.25 * torch.randn(B * L, 64, generator=g)
    return x.reshape(B * L, 3 * H).half().to(device)


def attn_restatement_fp32(qkv, mask, dctx, B, L, heads):
    """fp32 restatement of vlp_attn_fwd / vlp_attn_bwd with the kernels' documented rounding points (P, O and dS rounded to fp16; fp32 sums):
    returns (ctx fp16, lse fp32, dqkv fp16).  It is what the measured bounds of test_06 are taken from, against fp64, never the kernel."""
    H = heads * 64
    x = qkv.float().view(B, L, 3, heads, 64)
    q, k, v = (x[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    s = q @ k.transpose(-1, -2) * 0.125 + (1.0 - mask.float().to(qkv.device))[:, None] * -10000.0
    lse = torch.logsumexp(s, -1)
    p16 = torch.exp(s - lse[..., None]).half().float()
    o16 = (p16 @ v).half()
    do = dctx.float().view(B, L, heads, 64).permute(0, 2, 1, 3)
    dp = do @ v.transpose(-1, -2)
    delta = (do * o16.float()).sum(-1, keepdim=True)
    ds16 = (p16 * (dp - delta)).half().float()
    dq, dk, dv = (ds16 @ k) * 0.125, (ds16.transpose(-1, -2) @ q) * 0.125, p16.transpose(-1, -2) @ do
    dqkv = torch.stack([t.permute(0, 2, 1, 3) for t in (dq, dk, dv)], 2).reshape(B * L, 3 * H).half()
    return o16.permute(0, 2, 1, 3).reshape(B * L, H), lse, dqkv


def layernorm_restatement_fp32(x, gamma, beta, eps=1e-5, two_pass=True):
    """fp32 LayerNorm with one fp16 rounding of the output: two-pass variance (what csrc/layernorm.hip does), or the single-pass
    E[x^2] - E[x]^2 shortcut that the offset rows of ln_hard_rows are there to catch.  Returns (y fp16, mean, rstd)."""
    xf = x.float()
    u = xf.mean(-1, keepdim=True)
    var = (xf - u).pow(2).mean(-1, keepdim=True) if two_pass else ((xf * xf).mean(-1, keepdim=True) - u * u).clamp_min(0)
    rstd = 1.0 / torch.sqrt(var + eps)
    return (gamma.float() * ((xf - u) * rstd) + beta.float()).half(), u[:, 0], rstd[:, 0]


def pretext_sim_window(A, V, H):
    """The similarity matrix of vlp_pretext_fwd in fp64, and which of its entries may round to either neighbouring fp16 value in the kernel.
    A, V: [..., Pm, H] fp16 values (A = vispe + pooled already rounded to fp16).  The kernel sums each H-long dot product in fp32 -- 8
    fused multiply-adds per 8-column chunk, ceil(H / 512) chunks per lane, then a 6-level wave reduction: at most 8 ceil(H / 512) + 6
    roundings of 2^-24, each against no more than sum |a_k v_k| -- and rounds the sum to fp16.  An entry whose fp64 value is farther than
    that from every fp16 rounding boundary rounds the same way in both; the others are returned as `ambiguous`.  (sim fp64, ambiguous)."""
    a, v = A.double(), V.double()
    s64 = a @ v.transpose(-1, -2)
    slack = (8 * ((H + 511) // 512) + 6) * 2.0 ** -24 * (a.abs() @ v.abs().transpose(-1, -2))
    return s64, (s64 - slack).half() != (s64 + slack).half()


def pretext_sim_restatement_fp32(A, V):
    """sim[i][j] of pretext_fwd_kernel (csrc/pretext.hip) in its own summation order, fp32: lane l walks the 8-column chunks l, l + 64, ...
    of the row with one fma per column (the product of two fp16 values is exact in fp32, so an fma is an fp32 add of it), a butterfly over
    the 64 lanes adds the partial sums (both partners of a pair compute the same sum), and the result is rounded to fp16.  A, V: [Pm, H]."""
    Pm, H = A.shape
    nch = H // 8
    prod = (A.float()[:, None, :] * V.float()[None, :, :]).view(Pm, Pm, nch, 8)
    lanes = torch.zeros(Pm, Pm, 64)
    for c in range(nch):
        for t in range(8):
            lanes[:, :, c % 64] = lanes[:, :, c % 64] + prod[:, :, c, t]
    idx = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        lanes = lanes + lanes[:, :, idx ^ o]
    return lanes[:, :, 0].half()


def ce_rows_restatement_fp32(logits, labels):
    """fp32 max-subtracted log-sum-exp per row and row loss lse - logit[label] (the arithmetic of row_lse_kernel with the CE policy): (lse, row_loss)."""
    x = logits.float()
    m = x.max(-1, keepdim=True).values
    lse = (m + torch.log(torch.exp(x - m).sum(-1, keepdim=True)))[:, 0]
    return lse, lse - x.gather(1, labels[:, None])[:, 0]
