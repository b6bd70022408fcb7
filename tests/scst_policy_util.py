"""Shared by tests/test_scst_policy_cpu.py and tests/test_86_scst_policy_gpu.py: the fp64 restatement of the SCST policy kernels
(include/vlp_hip.h vlp_token_policy_fwd / _bwd) and the rows both files check it on."""
import math

import torch

GRID_V = (1, 7, 8, 257, 1000, 28996)
GRID_T = (0.5, 0.7, 1.0, 2.0)


def policy_reference(row16, id, T, g=None, h=None):
    """One fp16 logits row [V] in fp64: z = l / T, lse = logsumexp(z), q = exp(z - lse), logp = z_id - lse (id clamped to [0, V)),
    H = -sum q log q with 0 log 0 = 0.  With g (and h, default 0) also dlogits = (1/T) (g ([v == id] - q) - h q (log q + H)), the entropy term
    exactly 0 where q == 0.  Returns a dict of python floats / an fp64 tensor."""
    l = row16.detach().to(torch.float64).reshape(-1).cpu()
    V = l.numel()
    T = float(T)
    i = min(max(int(id), 0), V - 1)
    m = float(l.max())
    d = (l - m) / T                                   # <= 0; -inf stays -inf
    e = torch.exp(d)
    S = float(e.sum())
    lse = m / T + math.log(S)
    lq = d - math.log(S)                              # log q
    q = e / S
    live = q > 0
    H = -float((q[live] * lq[live]).sum())
    out = {"lse": lse, "logp": float(lq[i]), "H": H, "id": i}
    if g is not None:
        onehot = torch.zeros(V, dtype=torch.float64)
        onehot[i] = 1.0
        ent = torch.zeros(V, dtype=torch.float64)
        ent[live] = q[live] * (lq[live] + H)
        out["dlogits"] = (float(g) * (onehot - q) - float(0.0 if h is None else h) * ent) / T
    return out


def reference_rows(rows16, ids, T, g=None, h=None):
    """policy_reference over the rows of a [R, V] fp16 tensor: (lse [R], logp [R], H [R], dlogits [R, V] or None), fp64 on the CPU."""
    rows16, ids = rows16.detach().cpu(), ids.detach().cpu()
    R = rows16.shape[0]
    refs = [policy_reference(rows16[r], int(ids[r]), T, None if g is None else float(g[r]), None if h is None else float(h[r])) for r in range(R)]
    col = lambda k: torch.tensor([x[k] for x in refs], dtype=torch.float64)
    return col("lse"), col("logp"), col("H"), (None if g is None else torch.stack([x["dlogits"] for x in refs]))


def grid_rows(V, R, seed):
    """N(0, 3^2) fp16 logits [R, V] and ids [R] that include 0, V - 1 and out-of-range values (-3, V + 5: clamped) when R allows."""
    gen = torch.Generator().manual_seed(seed)
    x = (torch.randn(R, V, generator=gen) * 3.0).half()
    ids = torch.randint(0, V, (R,), generator=gen)
    for r, v in zip(range(R), (V + 5, 0, V - 1, -3)) if R > 1 else ((0, V + 5),):
        ids[r] = v
    return x, ids


def hard_rows(V=1000):
    """name -> (fp16 row [V], id): the hand-built rows of the issue."""
    inf = float("inf")
    rows = {}
    rows["all_equal"] = (torch.full((V,), 1.5).half(), V // 2)
    peak = torch.full((V,), -20.0)
    peak[V // 3] = 20.0
    rows["one_peak"] = (peak.half(), V // 3)
    gen = torch.Generator().manual_seed(5)
    third = (torch.randn(V, generator=gen) * 3.0)
    third[::3] = -inf
    rows["third_minus_inf"] = (third.half(), 1)
    one = torch.full((V,), -inf)
    one[min(7, V - 1)] = 2.0
    rows["one_finite"] = (one.half(), min(7, V - 1))
    span = torch.linspace(-65504.0, 65504.0, V)
    rows["span_fp16"] = (span.half(), V - 1)
    return rows


def forced_decode_logits(O, p, vf, vp, input_ids, token_type_ids, position_ids, am, sample_ids, mask_id, num_heads=12, Nv=100):
    """The oracle decoder's incremental forward (oracle.vlp_oracle._incr_step, passed in as O) fed the given sampled ids: every step's [MASK]
    logits [B, T, V], with autograd -- tests/test_scst_cpu.forced_decode_logp before its log_softmax."""
    in_len, out_len = input_ids.shape[1], token_type_ids.shape[1]
    prev_emb = prev_layers = None
    curr = input_ids
    mask_ids = input_ids[:, :1] * 0 + mask_id
    out, t, next_pos = [], 0, in_len
    while next_pos < out_len:
        st = next_pos - curr.shape[1]
        x_ids = torch.cat((curr, mask_ids), dim=1)
        emb, new_layers, logits = O._incr_step(p, vf, vp, x_ids, token_type_ids[:, st:next_pos + 1], position_ids[:, st:next_pos + 1],
                                               am[:, st:next_pos + 1, :next_pos + 1], prev_emb, prev_layers, num_heads, Nv)
        out.append(logits[:, -1, :])
        prev_emb = emb[:, :-1] if prev_emb is None else torch.cat((prev_emb, emb[:, :-1]), dim=1)
        prev_layers = [x[:, :-1] for x in new_layers] if prev_layers is None else [torch.cat((a, b[:, :-1]), dim=1)
                                                                                      for a, b in zip(prev_layers, new_layers)]
        curr = sample_ids[:, t:t + 1]
        next_pos += 1
        t += 1
    return torch.stack(out, dim=1)


def tempered_logp_entropy(logits, ids, T):
    """log softmax(logits / T) at ids and the entropy of softmax(logits / T), both [B, n], in torch (differentiable)."""
    lp = torch.log_softmax(logits / T, dim=-1)
    H = -(lp.exp() * lp).sum(-1)
    return lp.gather(2, ids.unsqueeze(2)).squeeze(2), H
