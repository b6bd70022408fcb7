"""Helpers of the diverse beam search tests (tests/test_diverse_beam_cpu.py, tests/test_47_diverse_beam_gpu.py): a transcription of
beam_select_kernel's scan, a brute force of the grouped selection over the whole vocabulary, and frames built to hurt."""
import numpy as np

F32 = np.float32


def scan_select(kk_scores, kk_ids, last_total, last_eos, first, eos_id):
    """beam_select_kernel (csrc/elementwise.hip) line by line: K successive strict scans over the K*K continuations (K on the first frame)."""
    kk_scores, kk_ids = np.asarray(kk_scores, F32), np.asarray(kk_ids, np.int64)
    B, K = kk_scores.shape[:2]
    out_scores, out_eos = np.zeros((B, K), F32), np.zeros((B, K), F32)
    out_ids, out_ptrs, src_rows = np.zeros((B, K), np.int64), np.zeros((B, K), np.int64), np.zeros(B * K, np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(B):
            pv, pi = F32(np.inf), -1
            for k in range(K):
                best, bi = F32(-np.inf), 0x7fffffff
                for i in range(K if first else K * K):
                    if first:
                        val = kk_scores[b, i]
                    else:
                        src = i // K
                        val = F32(F32(kk_scores[b, src, i % K] + F32(last_eos[b, src] * F32(-10000.0))) + last_total[b, src])
                    after = (val < pv) or (val == pv and i > pi)
                    if after and (val > best or (val == best and i < bi)):
                        best, bi = val, i
                pv, pi = best, bi
                ptr = 0 if first else bi // K
                wid = kk_ids[b, bi] if first else kk_ids[b, ptr, bi % K]
                out_scores[b, k], out_ids[b, k], out_ptrs[b, k], out_eos[b, k] = best, wid, ptr, 1.0 if wid == eos_id else 0.0
                src_rows[b * K + k] = b if first else b * K + ptr
    return out_scores, out_ids, out_ptrs, out_eos, src_rows


def topk_lists(logp, K):
    """Per-row top-K lists of [..., V] scores as vlp_logsoftmax_topk writes them: value descending, word id ascending on ties."""
    order = np.argsort(-logp, axis=-1, kind="stable")[..., :K]
    return np.take_along_axis(logp, order, axis=-1).astype(F32), order.astype(np.int64)


def brute_force(logp, last_total, last_eos, first, K, groups, penalty):
    """The grouped selection over the whole vocabulary: logp [B, K, V] ([B, V] on the first frame).  Returns per image the list of K
    (parent, word) pairs in slot order."""
    logp = np.asarray(logp, F32)
    B, V = logp.shape[0], logp.shape[-1]
    Kg, lam = K // groups, F32(penalty)
    out = []
    for b in range(B):
        picks = []
        for g in range(groups):
            rows = [0] if first else list(range(g * Kg, (g + 1) * Kg))
            cands = []
            for r in rows:
                for v in range(V):
                    v0 = logp[b, v] if first else F32(F32(logp[b, r, v] + F32(last_eos[b, r] * F32(-10000.0))) + last_total[b, r])
                    c = sum(1 for _, w in picks if w == v)
                    cands.append((-float(F32(v0 - F32(lam * F32(c)))), r * V + v, r, v))
            cands.sort()
            picks.extend((r, v) for _, _, r, v in cands[:Kg])
        out.append(picks)
    return out


EOS = 3
SCORE_VALUES = np.array([-1.5, -0.75, -2.25, -3.0], dtype=F32)


def hostile_frame(B, K, first, seed):
    """Inputs of one selection step built to hurt: scores from four values (ties decide), ids from a vocabulary of 6 (one word tops many rows,
    counts reach >= 2; EOS = 3 is one of them), 10 % -inf, 30 % ended parents; with B >= 3 the last image is all -inf and, in a later frame,
    the image before it has only ended parents (smaller batches keep ordinary images only).  Returns (kk_scores, kk_ids, last_total, last_eos), read only."""
    rng = np.random.RandomState(seed)
    shape = (B, K) if first else (B, K, K)
    ks = rng.choice(SCORE_VALUES, size=shape)
    ks[rng.rand(*shape) < 0.1] = -np.inf
    ki = rng.randint(0, 6, size=shape).astype(np.int64)
    lt = rng.choice(SCORE_VALUES, size=(B, K)) * F32(3.0)
    le = (rng.rand(B, K) < 0.3).astype(F32)
    if B >= 3:
        ks[B - 1] = -np.inf
        le[B - 2] = 1.0
    out = (ks.astype(F32), ki, None if first else lt.astype(F32), None if first else le)
    for a in out:
        if a is not None:
            a.setflags(write=False)
    return out


def fused_key(v0, lam, cnt):
    """What a contracted multiply-subtract gives: fl32(v0 - lam * cnt) with ONE rounding (the fp64 product of an fp32 and a small integer and
    the fp64 difference are exact here).  Stands in for vlp_amd.diverse._key to show what a case can tell apart."""
    return (v0.astype(np.float64) - np.float64(lam) * cnt.astype(np.float64)).astype(F32)


SEPARATING_PENALTY = 0.3


def separating_frame():
    """A later frame (B = 1, K = 18, G = 2, lambda = 0.3) on which a fused key changes the picks.  Group 0 (rows 0..8) picks word 11 seven
    times and word 10 twice (each row's best continuation at -1, the rest far below).  Row 9 of group 1 holds word 11 at v0 = -2.25 (i = 162)
    and word 10 at v0 = -3.75 (i = 163).  fl32(0.3f * 7) = 2.1000001430511475 (the exact product 2.1000000834... lies between two floats of
    the [2, 4) binade), 0.3f * 2 is exact; the keys lie in [4, 8), where floats are 2^-21 apart:
        two roundings   word 11: -9122612 * 2^-21    word 10: -9122611 * 2^-21    -> word 10 is picked first, then word 11
        one rounding    both -9122611 * 2^-21: a tie, the lower index wins        -> word 11 first, then word 10
    so slots 9 and 10 swap ids and scores.  Everything else of group 1 is far below (-50, distinct unpenalised words).
    Returns (kk_scores, kk_ids, last_total, last_eos), read only."""
    K = 18
    ks = np.full((1, K, K), -50.0, dtype=F32)
    ki = (100 + np.arange(K * K, dtype=np.int64)).reshape(1, K, K)
    ks[0, :9, 0] = -1.0
    ki[0, :7, 0], ki[0, 7:9, 0] = 11, 10
    ks[0, 9, 0], ks[0, 9, 1] = -2.25, -3.75
    ki[0, 9, 0], ki[0, 9, 1] = 11, 10
    out = (ks, ki, np.zeros((1, K), F32), np.zeros((1, K), F32))
    for a in out:
        a.setflags(write=False)
    return out
