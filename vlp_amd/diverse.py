"""Diverse (group) beam search (Vijayakumar et al., "Diverse Beam Search", 2016): the selection step of one frame with the K beams of an image
split into G groups of Kg = K / G.  The groups are extended one after another inside the frame; a candidate word is penalised by lambda for
every time an earlier group has already chosen that word in this frame.  Per image b, for g = 0 .. G-1 in order:

    candidates   later frames: the continuations of the group's own rows r in [g*Kg, (g+1)*Kg), index i = r*K + j (beam_select_kernel's index),
                     v0 = (kk_scores[b,r,j] + last_eos[b,r] * -10000.0f) + last_total[b,r]      (fp32, the kernel's expression and order)
                 first frame: every group sees the single row, i = j, v0 = kk_scores[b,j], pointer 0
    key          v0 - fl32(lambda * c), c = the number of picks of the groups < g of this frame and image whose word is the candidate's (every
                 pick counts: eos, and picks whose parent had ended, too); the product is rounded to fp32 before the subtraction.  A key that
                 is NaN (+inf + -inf in v0) orders as -inf, so a pick always exists
    selection    Kg successive picks, each the maximum of the candidates that come after the previous pick in the (key descending, i ascending)
                 order: the strict scan of beam_select_kernel, so -inf candidates and ties need no special case
    outputs      pick n of group g goes to slot b*K + g*Kg + n: out_scores = v0, the UNPENALISED cumulative log-probability (the penalty steers
                 the selection only, so the n-best ranking, --select logprob and the length penalty keep their meaning), out_ids, out_ptrs = r
                 (0 on the first frame), out_eos, src_rows = b*K + r (b on the first frame), next_ids

What follows from the rule:
  * parents stay inside their group: ptrs[s][b][k] // Kg == k // Kg for every frame s >= 1;
  * with lambda = 0 the groups of the first frame pick the same words (they all see the one row), and stay copies of each other;
  * G = 1 is vlp_beam_select's result bit for bit, for any lambda (no earlier group, c = 0), on inputs whose values v0 hold no NaN (the NaN
    rule above is an addition: beam_select_kernel never picks a NaN candidate and is undefined when only NaN candidates remain);
  * vlp_ngram_candidates, vlp_kv_gather and vlp_beam_nbest need no change: they only follow ptrs / src_rows.

The per-row top-K lists of vlp_logsoftmax_topk(_list) are enough, no second pass over the vocabulary is needed: group g picks Kg candidates and
penalises at most K - Kg distinct words (the picks of the earlier groups).  A word outside a row's top K has K words above it in that row; at
most K - Kg of them are penalised, so at least Kg unpenalised words of the row stay above it.  Those keep their score and the word's own score
cannot rise, so it can never be among the Kg picks.  (With exact ties at the K-th place the two forms may name different words of equal score:
the list orders ties by word id, a scan of the whole vocabulary by r*V + v.)

beam_select_groups_host is the specification (numpy, every operation in float32); the device form is vlp_beam_select_groups
(csrc/elementwise.hip) behind Engine.decode_beam(groups=G, diversity=lambda), BertForSeq2SeqDecoder(beam_groups=G, diversity_penalty=lambda)
and python -m vlp_amd.decode_img2txt --beam_groups G --diversity_penalty L.
"""
import math

import numpy as np

MIN_BEAMS, MAX_BEAMS = 2, 64      # Engine.decode_beam: 2 <= K <= 64 (one wave per image, the earlier groups' picks in LDS)


def check_limits(K, groups, penalty):
    K, G = int(K), int(groups)
    try:
        lam = float(penalty)
    except (TypeError, ValueError):
        lam = float("nan")
    if not (MIN_BEAMS <= K <= MAX_BEAMS and 1 <= G <= K and K % G == 0 and math.isfinite(lam) and lam >= 0.0):
        raise ValueError("a diverse beam search needs %d <= beams <= %d, 1 <= groups <= beams, beams %% groups == 0 and a finite penalty >= 0 "
                         "(got beams=%d, groups=%d, penalty=%r)" % (MIN_BEAMS, MAX_BEAMS, K, G, penalty))


def _key(v0, lam, cnt):
    """v0 - fl32(lam * cnt) on float32 arrays: two roundings, the product first (a fused multiply-subtract rounds once and differs in the last bit)."""
    return (v0 - (lam * cnt).astype(np.float32)).astype(np.float32)


def beam_select_groups_host(kk_scores, kk_ids, last_total, last_eos, first, eos_id, groups, penalty, next_ids_stride=1):
    """kk_scores f32 / kk_ids int64 [B, K, K] ([B, K] on the first frame), last_total / last_eos f32 [B, K] (None on the first frame); arrays
    or tensors.  Returns (out_scores f32 [B, K], out_ids int64 [B, K], out_ptrs int64 [B, K], out_eos f32 [B, K], src_rows int64 [B*K],
    next_ids int64 [B*K, next_ids_stride]: column 0 holds the chosen ids, the other columns zeros)."""
    def arr(t, dt):
        return np.ascontiguousarray((t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)).astype(dt, copy=False))
    first = bool(first)
    ks, ki = arr(kk_scores, np.float32), arr(kk_ids, np.int64)
    if ks.ndim != (2 if first else 3) or ki.shape != ks.shape or ks.shape[-1] != ks.shape[1]:
        raise ValueError("kk_scores and kk_ids must be [batch, beams, beams] arrays of one shape ([batch, beams] on the first frame)")
    B, K = ks.shape[0], ks.shape[1]
    G, lam = int(groups), np.float32(penalty)
    check_limits(K, G, penalty)
    Kg = K // G
    f32 = np.float32
    with np.errstate(invalid="ignore", over="ignore"):
        if first:
            v0 = ks                                                             # [B, K]
            ids = ki
        else:
            if last_total is None or last_eos is None:
                raise ValueError("a later frame needs last_total and last_eos")
            lt, le = arr(last_total, np.float32), arr(last_eos, np.float32)
            if lt.shape != (B, K) or le.shape != (B, K):
                raise ValueError("last_total and last_eos must be [batch, beams]")
            v0 = ((ks + (le * f32(-10000.0))[:, :, None]) + lt[:, :, None]).astype(np.float32).reshape(B, K * K)
            ids = ki.reshape(B, K * K)
        out_scores, out_eos = np.zeros((B, K), np.float32), np.zeros((B, K), np.float32)
        out_ids, out_ptrs = np.zeros((B, K), np.int64), np.zeros((B, K), np.int64)
        src_rows = np.zeros(B * K, np.int64)
        for b in range(B):
            picked = []
            for g in range(G):
                idx = np.arange(K) if first else np.arange(g * Kg * K, (g + 1) * Kg * K)
                cnt = np.zeros(len(idx), np.float32)
                for w in picked:
                    cnt += (ids[b, idx] == w)
                key = _key(v0[b, idx], lam, cnt)
                key[np.isnan(key)] = -np.inf
                order = idx[np.lexsort((idx, -key))][:Kg]                       # key descending, index ascending: the strict scan's order
                for n, i in enumerate(order.tolist()):
                    k, r = g * Kg + n, (0 if first else i // K)
                    out_scores[b, k], out_ids[b, k], out_ptrs[b, k] = v0[b, i], ids[b, i], r
                    out_eos[b, k] = 1.0 if ids[b, i] == int(eos_id) else 0.0
                    src_rows[b * K + k] = b if first else b * K + r
                picked.extend(out_ids[b, g * Kg:(g + 1) * Kg].tolist())
    next_ids = np.zeros((B * K, int(next_ids_stride)), np.int64)
    next_ids[:, 0] = out_ids.reshape(-1)
    return out_scores, out_ids, out_ptrs, out_eos, src_rows, next_ids
