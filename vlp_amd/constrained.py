"""Constrained beam search (Anderson et al., "Guided Open Vocabulary Image Captioning with Constrained Beam Search", 2017; the banked
selection is the dynamic beam allocation of Post & Vilar, 2018): the selection step of one frame when every image carries up to MAX_CONS
phrases that its caption must mention.  A phrase is 1..MAX_LEN word-piece ids; cons_ids int32 [B, C, Lc], cons_len int32 [B, C] (0: an unused
slot), ids in [0, V) and never eos (check_constraints, on the host before anything is launched).

    state        one int32 per beam: bits 0-7 `met` (bit c: phrase c is finished), bits 8-11 `cur + 1` (the phrase in progress, 0: none),
                 bits 16-23 `off` (how many tokens of `cur` are matched).  0 before frame 0.
    advance      (state, w): a phrase in progress whose next token is w moves on (off += 1; at off == len its bit is set and cur becomes
                 none).  On a mismatch the progress is dropped -- no KMP-style fallback -- and the start rule sees w: the lowest c with
                 len > 0, not met and cons[c][0] == w begins (and is met at once when len == 1).  A beam whose parent had ended
                 (last_eos != 0) keeps its parent's state.
    wanted       (state) per c: -1 when c is unused or met, cons[c][off] when c is in progress, cons[c][0] otherwise; all -1 for an ended
                 beam (one whose word is eos).
    bank         (state): the sum of len over the met phrases, plus off.  Tb = the sum of len over the image's phrases (<= 64).
    candidates   of image b: for parent row r (only r = 0 on the first frame) and slot j in [0, K + C), index i = r*(K+C) + j.  Slots j < K are
                 the row's top-K list (vlp_logsoftmax_topk_want); slot K + c is the row's wanted word c with its log-softmax value, absent
                 when the id is -1, when it is one of the row's K list ids or when it equals a wanted id of the row with smaller c.
                     v0 = (score + last_eos[b,r] * -10000.0f) + last_total[b,r]        (fp32, vlp_beam_select's expression and order)
                 and v0 = score on the first frame.  The candidate's state is advance(parent state, word).
    unmet eos    a candidate whose word is eos, whose parent had not ended and whose new state has not met every phrase is a forbidden word:
                 -10000.0f is added to its v0 (the convention of the n-gram blocking), and that value stays in out_scores.
    unmet end    the search's last frame (`last`) ends every hypothesis as an eos would: there, every candidate of a parent that had not
                 ended whose new state has not met every phrase is forbidden in the same way, whatever its word.  (Without this a search
                 whose hypotheses reach the target length -- they are ranked next to the finished ones -- would return the best unmet
                 one: the banks always keep a beam that has matched nothing, and it scores best.)
    live / dead  dead: the parent had ended, or an unmet eos / end.  Everything else is live.
    selection    K picks.  A bank cursor starts at Tb and moves down, wrapping from 0 back to Tb; it skips banks without an unpicked live
                 candidate.  A pick is the best unpicked live candidate of the cursor's bank in the (v0 descending, i ascending) order, a NaN
                 ordering as -inf (diverse.py's rule; a NaN v0 is stored as the canonical quiet NaN); the cursor then stands one below that bank.  When no live candidate is left the
                 remaining picks are the dead candidates in the same order.  Pick n goes to slot b*K + n.
    outputs      the six of vlp_beam_select with their meaning (out_scores = v0, out_ptrs = r, src_rows = b*K + r, or b on the first frame),
                 plus out_state [B, K] and want_next int32 [B*K, C] = wanted of every picked beam: the next frame's want_ids.

What follows from the rule:
  * with every cons_len == 0 there is no extra slot, one bank and no unmet eos: the picks are vlp_beam_select's bits on every frame whose
    live candidates outrank its dead ones -- any frame of a search, where a dead candidate carries the -10000 of its ended parent (the
    live-before-dead order is this rule's own; vlp_beam_select orders by value alone, and has no NaN rule);
  * vlp_ngram_candidates, vlp_kv_gather and vlp_beam_nbest need no change: they only follow ptrs / src_rows;
  * a hypothesis that ends, with eos or at the last frame, has met all its phrases, unless that end was a dead pick: it then carries the
    -10000 in its score, as a blocked n-gram does, and ranks behind everything that is not forbidden;
  * nothing is guaranteed when the beam is narrower than the work: with K < Tb + 1 the banks cannot all hold a beam, a phrase in progress
    can lose its only carrier to a better-scoring bank neighbour, and a target that ends before the phrases fit ends unmet.  K >= Tb + 1
    and a target with room for the phrases is the setting in which the search satisfies them.

beam_select_constrained_host is the specification (numpy, float32 where the kernel is float32); the device form is
vlp_beam_select_constrained (csrc/elementwise.hip) behind Engine.decode_beam(constraints=...), BertForSeq2SeqDecoder.beam_search(...,
constraints=...) and python -m vlp_amd.decode_img2txt --constraints_file PATH.
"""
import numpy as np

MAX_CONS, MAX_LEN = 8, 8          # phrases per image, word pieces per phrase (vlp_beam_select_constrained keeps them in LDS)
MIN_BEAMS, MAX_BEAMS = 2, 64      # Engine.decode_beam's limits


def _np(t, dt):
    return np.ascontiguousarray((t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)).astype(dt, copy=False))


def check_limits(K, C, Lc):
    K, C, Lc = int(K), int(C), int(Lc)
    if not (MIN_BEAMS <= K <= MAX_BEAMS and 1 <= C <= MAX_CONS and 1 <= Lc <= MAX_LEN):
        raise ValueError("a constrained beam search needs %d <= beams <= %d, 1 <= phrases per image <= %d and 1 <= pieces per phrase <= %d "
                         "(got beams=%d, C=%d, Lc=%d)" % (MIN_BEAMS, MAX_BEAMS, MAX_CONS, MAX_LEN, K, C, Lc))


def check_constraints(cons_ids, cons_len, vocab_size, eos_id):
    """The host check of a (cons_ids [B, C, Lc], cons_len [B, C]) pair; returns them as int32 arrays."""
    ci, cl = _np(cons_ids, np.int64), _np(cons_len, np.int64)
    if ci.ndim != 3 or cl.ndim != 2 or ci.shape[:2] != cl.shape:
        raise ValueError("constraints are cons_ids [batch, C, Lc] and cons_len [batch, C] (got %r and %r)" % (ci.shape, cl.shape))
    B, C, Lc = ci.shape
    if not (1 <= C <= MAX_CONS and 1 <= Lc <= MAX_LEN):
        raise ValueError("constraints hold 1..%d phrases of 1..%d word pieces per image (got C=%d, Lc=%d)" % (MAX_CONS, MAX_LEN, C, Lc))
    if cl.min() < 0 or cl.max() > Lc:
        raise ValueError("cons_len must lie in 0..Lc = 0..%d" % Lc)
    used = np.arange(Lc)[None, None, :] < cl[:, :, None]
    if used.any():
        ids = ci[used]
        if ids.min() < 0 or ids.max() >= int(vocab_size):
            raise ValueError("a constraint's word id lies outside the vocabulary [0, %d)" % int(vocab_size))
        if (ids == int(eos_id)).any():
            raise ValueError("a constraint must not contain the end-of-sequence id %d" % int(eos_id))
    return ci.astype(np.int32), cl.astype(np.int32)


def pack_constraints(lists, batch, C=None, Lc=None):
    """A list, one entry per image, of lists of id lists -> (cons_ids int32 [B, C, Lc], cons_len int32 [B, C]), C and Lc the largest that
    occur (at least 1) or, when given, at least that.  Empty phrases are refused; an image may have no phrase."""
    if len(lists) != int(batch):
        raise ValueError("constraints: %d entries for a batch of %d images" % (len(lists), int(batch)))
    C = max([len(p) for p in lists] + [1, int(C or 1)])
    Lc = max([len(ph) for p in lists for ph in p] + [1, int(Lc or 1)])
    if C > MAX_CONS or Lc > MAX_LEN:
        raise ValueError("constraints hold at most %d phrases of at most %d word pieces per image (got %d, %d)" % (MAX_CONS, MAX_LEN, C, Lc))
    ci, cl = np.zeros((len(lists), C, Lc), np.int32), np.zeros((len(lists), C), np.int32)
    for b, phrases in enumerate(lists):
        for c, ph in enumerate(phrases):
            if len(ph) == 0:
                raise ValueError("constraints: image %d has an empty phrase" % b)
            ci[b, c, :len(ph)] = [int(t) for t in ph]
            cl[b, c] = len(ph)
    return ci, cl


def _unpack(state):
    state = int(state)
    return state & 0xFF, ((state >> 8) & 0xF) - 1, (state >> 16) & 0xFF


def _pack(met, cur, off):
    return int(met) | ((int(cur) + 1) << 8) | (int(off) << 16)


def advance(state, w, cons_ids, cons_len, parent_ended=False):
    """The state of a beam that appends word w; cons_ids [C, Lc] / cons_len [C] of its image."""
    if parent_ended:
        return int(state)
    met, cur, off = _unpack(state)
    C, w = len(cons_len), int(w)
    if cur >= 0 and (cur >= C or off >= int(cons_len[cur])):     # no state this module makes; the kernel drops it the same way
        cur, off = -1, 0
    if cur >= 0:
        if w == int(cons_ids[cur][off]):
            off += 1
            if off == int(cons_len[cur]):
                met, cur, off = met | (1 << cur), -1, 0
            return _pack(met, cur, off)
        cur, off = -1, 0
    for c in range(C):
        if int(cons_len[c]) > 0 and not (met >> c) & 1 and int(cons_ids[c][0]) == w:
            if int(cons_len[c]) == 1:
                met |= 1 << c
            else:
                cur, off = c, 1
            break
    return _pack(met, cur, off)


def wanted(state, cons_ids, cons_len, ended=False):
    met, cur, off = _unpack(state)
    C = len(cons_len)
    out = np.full(C, -1, np.int32)
    if ended:
        return out
    for c in range(C):
        n = int(cons_len[c])
        if n > 0 and not (met >> c) & 1:
            out[c] = int(cons_ids[c][off]) if (c == cur and off < n) else int(cons_ids[c][0])
    return out


def bank(state, cons_len):
    met, cur, off = _unpack(state)
    return sum(int(cons_len[c]) for c in range(len(cons_len)) if (met >> c) & 1) + (off if cur >= 0 else 0)


def full_mask(cons_len):
    return sum(1 << c for c in range(len(cons_len)) if int(cons_len[c]) > 0)


def constraints_met(seq, cons_ids, cons_len, eos_id=None):
    """The met mask after walking the words of one finished hypothesis (a 1-d id sequence) with advance: to its end, or with eos_id to its
    first eos (what follows in a padded row is not part of the hypothesis)."""
    st = 0
    for w in (seq.tolist() if hasattr(seq, "tolist") else list(seq)):
        if eos_id is not None and int(w) == int(eos_id):
            break
        st = advance(st, int(w), cons_ids, cons_len)
    return st & 0xFF


def beam_select_constrained_host(kk_scores, kk_ids, want_ids, want_val, last_total, last_eos, prev_state, cons_ids, cons_len, first, eos_id,
                                 next_ids_stride=1, trace=None, last=False):
    """kk_scores f32 / kk_ids int64 [B, K, K] ([B, K] on the first frame), want_ids int32 / want_val f32 [B, K, C] ([B, C] on the first frame;
    [B*K, C] is taken too), last_total / last_eos f32 and prev_state int32 [B, K] (None on the first frame), cons_ids [B, C, Lc], cons_len
    [B, C]; arrays or tensors.  Returns (out_scores f32, out_ids int64, out_ptrs int64, out_eos f32 [B, K], src_rows int64 [B*K], next_ids
    int64 [B*K, next_ids_stride], out_state int32 [B, K], want_next int32 [B*K, C]).  `trace`, a dict, receives what the frame went through:
    the counts 'unmet_eos' (unmet ends of a last frame included), 'dropped' (a phrase in progress lost), 'wraps' (the cursor went from bank 0
    back to Tb) and 'dead_picks'.  last: this is the search's last frame."""
    first, eos_id, last = bool(first), int(eos_id), bool(last)
    ks, ki = _np(kk_scores, np.float32), _np(kk_ids, np.int64)
    ci, cl = _np(cons_ids, np.int32), _np(cons_len, np.int32)
    if ks.ndim != (2 if first else 3) or ki.shape != ks.shape or ks.shape[-1] != ks.shape[1]:
        raise ValueError("kk_scores and kk_ids must be [batch, beams, beams] arrays of one shape ([batch, beams] on the first frame)")
    B, K = ks.shape[0], ks.shape[1]
    if ci.ndim != 3 or ci.shape[0] != B or cl.shape != ci.shape[:2]:
        raise ValueError("cons_ids must be [batch, C, Lc] and cons_len [batch, C]")
    C, Lc = ci.shape[1], ci.shape[2]
    if not (1 <= K <= MAX_BEAMS and 1 <= C <= MAX_CONS and 1 <= Lc <= MAX_LEN):
        raise ValueError("needs 1 <= beams <= %d, 1 <= C <= %d, 1 <= Lc <= %d" % (MAX_BEAMS, MAX_CONS, MAX_LEN))
    R = 1 if first else K
    wi, wv = _np(want_ids, np.int32).reshape(B, R, C), _np(want_val, np.float32).reshape(B, R, C)
    ks, ki = ks.reshape(B, R, K), ki.reshape(B, R, K)
    if first:
        lt, le, ps = np.zeros((B, 1), np.float32), np.zeros((B, 1), np.float32), np.zeros((B, 1), np.int32)
    else:
        if last_total is None or last_eos is None or prev_state is None:
            raise ValueError("a later frame needs last_total, last_eos and prev_state")
        lt, le, ps = _np(last_total, np.float32), _np(last_eos, np.float32), _np(prev_state, np.int32)
        if lt.shape != (B, K) or le.shape != (B, K) or ps.shape != (B, K):
            raise ValueError("last_total, last_eos and prev_state must be [batch, beams]")
    f32, S = np.float32, K + C
    out_scores, out_eos = np.zeros((B, K), np.float32), np.zeros((B, K), np.float32)
    out_ids, out_ptrs = np.zeros((B, K), np.int64), np.zeros((B, K), np.int64)
    out_state, want_next = np.zeros((B, K), np.int32), np.full((B * K, C), -1, np.int32)
    src_rows = np.zeros(B * K, np.int64)
    tr = dict(unmet_eos=0, dropped=0, wraps=0, dead_picks=0)
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(B):
            cid, cln = ci[b], cl[b]
            Tb, full = int(cln.sum()), full_mask(cln)
            cand = []                       # (i, word, v0, key, state, bank, live)
            for r in range(R):
                ended = bool(le[b, r] != 0)
                for j in range(S):
                    if j < K:
                        w, sc = int(ki[b, r, j]), ks[b, r, j]
                    else:
                        c = j - K
                        w, sc = int(wi[b, r, c]), wv[b, r, c]
                        if w == -1 or (ki[b, r] == w).any() or (wi[b, r, :c] == w).any():
                            continue
                    v0 = sc if first else f32(f32(sc + f32(le[b, r] * f32(-10000.0))) + lt[b, r])
                    st = advance(ps[b, r], w, cid, cln, parent_ended=ended)
                    _, pcur, poff = _unpack(ps[b, r])
                    if not ended and 0 <= pcur < C and poff < int(cln[pcur]) and w != int(cid[pcur][poff]):
                        tr["dropped"] += 1
                    unmet = (w == eos_id or last) and not ended and (st & 0xFF) != full
                    if unmet:
                        v0 = f32(v0 + f32(-10000.0))
                        tr["unmet_eos"] += 1
                    if np.isnan(v0):
                        v0 = f32(np.nan)            # one NaN: the canonical quiet one, as the kernel stores it
                    key = f32(-np.inf) if np.isnan(v0) else f32(v0)
                    cand.append((r * S + j, w, f32(v0), key, st, bank(st, cln), not (ended or unmet)))
            left = list(cand)
            cursor = Tb
            for n in range(K):
                live = [x for x in left if x[6]]
                if live:
                    t, wrapped = cursor, False
                    while not any(x[5] == t for x in live):
                        t, wrapped = (t - 1, wrapped) if t > 0 else (Tb, True)
                    tr["wraps"] += int(wrapped)
                    pool = [x for x in live if x[5] == t]
                    cursor = t - 1 if t > 0 else Tb
                    tr["wraps"] += int(t == 0 and Tb > 0 and n + 1 < K)
                else:
                    pool = left
                    tr["dead_picks"] += 1
                pick = min(pool, key=lambda x: (-x[3], x[0]))         # v0 descending (NaN as -inf), index ascending
                left.remove(pick)
                i, w, v0, _, st, _, _ = pick
                r = i // S
                out_scores[b, n], out_ids[b, n], out_ptrs[b, n], out_state[b, n] = v0, w, r, st
                out_eos[b, n] = 1.0 if w == eos_id else 0.0
                src_rows[b * K + n] = b if first else b * K + r
                want_next[b * K + n] = wanted(st, cid, cln, ended=(w == eos_id))
    if trace is not None:
        trace.update(tr)
    next_ids = np.zeros((B * K, int(next_ids_stride)), np.int64)
    next_ids[:, 0] = out_ids.reshape(-1)
    return out_scores, out_ids, out_ptrs, out_eos, src_rows, next_ids, out_state, want_next
