"""Helpers of the constrained beam search tests (tests/test_49_constrained_beam_gpu.py): frames of one selection step built to hurt, and the
2-layer model and inputs of the diverse beam search tests (copied from tests/test_47_diverse_beam_gpu.py, not imported from it)."""
import functools

import numpy as np

from vlp_amd import constrained as CB

F32 = np.float32
EOS = 3
WORDS = 12                                                    # word ids 0..11: constraint words, duplicates and eos all occur
SCORE_VALUES = np.arange(-16, 1, dtype=F32) * F32(0.25)       # multiples of 0.25: ties decide


def hostile_frame(B, K, C, Lc, first, seed):
    """Inputs of one constrained selection step.  Phrases of 0..Lc words over the 11 non-eos words (image 0 uses every slot at full length, so
    Tb = C * Lc there; with B >= 3 the last image has no phrase at all and, in a later frame, the image before it only ended parents).  The
    parents' states are made by walking random words with advance, so every state is one the search can reach; want_ids are wanted() of
    those states, with a few overwritten by -1 or a random word; 30 % ended parents; 6 % -inf, 2 % +inf and 2 % NaN among the scores.
    Returns a dict of read-only arrays."""
    rng = np.random.RandomState(seed)
    R = 1 if first else K
    non_eos = np.array([w for w in range(WORDS) if w != EOS])
    cid = rng.choice(non_eos, size=(B, C, Lc)).astype(np.int32)
    cln = rng.randint(0, Lc + 1, size=(B, C)).astype(np.int32)
    cln[0] = Lc
    if B >= 3:
        cln[B - 1] = 0
    ps = np.zeros((B, R), np.int32)
    le = np.zeros((B, R), F32) if first else (rng.rand(B, R) < 0.3).astype(F32)
    if not first:
        if B >= 3:
            le[B - 2] = 1.0
        for b in range(B):
            for r in range(R):
                st = 0
                for _ in range(rng.randint(0, 2 * Lc + 2)):
                    w = CB.wanted(st, cid[b], cln[b])
                    w = w[w >= 0]
                    # mostly a wanted word (phrases progress and finish), else any word (phrases drop)
                    st = CB.advance(st, int(rng.choice(w)) if len(w) and rng.rand() < 0.8 else int(rng.choice(non_eos)), cid[b], cln[b])
                ps[b, r] = st
    want = np.stack([np.stack([CB.wanted(ps[b, r], cid[b], cln[b], ended=bool(le[b, r])) for r in range(R)]) for b in range(B)]).astype(np.int32)
    flip = rng.rand(B, R, C)
    want[flip < 0.1] = -1
    want = np.where((flip > 0.9), rng.randint(0, WORDS, size=(B, R, C)), want).astype(np.int32)
    wv = rng.choice(SCORE_VALUES, size=(B, R, C)).astype(F32) - F32(2.0)
    ks = rng.choice(SCORE_VALUES, size=(B, R, K)).astype(F32)
    for a in (ks, wv):
        u = rng.rand(*a.shape)
        a[u < 0.06] = -np.inf
        a[(u >= 0.06) & (u < 0.08)] = np.inf
        a[(u >= 0.08) & (u < 0.10)] = np.nan
    ki = rng.randint(0, WORDS, size=(B, R, K)).astype(np.int64)
    lt = (rng.choice(SCORE_VALUES, size=(B, R)) * F32(3.0)).astype(F32)
    if first:
        ks, ki, want, wv = ks[:, 0], ki[:, 0], want[:, 0], wv[:, 0]
    out = dict(ks=ks, ki=ki, want=want, wv=wv, lt=None if first else lt, le=None if first else le, ps=None if first else ps, cid=cid, cln=cln)
    for a in out.values():
        if a is not None:
            a.setflags(write=False)
    return out


def host_select(fr, first, trace=None, last=False):
    return CB.beam_select_constrained_host(fr["ks"], fr["ki"], fr["want"], fr["wv"], fr["lt"], fr["le"], fr["ps"], fr["cid"], fr["cln"], bool(first),
                                           EOS, next_ids_stride=2, trace=trace, last=last)


def walk_states(wids, ptrs, eos_id, cons_ids, cons_len):
    """The state of every beam of every frame, recomputed from the traces of one image by walking each hypothesis with advance: wids / ptrs
    int [frames, K].  A beam whose parent's word was eos keeps the parent's state."""
    F, K = wids.shape
    st = np.zeros((F, K), np.int32)
    for s in range(F):
        for k in range(K):
            if s == 0:
                st[s, k] = CB.advance(0, int(wids[s, k]), cons_ids, cons_len)
            else:
                p = int(ptrs[s, k])
                st[s, k] = CB.advance(int(st[s - 1, p]), int(wids[s, k]), cons_ids, cons_len, parent_ended=int(wids[s - 1, p]) == eos_id)
    return st


# ---- the 2-layer model of the n-best / diverse tests, B = 3, 6 generated tokens -------------------------------------------------------------
NB, NT = 3, 6
PLAIN = dict(forbid_duplicate_ngrams=False, min_len=0)
BLOCKED = dict(forbid_duplicate_ngrams=True, ngram_size=2, min_len=3)


@functools.lru_cache(maxsize=None)
def model_inputs(device):
    import torch
    from oracle import vlp_oracle as O
    from oracle.make_golden import BEAM_CASES, decode_inputs
    mk = BEAM_CASES["beam_2l_K3"][0]
    p = O.init_params(vocab_size=mk["vocab_size"], layers=mk["layers"], tasks=mk["tasks"], seed=mk["seed"], std=mk["std"])
    dv = [t.to(torch.device(device)) for t in decode_inputs(NB, NT, 213)]
    return mk, p, [dv[0].half(), dv[1].half()] + dv[2:]


def make_model(device, **kw):
    import torch
    from vlp_amd import synthetic as S
    from vlp_amd.modeling import BertConfig, BertForSeq2SeqDecoder
    mk, p, _ = model_inputs(device)
    cfg = BertConfig(mk["vocab_size"], num_hidden_layers=mk["layers"], type_vocab_size=6)
    m = BertForSeq2SeqDecoder(cfg, mask_word_id=S.MASK_ID, eos_id=S.SEP_ID, enable_butd=True, len_vis_input=100, length_penalty=0.4, **kw)
    sd = dict(p)
    sd["cls.predictions.decoder.weight"] = p["bert.embeddings.word_embeddings.weight"]
    m.load_state_dict(sd, strict=True)
    return m.half().to(torch.device(device)).eval()


def search(m, device, constraints=None, **attrs):
    import torch
    for k, v in attrs.items():
        setattr(m, k, v)
    with torch.no_grad():
        tr = m(*model_inputs(device)[2], task_idx=None, **({} if constraints is None else {"constraints": constraints}))
    return {k: v.cpu() for k, v in tr.items()}


def equal_dicts(a, b):
    import torch
    from tests import guard_util as GU
    return set(a) == set(b) and all(a[k].dtype == b[k].dtype and torch.equal(GU.bits(a[k]), GU.bits(b[k])) for k in a)
