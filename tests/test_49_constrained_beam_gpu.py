"""GPU: constrained beam search on the device (vlp_logsoftmax_topk_want, vlp_beam_select_constrained, Engine.decode_beam(constraints=,
constrained_select=), BertForSeq2SeqDecoder.forward(constraints=), python -m vlp_amd.decode_img2txt --constraints_file).

  * vlp_logsoftmax_topk_want against the existing top-K entry points (bit-equal lists) and torch.log_softmax (the wanted values);
  * vlp_beam_select_constrained against vlp_amd.constrained.beam_select_constrained_host on frames built to hurt: all eight outputs bit
    for bit, guard bands; constraints of length 0 against vlp_beam_select; refusals without a launch;
  * the model: the device selection equals the host path, constraints=None and empty lists are the decoder as it was, the structure of the
    traces, satisfaction, run / capture / replay with other constraints at the same shapes;
  * the command line.
"""
import functools
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from oracle import vlp_oracle as O                                  # noqa: E402  (checker: the parameters of a small model)
from tests import constrained_util as U                             # noqa: E402
from tests import guard_util as GU                                  # noqa: E402
from vlp_amd import _lib as K_                                      # noqa: E402
from vlp_amd import constrained as CB                               # noqa: E402
from vlp_amd import decode_img2txt as D                             # noqa: E402
from vlp_amd import eval_captions as EC                             # noqa: E402
from vlp_amd import synthetic as S                                  # noqa: E402
from vlp_amd.data import write_packed                               # noqa: E402
from vlp_amd.modeling import BertConfig                             # noqa: E402

DEV = torch.device("cuda:0")
EOS = U.EOS

# ------------------------------------------------------------------------------------------------
# vlp_logsoftmax_topk_want
# ------------------------------------------------------------------------------------------------
# (rows, V, K, C, ld): K <= 4 / <= 8 / <= 16 take the three register-list kernels, K = 50 and the odd pitch the scalar K+2-pass kernel
TOPK_SHAPES = [(5, 1000, 3, 2, 1024), (2, 50, 50, 8, 64), (3, 100, 16, 4, 128), (7, 28996, 8, 1, 29056), (4, 300, 5, 3, 301)]
TOPK_EOS = 7


@functools.lru_cache(maxsize=None)
def topk_case(rows, V, Kb, C, ld):
    """Logits, a dense forbid mask, the same words as lists, and wanted ids: per row some of the row's own top K, some forbidden words, the
    eos (blocked when block_eos is on), a -1 and random words.  Computed once, read only."""
    g = torch.Generator().manual_seed(V + Kb)
    logits = (torch.randn(rows, ld, generator=g) * 3).half()
    logits[:, V:] = 100.0                                            # the pitch padding: a stray read wins every maximum
    forbid = (torch.rand(rows, V, generator=g) < min(0.05, 40.0 / V)).to(torch.uint8)      # a list holds at most 1024 ids
    forbid[:, TOPK_EOS] = 0
    ref = torch.log_softmax(logits[:, :V].float(), dim=-1)
    top = torch.topk(ref, Kb, dim=-1).indices
    want = torch.randint(0, V, (rows, C), generator=g, dtype=torch.int32)
    pool = []
    for r in range(rows):
        fb = torch.nonzero(forbid[r]).reshape(-1).tolist()
        pool.append([int(top[r, 0]), fb[0] if fb else 0, TOPK_EOS, -1, int(top[r, Kb - 1]), fb[-1] if fb else 1])
    for r in range(rows):
        for c in range(C):
            if (r + c) % 8 < 6:                                      # C = 1: the rows take turns, so every kind occurs in every case
                want[r, c] = pool[r][(r + c) % 8]
    cnt = forbid.sum(1).to(torch.int32)
    lists = torch.full((rows, max(int(cnt.max()), 1) + 3), -7, dtype=torch.int32)
    for r in range(rows):
        lists[r, :int(cnt[r])] = torch.nonzero(forbid[r]).reshape(-1).to(torch.int32)
    return logits, forbid, lists, cnt, want, ref


@pytest.mark.parametrize("block_eos", [False, True])
@pytest.mark.parametrize("mode", ["none", "dense", "list"])
@pytest.mark.parametrize("shape", TOPK_SHAPES, ids=["r%d_V%d_K%d_C%d_ld%d" % s for s in TOPK_SHAPES])
def test_topk_want(shape, mode, block_eos):
    """The top-K outputs are those of vlp_logsoftmax_topk / _list bit for bit.  want_val: -inf for -1; the list's bits for a word of the
    row's list; within 2e-4 of torch.log_softmax (test_40's bound) where no penalty applies; exactly -10000 for the blocked eos.  A forbidden
    word is held to the bits of fl32(u + -10000.0f), u the unpenalised value of the same kernel (the no-forbid run, itself within 2e-4): fp32
    is 9.8e-4 apart at 1e4, so the sum cannot be held to 2e-4 of anything, and the kernel's expression can be held exactly."""
    rows, V, Kb, C, ld = shape
    logits, forbid, lists, cnt, want, ref = topk_case(*shape)
    lg = GU.guarded(rows, V, ld=ld, dtype=torch.float16, fill=100.0, device=DEV)
    lg.full.copy_(logits.to(DEV))
    lg.seal()
    d_forbid, d_lists, d_cnt, d_want = forbid.to(DEV), lists.to(DEV), cnt.to(DEV), want.to(DEV).contiguous()
    base_s, base_i = torch.zeros(rows, Kb, device=DEV), torch.zeros(rows, Kb, dtype=torch.long, device=DEV)
    if mode == "list":
        K_.logsoftmax_topk_list(lg.view, ld, rows, V, Kb, base_s, base_i, d_lists, d_cnt, eos_id=TOPK_EOS, block_eos=block_eos)
    else:
        K_.logsoftmax_topk(lg.view, ld, rows, V, Kb, base_s, base_i, forbid=d_forbid if mode == "dense" else None, eos_id=TOPK_EOS, block_eos=block_eos)
    g_s = GU.guarded(rows, Kb, dtype=torch.float32, fill="sentinel", device=DEV)
    g_i = GU.guarded(rows, Kb, dtype=torch.int64, fill="sentinel", device=DEV)
    g_w = GU.guarded(rows, C, dtype=torch.float32, fill="sentinel", device=DEV)
    kw = dict(forbid=d_forbid) if mode == "dense" else (dict(cand_ids=d_lists, cand_cnt=d_cnt) if mode == "list" else {})
    K_.logsoftmax_topk_want(lg.view, ld, rows, V, Kb, g_s.view, g_i.view, d_want, g_w.view, eos_id=TOPK_EOS, block_eos=block_eos, **kw)
    plain_w = torch.zeros(rows, C, device=DEV)                       # the unpenalised values of the same kernel
    K_.logsoftmax_topk_want(lg.view, ld, rows, V, Kb, torch.zeros_like(base_s), torch.zeros_like(base_i), d_want, plain_w, eos_id=TOPK_EOS,
                            block_eos=False)
    torch.cuda.synchronize()
    for g, name in ((g_s, "out_scores"), (g_i, "out_ids"), (g_w, "want_val")):
        GU.assert_untouched(g, written="logical", name=name)
        GU.assert_written(g, written="logical", name=name)
    GU.assert_untouched(lg, written=None, name="logits")
    assert torch.equal(GU.bits(g_s.view), GU.bits(base_s)) and torch.equal(g_i.view, base_i)
    got, plain, ids, sc = g_w.view.cpu(), plain_w.cpu(), base_i.cpu(), base_s.cpu()
    seen = dict(listed=0, forbidden=0, eos=0, none=0, free=0)
    for r in range(rows):
        for c in range(C):
            w = int(want[r, c])
            if w == -1:
                assert got[r, c] == -np.inf and plain[r, c] == -np.inf
                seen["none"] += 1
                continue
            assert abs(float(plain[r, c]) - float(ref[r, w])) < 2e-4, (r, c, w, float(plain[r, c]), float(ref[r, w]))
            hit = torch.nonzero(ids[r] == w).reshape(-1)
            if len(hit):                                             # a wanted word of the row's list carries the list's bits
                assert torch.equal(GU.bits(got[r, c]), GU.bits(sc[r, int(hit[0])])), (r, c, w)
                seen["listed"] += 1
            if block_eos and w == TOPK_EOS:
                assert float(got[r, c]) == -10000.0
                seen["eos"] += 1
            elif mode != "none" and bool(forbid[r, w]):
                assert torch.equal(GU.bits(got[r, c]), GU.bits(plain[r, c] + torch.tensor(-10000.0))), (r, c, w)
                seen["forbidden"] += 1
            else:
                assert torch.equal(GU.bits(got[r, c]), GU.bits(plain[r, c]))
                seen["free"] += 1
    assert seen["listed"] and seen["none"] and seen["free"] and (mode == "none" or seen["forbidden"]) and (not block_eos or seen["eos"]), seen


def test_topk_want_refusals():
    rows, V, Kb, C = 2, 64, 3, 2
    lg = torch.zeros(rows, 64, dtype=torch.float16, device=DEV)
    s, i = torch.zeros(rows, Kb, device=DEV), torch.zeros(rows, Kb, dtype=torch.long, device=DEV)
    want, wv = torch.zeros(rows, C, dtype=torch.int32, device=DEV), GU.guarded(rows, C, dtype=torch.float32, fill="sentinel", device=DEV)
    fb = torch.zeros(rows, V, dtype=torch.uint8, device=DEV)
    li, lc = torch.zeros(rows, 4, dtype=torch.int32, device=DEV), torch.zeros(rows, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="vlp_logsoftmax_topk_want"):      # the two forbid forms exclude each other
        K_.logsoftmax_topk_want(lg, 64, rows, V, Kb, s, i, want, wv.view, forbid=fb, cand_ids=li, cand_cnt=lc)
    with pytest.raises(RuntimeError, match="vlp_logsoftmax_topk_want"):      # C outside 1..8
        K_.logsoftmax_topk_want(lg, 64, rows, V, Kb, s, i, torch.zeros(rows, 9, dtype=torch.int32, device=DEV), torch.zeros(rows, 9, device=DEV))
    torch.cuda.synchronize()
    GU.assert_untouched(wv, written=None, name="want_val")


# ------------------------------------------------------------------------------------------------
# vlp_beam_select_constrained against the host specification
# ------------------------------------------------------------------------------------------------
SHAPES = [(1, 2, 1, 1), (3, 5, 2, 3), (4, 3, 4, 2), (2, 64, 8, 8)]
NAMES = ("out_scores", "out_ids", "out_ptrs", "out_eos", "src_rows", "next_ids", "out_state", "want_next")


@functools.lru_cache(maxsize=None)
def frame(B, K, C, Lc, first):
    return U.hostile_frame(B, K, C, Lc, bool(first), 1000 * K + 10 * B + int(first))


@functools.lru_cache(maxsize=None)
def host(B, K, C, Lc, first, last=0):
    """The specification's eight arrays and its trace for a case; computed once, read only."""
    tr = {}
    out = U.host_select(frame(B, K, C, Lc, first), first, tr, last=bool(last))
    for a in out:
        a.setflags(write=False)
    return out, tr


def put(a, fill):
    dt = {np.dtype(np.float32): torch.float32, np.dtype(np.int64): torch.int64, np.dtype(np.int32): torch.int32}[a.dtype]
    return GU.guarded_vec(a.size, dt, fill, device=DEV).set(torch.from_numpy(np.array(a)).to(DEV))


def device_inputs(fr):
    """The float inputs sit between NaN guards, ids and states between guards that hold a valid word / the state 0."""
    return {k: None if fr[k] is None else put(fr[k], "nan" if fr[k].dtype == np.float32 else (5 if k in ("ki", "want", "cid") else 0)) for k in fr}


def guarded_outputs(B, K, C):
    R = B * K
    return (GU.guarded_vec(R, torch.float32, "sentinel", device=DEV), GU.guarded_vec(R, torch.int64, "sentinel", device=DEV),
            GU.guarded_vec(R, torch.int64, "sentinel", device=DEV), GU.guarded_vec(R, torch.float32, "sentinel", device=DEV),
            GU.guarded_vec(R, torch.int64, "sentinel", device=DEV),
            GU.guarded(R, 1, ld=2, dtype=torch.int64, fill="sentinel", device=DEV),     # the engine's xids[:, 0]: stride 2
            GU.guarded_vec(R, torch.int32, "sentinel", device=DEV), GU.guarded_vec(R * C, torch.int32, "sentinel", device=DEV))


def launch(ins, outs, B, K, C, Lc, first, drop=(), plain=False, last=0):
    v = {k: (None if g is None or k in drop else g.vec) for k, g in ins.items()}
    o = [None if n in drop else (g.view[:, 0] if n == "next_ids" else g.vec) for n, g in zip(NAMES, outs)]
    args = (v["ks"], v["ki"], v["lt"], v["le"], o[0], o[1], o[2], o[3], o[4], o[5], B, K, bool(first), EOS)
    if plain:
        K_.beam_select(*args)
    else:
        K_.beam_select_constrained(*args, v["want"], v["wv"], v["ps"], v["cid"], v["cln"], C, Lc, o[6], o[7], last=bool(last))


def read(outs):
    return [GU.bits(g.view).cpu().numpy().reshape(-1) for g in outs]


def same_bits(got, want):
    return np.array_equal(got, np.ascontiguousarray(want).reshape(-1).view(got.dtype))


@pytest.mark.parametrize("last", [0, 1])
@pytest.mark.parametrize("first", [0, 1])
@pytest.mark.parametrize("B,K,C,Lc", SHAPES, ids=["B%d_K%d_C%d_Lc%d" % s for s in SHAPES])
def test_kernel_equals_the_host_specification(B, K, C, Lc, first, last):
    want, _ = host(B, K, C, Lc, first, last)
    ins = device_inputs(frame(B, K, C, Lc, first))
    runs = []
    for _ in range(2):
        outs = guarded_outputs(B, K, C)
        launch(ins, outs, B, K, C, Lc, first, last=last)
        torch.cuda.synchronize()
        for g, name in zip(outs, NAMES):
            GU.assert_untouched(g, written="logical", name=name)
            GU.assert_written(g, written="logical", name=name)
        runs.append(read(outs))
    for k, g in ins.items():
        if g is not None:
            GU.assert_untouched(g, written=None, name=k)
    for name, a, w in zip(NAMES, runs[0], want[:5] + (want[5][:, 0],) + want[6:]):
        assert same_bits(a, w), (name, a, np.asarray(w).reshape(-1))
    assert all(np.array_equal(a, b) for a, b in zip(*runs)), "two launches differ"


def test_hostile_frames_reach_what_they_are_for():
    """Taken together the cases hold unmet eos candidates, dropped phrases, cursor wraps, dead picks, ties, -inf picks, NaN and +inf among
    the candidates (a NaN orders as -inf and is picked last of its bank), and last frames that change the picks."""
    tot = dict(unmet_eos=0, dropped=0, wraps=0, dead_picks=0)
    ties = minus_inf = nan = plus_inf = last_changes = 0
    for shape in SHAPES:
        for first in (0, 1):
            out, tr = host(*shape, first)
            for k in tot:
                tot[k] += tr[k]
            sc = out[0]
            ties += int((sc[:, 1:] == sc[:, :-1]).sum())
            minus_inf += int(np.isneginf(sc).sum())
            fr = frame(*shape, first)
            nan += int(np.isnan(fr["ks"]).sum() + np.isnan(fr["wv"]).sum())
            plus_inf += int(np.isposinf(fr["ks"]).sum())
            last_changes += int(not np.array_equal(host(*shape, first, 1)[0][1], out[1]))
    assert min(tot.values()) >= 1 and ties >= 10 and minus_inf >= 1 and nan >= 1 and plus_inf >= 1 and last_changes >= 3, \
        (tot, ties, minus_inf, nan, plus_inf, last_changes)
    fr = frame(3, 5, 2, 3, 0)
    assert fr["le"][1].all() and not fr["cln"][2].any() and fr["cln"][0].sum() == 6      # only ended parents; no phrase; Tb = C * Lc


@pytest.mark.parametrize("first", [0, 1])
def test_no_constraints_equals_vlp_beam_select(first):
    """Every cons_len == 0 (the images of a batch without an entry): the six outputs are vlp_beam_select's bits, the states stay 0 and nothing
    is wanted.  Scores of a search: finite log-probabilities, ended parents at -10000."""
    B, K, C, Lc = 3, 5, 2, 3
    rng = np.random.RandomState(7 + first)
    R = 1 if first else K
    fr = dict(ks=-np.sort(rng.randint(0, 40, size=(B, R, K)) * U.F32(0.25), axis=-1).astype(U.F32), ki=rng.randint(0, 12, size=(B, R, K)).astype(np.int64),
              want=np.full((B, R, C), -1, np.int32), wv=np.full((B, R, C), -np.inf, U.F32),
              lt=None if first else (-rng.randint(0, 40, size=(B, K)) * U.F32(0.25)).astype(U.F32),
              le=None if first else (rng.rand(B, K) < 0.3).astype(U.F32), ps=None if first else np.zeros((B, K), np.int32),
              cid=rng.randint(0, 12, size=(B, C, Lc)).astype(np.int32), cln=np.zeros((B, C), np.int32))
    ins = device_inputs(fr)
    a, b = guarded_outputs(B, K, C), guarded_outputs(B, K, C)
    launch(ins, a, B, K, C, Lc, first)
    launch(ins, b, B, K, C, Lc, first, plain=True)
    torch.cuda.synchronize()
    ra, rb = read(a), read(b)
    for name, x, y in zip(NAMES[:6], ra, rb):
        assert np.array_equal(x, y), name
    assert not ra[6].any() and (ra[7] == -1).all()


@pytest.mark.parametrize("what", ["null_scores", "null_want", "null_val", "null_cons", "null_len", "null_state_out", "null_want_next", "null_next",
                                  "B_zero", "K_zero", "K_65", "C_zero", "C_9", "Lc_zero", "Lc_9", "no_last_total", "no_last_eos", "no_prev_state"])
def test_refusals_launch_nothing(what):
    B, K, C, Lc = 2, 4, 2, 2
    fr = frame(3, 5, 2, 3, 0)                  # any buffers large enough: nothing is read
    ins = device_inputs(fr)
    outs = guarded_outputs(3, 5, 2)
    drop = {"null_scores": ("ks",), "null_want": ("want",), "null_val": ("wv",), "null_cons": ("cid",), "null_len": ("cln",),
            "null_state_out": ("out_state",), "null_want_next": ("want_next",), "null_next": ("next_ids",), "no_last_total": ("lt",),
            "no_last_eos": ("le",), "no_prev_state": ("ps",)}.get(what, ())
    B = 0 if what == "B_zero" else B
    K = {"K_zero": 0, "K_65": 65}.get(what, K)
    C = {"C_zero": 0, "C_9": 9}.get(what, C)
    Lc = {"Lc_zero": 0, "Lc_9": 9}.get(what, Lc)
    with pytest.raises(RuntimeError, match="vlp_beam_select_constrained"):
        launch(ins, outs, B, K, C, Lc, 0, drop=drop)
    torch.cuda.synchronize()
    for g, name in zip(outs, NAMES):
        GU.assert_untouched(g, written=None, name=name)


# ------------------------------------------------------------------------------------------------
# the model
# ------------------------------------------------------------------------------------------------
NB, NT = U.NB, U.NT
TRACES = ("pred_seq", "scores", "wids", "ptrs")
NBEST = ("nbest_seq", "nbest_score", "nbest_value", "nbest_len", "nbest_ok")
DEVS = "cuda:0"
# image 0: one phrase of two pieces; image 1: two single pieces, one of them the first piece of image 0's phrase; image 2: nothing
CONS = [[[300, 301]], [[300], [411]], []]


def make_model(**kw):
    return U.make_model(DEVS, **kw)


def search(m, constraints=None, **attrs):
    return U.search(m, DEVS, constraints, **attrs)


def check_structure(tr, m, cons):
    """cons_state is the state recomputed by walking every hypothesis; a hypothesis whose last word is eos, or that stands in the last frame,
    (and that is not a dead pick: its score carries no -10000) has met all its phrases; pred_met is constraints_met of pred_seq.  Returns
    how many hypotheses were held to that."""
    ci, cl = CB.pack_constraints(cons, NB) if isinstance(cons, list) else cons
    wids, ptrs, sc, st = (tr[k][:, :NT].numpy() for k in ("wids", "ptrs", "scores", "cons_state"))
    ended_met = 0
    for b in range(NB):
        assert np.array_equal(st[b], U.walk_states(wids[b], ptrs[b], m.eos_id, ci[b], cl[b])), b
        full = CB.full_mask(cl[b])
        for s in range(NT):
            for k in range(wids.shape[2]):
                if (wids[b, s, k] == m.eos_id or s == NT - 1) and sc[b, s, k] > -5000.0:
                    assert (st[b, s, k] & 0xFF) == full, (b, s, k)
                    ended_met += 1
        assert int(tr["pred_met"][b]) == CB.constraints_met(tr["pred_seq"][b].numpy(), ci[b], cl[b], eos_id=m.eos_id)
        if "nbest_met" in tr:
            for n in range(tr["nbest_seq"].shape[1]):
                assert int(tr["nbest_met"][b, n]) == CB.constraints_met(tr["nbest_seq"][b, n].numpy(), ci[b], cl[b], eos_id=m.eos_id)
    assert not tr["cons_state"][:, NT:].any()
    return ended_met


@pytest.mark.parametrize("K,n_best,extra", [(3, 1, U.PLAIN), (5, 1, U.PLAIN), (3, 1, U.BLOCKED), (5, 5, U.BLOCKED), (5, 3, dict(U.PLAIN, min_len=2))],
                         ids=["K3", "K5", "K3_ngram_min_len_3", "K5_ngram_min_len_3_nbest", "K5_min_len_2_nbest"])
def test_device_selection_equals_the_host_path(K, n_best, extra):
    m = make_model(search_beam_size=K, n_best=n_best, **extra)
    assert m.constrained_select == "device" and m.ngram_blocking == "device"
    on_host = search(m, CONS, constrained_select="host")
    on_dev = search(m, CONS, constrained_select="device")
    want_keys = set(TRACES) | {"cons_state", "pred_met"} | (set(NBEST) | {"nbest_met"} if n_best > 1 else set())
    assert set(on_dev) == want_keys and U.equal_dicts(on_dev, on_host)
    assert check_structure(on_host, m, CONS) >= NB and check_structure(on_dev, m, CONS) >= NB      # every image ends with one at least
    plain = search(make_model(search_beam_size=K, n_best=n_best, **extra))
    assert not torch.equal(plain["wids"], on_dev["wids"])                      # the constraints do something
    assert torch.equal(plain["wids"][2], on_dev["wids"][2]) and torch.equal(GU.bits(plain["scores"][2]), GU.bits(on_dev["scores"][2]))   # not to image 2


def test_no_constraints_is_the_decoder_as_it_was():
    for extra in (U.PLAIN, U.BLOCKED):
        m = make_model(search_beam_size=4, n_best=4, **extra)
        plain = search(make_model(search_beam_size=4, n_best=4, **extra))
        assert U.equal_dicts(search(m, None), plain) and set(plain) == set(TRACES + NBEST)
        empty = search(m, [[], [], []])
        assert not empty["cons_state"].any() and not empty["pred_met"].any() and not empty["nbest_met"].any()
        assert U.equal_dicts({k: empty[k] for k in plain}, plain)
        pair = search(m, (np.zeros((NB, 2, 3), np.int32), np.zeros((NB, 2), np.int32)))
        assert U.equal_dicts({k: pair[k] for k in plain}, plain)
    m = make_model(search_beam_size=4, beam_groups=2, diversity_penalty=0.5)
    with pytest.raises(ValueError, match="exclude each other"), torch.no_grad():
        m(*U.model_inputs(DEVS)[2], task_idx=None, constraints=CONS)
    with pytest.raises(ValueError, match="exclude each other"):
        m.engine.decode_beam(*U.model_inputs(DEVS)[2], S.MASK_ID, 4, S.SEP_ID, groups=2, diversity=0.5, constraints=CB.pack_constraints(CONS, NB))
    m = make_model(search_beam_size=4)
    for bad, msg in (([[[S.SEP_ID]], [], []], "end-of-sequence"), ([[[5000]], [], []], "outside the vocabulary"), ([[], []], "entries")):
        with pytest.raises(ValueError, match=msg), torch.no_grad():
            m(*U.model_inputs(DEVS)[2], task_idx=None, constraints=bad)
    with pytest.raises(ValueError, match="constrained_select"):
        search(m, CONS, constrained_select="gpu")
    with pytest.raises(ValueError, match="search_beam_size >= 2"), torch.no_grad():
        make_model(search_beam_size=1)(*U.model_inputs(DEVS)[2], task_idx=None, constraints=CONS)


def test_constraints_are_satisfied():
    """Per image one or two word pieces that its unconstrained best caption does not contain (the first ids from 300 + 50 b on that are not in
    it), K = 4 >= Tb + 1 = 3, six tokens of room: every phrase of every image is met, on the host path first, then on the device."""
    plain = search(make_model(search_beam_size=4, **U.PLAIN))
    cons = []
    for b in range(NB):
        used = set(plain["pred_seq"][b].tolist())
        free = [w for w in range(300 + 50 * b, 400 + 50 * b) if w not in used]
        cons.append([[free[0], free[1]]] if b == 0 else ([[free[0]], [free[1]]] if b == 1 else [[free[0]]]))
    ci, cl = CB.pack_constraints(cons, NB)
    m = make_model(search_beam_size=4, **U.PLAIN)
    for where in ("host", "device"):
        tr = search(m, cons, constrained_select=where)
        print(where, "pred_seq", tr["pred_seq"][:, :NT].tolist(), "pred_met", tr["pred_met"].tolist())
        assert tr["pred_met"].tolist() == [CB.full_mask(cl[b]) for b in range(NB)], where
        for b in range(NB):
            seq = tr["pred_seq"][b].tolist()
            for ph in cons[b]:
                assert any(seq[i:i + len(ph)] == ph for i in range(len(seq))), (b, ph, seq)
        check_structure(tr, m, cons)


def test_run_capture_replay_and_other_constraints_at_the_same_shapes():
    """Call 1 (run), 2 (captured) and 3 (replayed) return the same bits; a call with other constraints of the same (C, Lc) -- which replays the
    same graphs -- returns what a fresh decoder returns: the captured launches read the workspace's copies, not the first caller's tensors;
    a plain search on the used decoder afterwards is a fresh decoder's."""
    other = [[[520], [300]], [[301, 300]], [[640]]]
    assert CB.pack_constraints(other, NB)[0].shape == CB.pack_constraints(CONS, NB)[0].shape
    kw = dict(search_beam_size=4, n_best=4, **U.BLOCKED)
    fresh_a, fresh_b, fresh_plain = search(make_model(**kw), CONS), search(make_model(**kw), other), search(make_model(**kw))
    assert not U.equal_dicts(fresh_a, fresh_b)
    used = make_model(**kw)
    pair = tuple(torch.from_numpy(a).to(DEV) for a in CB.pack_constraints(CONS, NB))       # device tensors of the caller, overwritten below
    for rep in range(3):
        assert U.equal_dicts(search(used, pair), fresh_a), rep
    pair[0].fill_(777)
    assert U.equal_dicts(search(used, other), fresh_b)
    assert U.equal_dicts(search(used, CONS), fresh_a)
    assert U.equal_dicts(search(used), fresh_plain)
    assert U.equal_dicts(search(used, other), fresh_b)


# ------------------------------------------------------------------------------------------------
# python -m vlp_amd.decode_img2txt --constraints_file
# ------------------------------------------------------------------------------------------------
NV, TC, VOCAB = 100, 8, 1024
LIST = [("test", 391895), ("val", 522418), ("test", 184613), ("test", 318219)]


def fname(i):
    return "COCO_val2014_%012d.jpg" % i


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    """A packed store of 3 images, a 2-layer checkpoint, a vocabulary and a Karpathy-style image list with references."""
    root = str(tmp_path_factory.mktemp("constrained_cli"))
    rng = np.random.RandomState(9)
    test_ids = [i for sp, i in LIST if sp == "test"]
    n = len(test_ids)
    keys = [fname(i)[:-4] for i in reversed(test_ids)]
    feats = np.abs(rng.randn(n, NV, 2048)).astype(np.float16)
    cls = rng.rand(n, NV, 1601).astype(np.float32)
    cls /= cls.sum(-1, keepdims=True)
    xy = rng.rand(n, NV, 2, 2) * 400
    boxes = np.concatenate([xy.min(2), xy.max(2) + 1.0, np.zeros((n, NV, 1)), rng.rand(n, NV, 1)], axis=-1).astype(np.float32)
    store = os.path.join(root, "store")
    write_packed(store, keys, feats, cls, boxes)
    bert = os.path.join(root, "bert")
    os.makedirs(bert)
    with open(os.path.join(bert, "bert_config.json"), "w") as f:
        f.write(BertConfig(VOCAB, num_hidden_layers=2, type_vocab_size=2).to_json_string())
    special = {S.PAD_ID: "[PAD]", S.UNK_ID: "[UNK]", S.CLS_ID: "[CLS]", S.SEP_ID: "[SEP]", S.MASK_ID: "[MASK]"}
    with open(os.path.join(bert, "vocab.txt"), "w") as f:
        f.write("\n".join(special.get(i, "w%d" % i if i < 900 else "##p%d" % i) for i in range(VOCAB)) + "\n")
    p = O.init_params(vocab_size=VOCAB, layers=2, tasks="img2txt", seed=27, std=0.1)
    sd = dict(p)
    sd["cls.predictions.decoder.weight"] = p["bert.embeddings.word_embeddings.weight"]
    ckpt = os.path.join(root, "model.3.bin")
    torch.save(sd, ckpt)
    src = os.path.join(root, "dataset.json")
    with open(src, "w") as f:
        json.dump({"images": [{"split": sp, "filename": fname(i), "filepath": "val2014", "imgid": k,
                               "sentences": [{"tokens": ["w%d" % t for t in rng.randint(300, 340, size=5)]} for _ in range(2)]}
                              for k, (sp, i) in enumerate(LIST)]}, f)
    return dict(root=root, store=store, bert=bert, ckpt=ckpt, src=src, test_ids=test_ids)


def run(su, name, *extra):
    out = os.path.join(su["root"], name)
    res = D.main(["--bert_model", su["bert"], "--model_recover_path", su["ckpt"], "--packed_features", su["store"], "--src_file", su["src"],
                  "--split", "test", "--dataset", "coco", "--output_file", out, "--batch_size", "2", "--beam_size", "4", "--forbid_duplicate_ngrams",
                  "--ngram_size", "2", "--min_len", "2", "--max_tgt_length", str(TC), "--new_segment_ids", "--fp16", "--enable_butd"] + list(extra))
    with open(out) as f:
        text = f.read()
    assert res == {su["ckpt"]: json.loads(text)}
    return text


def test_cli_constraints_file(setup):
    """Without the flag the records are {image_id, caption} as ever, and a file that constrains no image of the split changes nothing but
    the two added keys; with phrases (text that needs the WordPiece split, and ids) the records carry them and what was met, the captions
    contain the met phrases, and eval_captions reads the file."""
    su = setup
    plain = run(su, "plain.json")
    assert [set(r) for r in json.loads(plain)] == [{"image_id", "caption"}] * 3
    ids = su["test_ids"]
    none = os.path.join(su["root"], "none.json")
    with open(none, "w") as f:
        json.dump({"1": [[300]]}, f)                                                    # no image of the split
    got = json.loads(run(su, "none_out.json", "--constraints_file", none))
    assert [{k: r[k] for k in ("image_id", "caption")} for r in got] == json.loads(plain)
    assert all(r["constraints"] == [] and r["met"] == [] for r in got)
    cons = os.path.join(su["root"], "cons.json")
    with open(cons, "w") as f:
        json.dump({str(ids[0]): ["w350p901"], str(ids[2]): [[360], "w370 w371"]}, f)    # w350 + ##p901: greedy longest match
    out = os.path.join(su["root"], "cons_out.json")
    nb = os.path.join(su["root"], "cons_nbest.json")
    got = json.loads(run(su, "cons_out.json", "--constraints_file", cons, "--n_best", "2", "--nbest_file", nb))
    assert [r["image_id"] for r in got] == ids
    assert [r["constraints"] for r in got] == [[[350, 901]], [], [[360], [370, 371]]]
    assert got[1]["met"] == [] and got[1]["caption"] == json.loads(plain)[1]["caption"]
    print("met", [r["met"] for r in got], "captions", [r["caption"] for r in got])
    for r in got:
        for ph, met in zip(r["constraints"], r["met"]):
            text = " ".join(D.merge_word_pieces(["w%d" % t if t < 900 else "##p%d" % t for t in ph]))
            assert met == (text in r["caption"]), (r, text)
    assert any(any(r["met"]) for r in got)
    ids_read, hyps_read = EC.load_predictions(out, EC.references_of(su["src"], "test", "coco"))       # what eval_captions reads
    assert ids_read == ids and len(hyps_read) == 3
    with open(nb) as f:
        listed = json.load(f)
    assert all("constraints" in r and len(r["met"]) == len(r["constraints"]) for r in listed)
