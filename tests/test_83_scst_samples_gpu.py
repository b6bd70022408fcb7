"""GPU: self-critical training with K samples per image and a leave-one-out baseline (--scst_samples K).

(a) vlp_cider_d_multi / vlp_cider_d_multi_df (csrc/reward.hip) against the fp64 host class (scst_df_util.host_scores) on seeded corpora, with
    the call's own document frequencies and with a table: scores within the project's (4 T + 16) * 2^-24 * 10, leave-one-out rewards within
    2 * that + (mult + 1) * 2^-24 * 10 (tests/scst_samples_util.py says why).  Asserted on the host scorer alone first: every score and every
    reward of the listed shapes is non-zero.  mult == 2 against the existing entries bit for bit, repeats, guard bands, garbage behind a
    row's end and in invalid reference rows, refusals before any launch, the old entries' refusal of mult 3;
(b) vlp_sample_rows_rep (csrc/elementwise.hip) against vlp_sample_rows bit for bit, the second id output, padding, distinct draws of one
    logits row, the distribution;
(c) Engine.decode_sample_group: one sample per image equals decode_greedy(sample=True) bit for bit; four samples per image over the plain
    call, the capturing call and the replaying call against a teacher-forced oracle;
(d) the train-mode forward with n_samples = 3 against score_samples on tiled inputs and the oracle's gradients; the entry script.
Every test prints what it measured (pytest -s)."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from oracle import vlp_oracle as O                                  # noqa: E402  (checker only)
from tests import guard_util as GU                                  # noqa: E402
from tests import scst_df_util as U                                 # noqa: E402
from tests import scst_samples_util as SU                           # noqa: E402
from vlp_amd import _lib as K                                       # noqa: E402
from vlp_amd import scst as SC                                      # noqa: E402
from vlp_amd import synthetic as S                                  # noqa: E402
from vlp_amd.input_prep import CaptionRefs                          # noqa: E402

DEV = torch.device("cuda:0")
REPORT = {}


def report(key, **kw):
    REPORT.setdefault(key, {}).update(kw)
    print("%s: %s" % (key, json.dumps(REPORT[key], sort_keys=True)))


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def run_multi(hyp, ref, count, mult, tab=None, workspace=None):
    """(scores [mult*G], reward [mult*G]) of vlp_cider_d_multi (tab None) or vlp_cider_d_multi_df, on the CPU."""
    G = ref.shape[0]
    h, r = torch.from_numpy(hyp).to(DEV), torch.from_numpy(ref).to(DEV)
    c = torch.from_numpy(count).to(DEV) if count is not None else None
    scores = torch.full((mult * G,), float("nan"), device=DEV)
    reward = torch.full((mult * G,), float("nan"), device=DEV)
    if tab is None:
        K.cider_d_multi(h, r, c, mult, scores, reward, workspace=workspace)
    else:
        keys, vals = tab.to(DEV)
        K.cider_d_multi_df(h, r, c, mult, scores, keys, vals, tab.n_docs, reward, workspace=workspace)
    torch.cuda.synchronize()
    return scores.cpu(), reward.cpu()


def _tab(T, mode):
    return U.table(T, 0) if mode == "table" else None


# ---- (a) reward kernels ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,seed", SU.SHAPES, ids=["G%d_R%d_T%d_m%d" % s for s, _ in SU.SHAPES])
@pytest.mark.parametrize("mode", ["batch", "table"])
def test_kernels_against_host_scorer(shape, seed, mode):
    G, R, T, mult = shape
    hyp, ref, count = U.make_corpus(G, R, T, mult, seed)
    tab = _tab(T, mode)
    want = U.host_scores(hyp, ref, count, mult, df=tab if tab is not None else "corpus")
    want_r = SU.loo(want, mult)
    # on the host scorer alone, before the kernel's output is looked at
    nz_s, nz_r = float(np.mean(want != 0)), float(np.mean(want_r != 0))
    assert nz_s == 1.0 and nz_r >= 0.5, (nz_s, nz_r)
    got, reward = run_multi(hyp, ref, count, mult, tab)
    e_s = float(np.abs(got.double().numpy() - want).max())
    e_r = float(np.abs(reward.double().numpy() - want_r).max())
    report("kernel_G%d_R%d_T%d_m%d_%s" % (shape + (mode,)), score_err=e_s, score_bound=SU.score_bound(T), reward_err=e_r,
           reward_bound=SU.reward_bound(T, mult), nonzero_scores=nz_s, nonzero_rewards=nz_r, max_score=float(want.max()))
    assert e_s <= SU.score_bound(T), (e_s, SU.score_bound(T))
    assert e_r <= SU.reward_bound(T, mult), (e_r, SU.reward_bound(T, mult))
    # the reward is the stated fp32 expression of the kernel's own scores, bit for bit
    assert same_bits(reward, torch.from_numpy(SU.loo(got.numpy(), mult)))


@pytest.mark.parametrize("shape,seed,mode", [(s, sd, m) for s, sd, modes in SU.EXTRA for m in modes] + [((1, 1, 4, 3), 1, "batch")],
                         ids=lambda v: v if isinstance(v, str) else ("G%d_R%d_T%d_m%d" % v if isinstance(v, tuple) else "s%d" % v))
def test_kernels_extra_shapes_rewards(shape, seed, mode):
    G, R, T, mult = shape
    hyp, ref, count = U.make_corpus(G, R, T, mult, seed)
    tab = _tab(T, mode)
    want = U.host_scores(hyp, ref, count, mult, df=tab if tab is not None else "corpus")
    want_r = SU.loo(want, mult)
    got, reward = run_multi(hyp, ref, count, mult, tab)
    if G == 1 and mode == "batch":                    # one group: every idf is log(mult) - log(mult) = 0
        assert not want.any()
        assert not got.numpy().any() and not reward.numpy().any()
        return
    assert float(np.mean(want_r != 0)) >= 0.5, want_r
    e_r = float(np.abs(reward.double().numpy() - want_r).max())
    report("extra_G%d_R%d_T%d_m%d_%s" % (shape + (mode,)), reward_err=e_r, reward_bound=SU.reward_bound(T, mult))
    assert e_r <= SU.reward_bound(T, mult), (e_r, SU.reward_bound(T, mult))


@pytest.mark.parametrize("mode", ["batch", "table"])
def test_two_hypotheses_equal_the_existing_entries_and_repeat(mode):
    G, R, T, mult = 5, 3, 21, 2
    hyp, ref, count = U.make_corpus(G, R, T, mult, 0)
    tab = _tab(T, mode)
    h, r, c = torch.from_numpy(hyp).to(DEV), torch.from_numpy(ref).to(DEV), torch.from_numpy(count).to(DEV)
    old_s, old_r = torch.zeros(2 * G, device=DEV), torch.zeros(G, device=DEV)
    if tab is None:
        K.cider_d(h, r, c, 2, old_s, old_r)
    else:
        K.cider_d_df(h, r, c, 2, old_s, *tab.to(DEV), tab.n_docs, old_r)
    new_s, new_r = run_multi(hyp, ref, count, 2, tab)
    assert old_r.cpu().numpy().any()
    assert same_bits(new_s, old_s.cpu())
    assert same_bits(new_r[:G], old_r.cpu()) and torch.equal(new_r[G:], -new_r[:G])
    again_s, again_r = run_multi(hyp, ref, count, 2, tab)
    assert same_bits(again_s, new_s) and same_bits(again_r, new_r)
    # a repeat at mult 5 as well
    hyp5, ref5, count5 = U.make_corpus(G, R, T, 5, 2)
    a, b = run_multi(hyp5, ref5, count5, 5, tab), run_multi(hyp5, ref5, count5, 5, tab)
    assert same_bits(a[0], b[0]) and same_bits(a[1], b[1])


@pytest.mark.parametrize("mode", ["batch", "table"])
def test_guard_bands(mode):
    G, R, T, mult = 5, 3, 21, 5
    hyp, ref, count = U.make_corpus(G, R, T, mult, 2)
    tab = _tab(T, mode)
    plain_s, plain_r = run_multi(hyp, ref, count, mult, tab)
    gh = GU.guarded(mult * G, T, ld=T + 5, dtype=torch.int64, fill=1000, device=DEV).set(torch.from_numpy(hyp).to(DEV))
    r, c = torch.from_numpy(ref).to(DEV), torch.from_numpy(count).to(DEV)
    need = (K.cider_d_multi_workspace_bytes if tab is None else K.cider_d_multi_df_workspace_bytes)(G, R, T, mult)
    assert need > 0 and K.cider_d_workspace_bytes(G, R, T, mult) == 0 and K.cider_d_df_workspace_bytes(G, R, T, mult) == 0
    gs = GU.guarded_vec(mult * G, dtype=torch.float32, fill="sentinel", device=DEV)
    gw = GU.guarded_vec(mult * G, dtype=torch.float32, fill="sentinel", device=DEV)
    ws = GU.guarded_vec(need, dtype=torch.uint8, fill="sentinel", device=DEV)
    if tab is None:
        K.cider_d_multi(gh.view, r, c, mult, gs.vec, gw.vec, workspace=ws.vec)
    else:
        K.cider_d_multi_df(gh.view, r, c, mult, gs.vec, *tab.to(DEV), tab.n_docs, gw.vec, workspace=ws.vec)
    torch.cuda.synchronize()
    for g, name, written in ((gs, "scores", "logical"), (gw, "reward", "logical"), (ws, "workspace", "logical"), (gh, "hyp", None)):
        GU.assert_untouched(g, written=written, name=name)
    GU.assert_written(gs, name="scores")
    GU.assert_written(gw, name="reward")
    assert same_bits(gs.vec.cpu(), plain_s) and same_bits(gw.vec.cpu(), plain_r)


@pytest.mark.parametrize("mode", ["batch", "table"])
def test_garbage_behind_the_end_and_in_invalid_rows_changes_nothing(mode):
    G, R, T, mult = 5, 3, 21, 5
    hyp, ref, count = U.make_corpus(G, R, T, mult, 2)
    tab = _tab(T, mode)
    clean = run_multi(hyp, ref, count, mult, tab)
    rng = np.random.RandomState(11)
    hyp2, ref2 = hyp.copy(), ref.copy()
    touched = 0
    for row in list(hyp2) + list(ref2.reshape(G * R, T)):
        z = np.flatnonzero(row == 0)
        if len(z) and z[0] + 1 < T:
            row[z[0] + 1:] = rng.randint(1000, 1012, size=T - z[0] - 1)
            touched += 1
    for g in range(G):
        for j in range(int(count[g]), R):
            ref2[g, j] = rng.randint(1000, 1012, size=T)
            touched += 1
    assert touched > G and int(count.min()) < R
    dirty = run_multi(hyp2, ref2, count, mult, tab)
    assert same_bits(clean[0], dirty[0]) and same_bits(clean[1], dirty[1])


REFUSALS = ["mult1", "mult17", "T65", "R9", "G0", "workspace_short"]


@pytest.mark.parametrize("what", REFUSALS)
@pytest.mark.parametrize("mode", ["batch", "table"])
def test_refusals_before_any_launch(what, mode):
    G, R, T, mult = {"mult1": (2, 2, 4, 1), "mult17": (2, 2, 4, 17), "T65": (2, 1, 65, 3), "R9": (2, 9, 4, 3), "G0": (0, 1, 4, 3)}.get(what, (2, 2, 4, 3))
    hyp = torch.full((max(mult * G, 1), T), 1000, dtype=torch.int64, device=DEV)[:mult * G]
    ref = torch.full((max(G, 1), R, T), 1000, dtype=torch.int64, device=DEV)[:G]
    size = K.cider_d_multi_workspace_bytes if mode == "batch" else K.cider_d_multi_df_workspace_bytes
    need = size(G, R, T, mult)
    assert (need > 0) == (what == "workspace_short")
    gs = GU.guarded_vec(max(mult * G, 1), dtype=torch.float32, fill="sentinel", device=DEV)
    gw = GU.guarded_vec(max(mult * G, 1), dtype=torch.float32, fill="sentinel", device=DEV)
    ws = GU.guarded_vec(need - 1 if what == "workspace_short" else 1 << 16, dtype=torch.uint8, fill="sentinel", device=DEV)
    s = K.CiderDArgs(K.ptr(hyp), hyp.stride(0), K.ptr(ref), ref.stride(0), ref.stride(1), None, G, R, T, mult, 6.0, K.ptr(gs.vec), K.ptr(gw.vec),
                     K.ptr(ws.vec), ws.vec.numel())
    if mode == "batch":
        rc = K.load().vlp_cider_d_multi(C.byref(s), K.stream_ptr())
    else:
        tab = U.table(4, 0)
        keys, vals = tab.to(DEV)
        a = K.CiderDDfArgs(s, C.c_void_p(keys.data_ptr()), C.c_void_p(vals.data_ptr()), len(tab), tab.n_docs)
        rc = K.load().vlp_cider_d_multi_df(C.byref(a), K.stream_ptr())
    assert rc == -1, rc
    assert "vlp_cider_d_multi" in K.load().vlp_last_error_string().decode()
    torch.cuda.synchronize()
    for g, name in ((gs, "scores"), (gw, "reward"), (ws, "workspace")):
        GU.assert_untouched(g, written=None, name=name)


def test_short_reward_is_refused_and_the_old_entries_keep_refusing_three():
    G, R, T, mult = 2, 2, 4, 3
    hyp = torch.full((mult * G, T), 1000, dtype=torch.int64, device=DEV)
    ref = torch.full((G, R, T), 1000, dtype=torch.int64, device=DEV)
    scores = torch.zeros(mult * G, device=DEV)
    tab = U.table(4, 0)
    with pytest.raises(RuntimeError, match="reward"):
        K.cider_d_multi(hyp, ref, None, mult, scores, torch.zeros(mult * G - 1, device=DEV))
    with pytest.raises(RuntimeError, match="reward"):
        K.cider_d_multi_df(hyp, ref, None, mult, scores, *tab.to(DEV), tab.n_docs, torch.zeros(G, device=DEV))
    assert not scores.cpu().numpy().any()
    assert K.cider_d_workspace_bytes(G, R, T, 3) == 0 and K.cider_d_df_workspace_bytes(G, R, T, 3) == 0
    assert K.cider_d_multi_workspace_bytes(G, R, T, 3) > 0 and K.cider_d_multi_df_workspace_bytes(G, R, T, 3) > K.cider_d_multi_workspace_bytes(G, R, T, 3)
    with pytest.raises(RuntimeError, match="mult 1 or 2"):
        K.cider_d(hyp, ref, None, 3, scores, workspace=torch.empty(1 << 16, dtype=torch.uint8, device=DEV))
    with pytest.raises(RuntimeError, match="mult 1 or 2"):
        K.cider_d_df(hyp, ref, None, 3, scores, *tab.to(DEV), tab.n_docs, workspace=torch.empty(1 << 16, dtype=torch.uint8, device=DEV))
    assert not scores.cpu().numpy().any()


def test_device_reward_function_against_the_host_function():
    B, R, T, Ks = 16, 5, 21, 16
    hyp, ref, count = U.make_corpus(B, R, T, Ks, 0)
    refs_h = CaptionRefs(torch.from_numpy(ref), torch.from_numpy(count))
    refs_d = refs_h.to(DEV)
    for tab in (None, U.table(T, 0)):
        want_r, want_s = SC.self_critical_reward_group(hyp, refs_h, Ks, df=tab)
        reward, scores = SC.self_critical_reward_group_device(torch.from_numpy(hyp).to(DEV), refs_d, Ks, df=tab)
        assert tuple(reward.shape) == (Ks * B, T) and reward.dtype == torch.float32 and reward.is_cuda
        assert float(np.abs(scores.double().cpu().numpy() - want_s).max()) <= SU.score_bound(T)
        assert float(np.abs(reward.double().cpu().numpy() - want_r).max()) <= SU.reward_bound(T, Ks)
        sums = reward[:, 0].view(Ks, B).sum(0)
        assert float(sums.abs().max()) <= Ks * SU.reward_bound(T, Ks)
    # the single-reference form: [B, T] ground-truth ids as a strided view
    wide = torch.zeros(B, 102 + T, dtype=torch.long, device=DEV)
    wide[:, 102:] = torch.from_numpy(ref[:, 0])
    r1, s1 = SC.self_critical_reward_group_device(torch.from_numpy(hyp[:3 * B]).to(DEV), wide[:, 102:], 3)
    w1, ws1 = SC.self_critical_reward_group(hyp[:3 * B], ref[:, 0], 3)
    assert float(np.abs(s1.double().cpu().numpy() - ws1).max()) <= SU.score_bound(T)
    assert float(np.abs(r1.double().cpu().numpy() - w1).max()) <= SU.reward_bound(T, 3)


# ---- (b) the sampling kernel ----------------------------------------------------------------------------------------------------------
def _cell(v):
    return torch.tensor([v], dtype=torch.long, device=DEV)


@pytest.mark.parametrize("rows,V", [(64, 28996), (5, 11)])
def test_sample_rows_rep_1_equals_sample_rows(rows, V):
    Vp = (V + 63) // 64 * 64
    g = torch.Generator().manual_seed(V)
    logits = (torch.randn(rows, Vp, generator=g) * 3).half().to(DEV)
    logits[:, V:] = 50.0
    seed = 0x5EED + 77
    ids, lp = torch.zeros(rows, dtype=torch.long, device=DEV), torch.zeros(rows, device=DEV)
    K.sample_rows(logits, Vp, rows, V, seed, 7001, ids, lp)
    ids_r, lp_r, ids2 = torch.full_like(ids, -1), torch.full_like(lp, float("nan")), torch.full((rows, 2), -1, dtype=torch.long, device=DEV)
    K.sample_rows_rep(logits, Vp, rows, V, 1, _cell(seed - 3), 3, 7001, ids_r, lp_r, ids2=ids2[:, 0])
    torch.cuda.synchronize()
    assert torch.equal(ids, ids_r) and same_bits(lp, lp_r)
    assert torch.equal(ids2[:, 0], ids) and bool((ids2[:, 1] == -1).all())
    assert int(ids.max()) < V                                   # the padding columns at 50.0 are never drawn
    K.sample_rows_rep(logits, Vp, rows, V, 1, _cell(seed - 3), 4, 7001, ids_r, lp_r)
    assert not torch.equal(ids, ids_r)                          # seed_add is part of the seed


def test_sample_rows_rep_5_equals_sample_rows_on_repeated_logits():
    rows, V, rep = 7, 1000, 5
    Vp = 1024
    g = torch.Generator().manual_seed(5)
    logits = (torch.randn(rows, Vp, generator=g) * 2).half().to(DEV)
    logits[:, V:] = 50.0
    n = rows * rep
    ids, lp = torch.zeros(n, dtype=torch.long, device=DEV), torch.zeros(n, device=DEV)
    K.sample_rows(logits.repeat_interleave(rep, dim=0).contiguous(), Vp, n, V, 991, 7001, ids, lp)
    out = torch.full((n, 3), -1, dtype=torch.long, device=DEV)          # strided outputs
    lp_r, ids2 = torch.zeros(n, 2, device=DEV), torch.full((n,), -1, dtype=torch.long, device=DEV)
    K.sample_rows_rep(logits, Vp, n, V, rep, _cell(990), 1, 7001, out[:, 1], lp_r[:, 1], ids2=ids2)
    torch.cuda.synchronize()
    assert torch.equal(out[:, 1], ids) and same_bits(lp_r[:, 1].contiguous(), lp) and torch.equal(ids2, ids)
    assert bool((out[:, 0] == -1).all()) and bool((out[:, 2] == -1).all()) and not lp_r[:, 0].any()
    assert int(ids.max()) < V
    assert any(len(set(ids[r * rep:(r + 1) * rep].tolist())) > 1 for r in range(rows))


def test_sample_rows_rep_draws_of_one_uniform_row_differ():
    V, rep = 28996, 5
    Vp = (V + 63) // 64 * 64
    logits = torch.zeros(1, Vp).half()
    logits[:, V:] = 50.0
    ids, lp = torch.zeros(rep, dtype=torch.long, device=DEV), torch.zeros(rep, device=DEV)
    K.sample_rows_rep(logits.to(DEV), Vp, rep, V, rep, _cell(12), 0, 7001, ids, lp)
    assert len(set(ids.tolist())) > 1 and int(ids.max()) < V
    assert float((lp + np.log(V)).abs().max()) < 1e-3


def test_sample_rows_rep_distribution():
    rows, V, rep = 4096, 11, 4
    Vp = 64
    base = torch.tensor([2.0, 1.0, 0.0, -1.0, 0.5, 3.0, -2.0, 0.0, 1.5, -0.5, 2.5])
    logits = torch.zeros(rows // rep, Vp).half()
    logits[:, :V] = base.half()
    logits[:, V:] = 50.0
    ids, lp = torch.zeros(rows, dtype=torch.long, device=DEV), torch.zeros(rows, device=DEV)
    K.sample_rows_rep(logits.to(DEV), Vp, rows, V, rep, _cell(1234), 0, 7001, ids, lp)
    ref_lp = torch.log_softmax(base.half().float(), dim=-1).to(DEV)
    assert int(ids.max()) < V
    assert float((lp - ref_lp[ids]).abs().max()) < 1e-5
    freq = torch.bincount(ids, minlength=V).float() / rows
    prob = ref_lp.exp()
    sigma = torch.sqrt(prob * (1 - prob) / rows)
    assert float(((freq - prob).abs() / sigma).max()) < 5.0, (freq, prob)          # every bin within 5 sigma


# ---- (c) the decoder -------------------------------------------------------------------------------------------------------------------
def _small_decoder():
    from tests.test_40_decode_gpu import build_decoder, decode_inputs
    mk = dict(vocab_size=1024, layers=2, tasks="img2txt", seed=41, std=0.05)
    p = O.init_params(vocab_size=mk["vocab_size"], layers=mk["layers"], tasks=mk["tasks"], seed=mk["seed"], std=mk["std"])
    B, T = 3, 6
    m = build_decoder(p, mk)
    dv = [t.to(DEV) for t in decode_inputs(B, T, 99)]
    return p, m, [dv[0].half(), dv[1].half()] + dv[2:], B, T


def test_one_sample_per_image_is_the_existing_sampled_decode():
    p, m, dv, B, T = _small_decoder()
    eng = m.engine
    s0 = eng.step_seed
    for call in range(3):                                  # plain, capture, replay
        eng.step_seed = s0 + 100 * call
        ids_g, lp_g = eng.decode_greedy(*dv, S.MASK_ID, sample=True)
        after = eng.step_seed
        eng.step_seed = s0 + 100 * call
        ids_s, lp_s = eng.decode_sample_group(*dv, S.MASK_ID, 1)
        assert eng.step_seed == after == s0 + 100 * call + T
        assert tuple(ids_s.shape) == (B, T) and torch.equal(ids_g, ids_s) and same_bits(lp_g, lp_s), call


def test_four_samples_per_image_plain_capture_replay():
    p, m, dv, B, T = _small_decoder()
    Ks = 4
    eng = m.engine
    pd = {k: v.to(DEV).half().float() for k, v in p.items()}
    in_len = dv[2].shape[1]
    vf, vp = O.vis_embed(pd, dv[0].float()), O.vis_pe_embed(pd, dv[1].float())

    def tiled(t):
        return t.repeat(Ks, *([1] * (t.dim() - 1)))
    vf, vp, prefix, seg, pos, am = [tiled(t) for t in (vf, vp, dv[2], dv[3], dv[4], dv[5])]
    outs = []
    for call in range(3):
        ids, lps = eng.decode_sample_group(*dv, S.MASK_ID, Ks)
        assert tuple(ids.shape) == (Ks * B, T) and tuple(lps.shape) == (Ks * B, T) and float(lps.max()) <= 0.0
        worst = 0.0
        for s in range(T):                                 # teacher-forced: row k*B + b is image b
            x = torch.cat((prefix, ids[:, :s], torch.full((Ks * B, 1), S.MASK_ID, device=DEV, dtype=torch.long)), dim=1)
            Lk = in_len + s + 1
            emb, _ = O.embeddings(pd, vf, vp, x, seg[:, :Lk], 100, position_ids=pos[:, :Lk])
            hs = O.encoder(pd, emb, O.extended_attention_mask(am[:, :Lk, :Lk], torch.float32), 12)
            logp = torch.log_softmax(O.lm_head(pd, hs[-1][:, -1:, :])[:, 0], dim=-1)
            ref = torch.gather(logp, 1, ids[:, s:s + 1])[:, 0]
            worst = max(worst, float((ref - lps[:, s]).abs().max()))
        report("decode_group_call%d" % call, logp_err=worst)
        assert worst < 3e-2, (call, worst)
        per_image = ids.view(Ks, B, T)
        assert all(len({tuple(per_image[k, b].tolist()) for k in range(Ks)}) > 1 for b in range(B))     # the samples of an image differ
        outs.append(ids)
    assert not torch.equal(outs[0], outs[1]) and not torch.equal(outs[1], outs[2]) and not torch.equal(outs[0], outs[2])
    ws = eng._ws[("dec", B, in_len + 1, in_len + T, Ks, "group")]
    assert ws["calls"] == 3
    assert all(("sample_group", s) in ws["plans"] for s in range(1, T)), sorted(ws["plans"], key=str)


def test_more_than_512_sequences_decode_unfused_and_say_so_once():
    """K*B = 520 > 512: M = 2 R exceeds the fused token step's 1024 rows, the decode takes the unfused path (one VlpPerformanceWarning per
    engine) and computes the same thing; more than 1024 sequences are refused before anything is launched."""
    import warnings
    from tests.test_40_decode_gpu import build_decoder, decode_inputs
    from vlp_amd.engine import VlpPerformanceWarning
    mk = dict(vocab_size=1024, layers=2, tasks="img2txt", seed=41, std=0.05)
    p = O.init_params(vocab_size=mk["vocab_size"], layers=mk["layers"], tasks=mk["tasks"], seed=mk["seed"], std=mk["std"])
    B, T, Ks = 65, 3, 8
    m = build_decoder(p, mk)
    eng = m.engine
    dv = [t.to(DEV) for t in decode_inputs(B, T, 7)]
    dv = [dv[0].half(), dv[1].half()] + dv[2:]
    with pytest.raises(RuntimeError, match="at most 1024"):
        eng.decode_sample_group(*dv, S.MASK_ID, 16)
    assert not any(k[0] == "dec" for k in eng._ws if isinstance(k, tuple))          # refused before a workspace existed
    said = []
    for call in range(2):
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            ids, lps = eng.decode_sample_group(*dv, S.MASK_ID, Ks)
        said.append([x for x in w if issubclass(x.category, VlpPerformanceWarning) and "unfused" in str(x.message)])
    assert len(said[0]) == 1 and len(said[1]) == 0
    assert tuple(ids.shape) == (Ks * B, T)
    pd = {k: v.to(DEV).half().float() for k, v in p.items()}
    in_len = dv[2].shape[1]

    def tiled(t):
        return t.repeat(Ks, *([1] * (t.dim() - 1)))
    vf, vp = tiled(O.vis_embed(pd, dv[0].float())), tiled(O.vis_pe_embed(pd, dv[1].float()))
    prefix, seg, pos, am = [tiled(t) for t in dv[2:]]
    worst = 0.0
    for s in range(T):
        x = torch.cat((prefix, ids[:, :s], torch.full((Ks * B, 1), S.MASK_ID, device=DEV, dtype=torch.long)), dim=1)
        Lk = in_len + s + 1
        emb, _ = O.embeddings(pd, vf, vp, x, seg[:, :Lk], 100, position_ids=pos[:, :Lk])
        hs = O.encoder(pd, emb, O.extended_attention_mask(am[:, :Lk, :Lk], torch.float32), 12)
        logp = torch.log_softmax(O.lm_head(pd, hs[-1][:, -1:, :])[:, 0], dim=-1)
        worst = max(worst, float((torch.gather(logp, 1, ids[:, s:s + 1])[:, 0] - lps[:, s]).abs().max()))
    report("decode_group_520_sequences", logp_err=worst)
    assert worst < 3e-2, worst


# ---- (d) the step ----------------------------------------------------------------------------------------------------------------------
def test_train_forward_with_three_samples_logprobs_and_gradients():
    from tests.test_80_scst_gpu import _decoder, rel
    from tests.test_scst_cpu import forced_decode_logp, scst_inputs
    V, layers, B, Ks, seed = 1024, 3, 3, 3, 21
    p = O.init_params(vocab_size=V, layers=layers, seed=seed, std=0.05)
    m = _decoder(p, V, layers).train()
    eng = m.engine
    img, vis_pe, prefix, seg, pos, am, _, _ = scst_inputs(B, 12, seed, V, short=(1,), ragged=((0, 41),), pos_offset=2)
    dv = [t.to(DEV) for t in (img, vis_pe, prefix, seg, pos, am)]
    dv[0], dv[1] = dv[0].half(), dv[1].half()
    ids, logp = m(*dv, sample_mode="sample", n_samples=Ks)
    T = ids.shape[1]
    assert tuple(ids.shape) == (Ks * B, T) and logp.requires_grad and logp.grad_fn is not None

    def tiled(t):
        return t.repeat(Ks, *([1] * (t.dim() - 1)))
    tv = [tiled(t) for t in dv]
    gen = SC.clean_captions(ids, S.SEP_ID)
    g = torch.Generator().manual_seed(seed)
    reward = (torch.randn(Ks * B, 1, generator=g) * 2.0).expand(Ks * B, T).to(DEV)
    eng.zero_grad()
    loss = SC.RewardCriterion()(logp, gen, reward)
    (loss * 1024.0).backward()
    torch.cuda.synchronize()
    grads = {n: (q.grad.float() / 1024.0) for n, q in m.named_parameters()}
    # score_samples on explicitly tiled inputs: the same bits
    _, lp_tiled = eng.score_samples(*tv, ids, S.MASK_ID)
    assert same_bits(logp.detach().cpu(), lp_tiled.cpu())
    pd = {k: v.to(DEV).half().float().requires_grad_(True) for k, v in p.items()}
    vf, vp = O.vis_embed(pd, tv[0].float()), O.vis_pe_embed(pd, tv[1].float())
    lp_o = forced_decode_logp(pd, vf, vp, *tv[2:], ids, S.MASK_ID)
    SC.RewardCriterion()(lp_o, gen, reward).backward()
    e_lp = float((logp.detach() - lp_o.detach()).abs().max())
    errs = {}
    for k, t in pd.items():
        if t.grad is None:
            continue
        if k.endswith("attention.self.key.bias"):     # true value 0: bounded against the sibling query-bias gradient (as test_80 does)
            d, qb = (grads[k] - t.grad).double(), pd[k.replace("key.bias", "query.bias")].grad.double()
            errs[k] = max(float(d.abs().max() / qb.abs().max()), float(d.norm() / qb.norm()))
        else:
            errs[k] = rel(grads[k], t.grad)
    worst = max(errs, key=errs.get)
    report("train_forward_3_samples", logp_vs_oracle=e_lp, worst_grad=worst, worst_grad_rel=errs[worst], rows=Ks * B, T=T)
    assert e_lp < 0.0036, e_lp                          # test_80's small-model bounds
    assert errs[worst] < 0.07, (worst, errs[worst])
    with pytest.raises(ValueError):
        m(*dv, sample_mode="greedy", n_samples=2)
    m.search_beam_size = 2
    with pytest.raises(ValueError, match="search_beam_size"):
        m(*dv, sample_mode="sample", n_samples=2)


def test_scst_step_with_three_samples_host_and_device_agree(monkeypatch):
    """scst_step(samples=3) from the same state with the reward on the host and on the device: the same K*B samples, no greedy decode,
    rewards that are not all zero and agree within the bound, a mean reward of zero, the same loss."""
    from tests.test_80_scst_gpu import _decoder
    from vlp_amd import run_img2txt_dist as R
    from vlp_amd.optimization_fp16 import FP16_Optimizer_State, FusedAdam
    V, B, Ks, max_len_b = 1024, 4, 3, 12
    T = max_len_b + 1
    words = list(range(300, 306))
    rng = np.random.RandomState(5)
    p = O.init_params(vocab_size=V, layers=2, seed=21, std=0.05)
    # an untrained model draws from all 1024 words and shares nothing with its ground truth; a bias towards the six words of the captions
    # (and [SEP]) makes the samples overlap with the references, so the rewards are not all zero (as tests/test_82_scst_df_gpu.py does)
    p["cls.predictions.bias"][words] = 8.0
    p["cls.predictions.bias"][S.SEP_ID] = 7.0
    batch = S.batch_to(S.make_batch(B, max_len_b=max_len_b, len_vis_input=100, vocab_size=V, max_pred=0, mask_prob=0.0, seed=7), DEV, half=True)
    ids = batch.input_ids.clone()
    for b in range(B):
        row = [int(t) for t in rng.choice(words, size=rng.randint(3, max_len_b + 1))] + [S.SEP_ID]
        ids[b, 102:] = torch.tensor(row + [0] * (T - len(row)), device=DEV)
    batch = batch._replace(input_ids=ids)
    log = []
    real_host, real_dev = SC.self_critical_reward_group, SC.self_critical_reward_group_device

    def host(gen, refs, n, **kw):
        r, s = real_host(gen, refs, n, **kw)
        log.append(("host", n, gen.detach().cpu().numpy(), r))
        return r, s

    def dev(gen, refs, n, **kw):
        r, s = real_dev(gen, refs, n, **kw)
        log.append(("device", n, gen.detach().cpu().numpy(), r.detach().cpu().numpy().copy()))
        return r, s
    monkeypatch.setattr(SC, "self_critical_reward_group", host)
    monkeypatch.setattr(SC, "self_critical_reward_group_device", dev)
    out, marks = {}, {}
    for mode in ("host", "device"):
        torch.manual_seed(3)
        m = _decoder(p, V, 2).train()
        m.engine.step_seed = 1234
        named = list(m.named_parameters())
        nd = ["bias", "LayerNorm.bias", "LayerNorm.weight"]
        groups = [{"params": [q for n, q in named if not any(x in n for x in nd)], "weight_decay": 0.01},
                  {"params": [q for n, q in named if any(x in n for x in nd)], "weight_decay": 0.0}]
        opt = FP16_Optimizer_State(FusedAdam(groups, lr=1e-4, bias_correction=False, max_grad_norm=1.0), dynamic_loss_scale=True)
        before = m.bert.encoder.layer[0].attention.self.query.weight.detach().clone()
        marks[mode] = []
        loss, mean_r = R.scst_step(m, opt, batch, 1e-4, 100, SC.RewardCriterion(), mark=marks[mode].append, reward_on=mode, samples=Ks)
        torch.cuda.synchronize()
        out[mode] = (float(loss.detach()), float(mean_r))
        assert not torch.equal(m.bert.encoder.layer[0].attention.self.query.weight.detach(), before)      # the step moved the model
    assert marks["host"] == ["sample_forward", "reward_host", "backward", "optimizer"]
    assert marks["device"] == ["sample_forward", "reward_device", "backward", "optimizer"]
    (ka, na, gen_a, r_a), (kb, nb, gen_b, r_b) = log
    assert (ka, kb, na, nb) == ("host", "device", Ks, Ks)
    assert gen_a.shape == (Ks * B, T) and np.array_equal(gen_a, gen_b)
    assert np.count_nonzero(r_a[:, 0]) >= Ks * B // 2, r_a[:, 0]
    e_r = float(np.abs(r_b.astype(np.float64) - r_a).max())
    report("scst_step_three_samples", reward_err=e_r, bound=SU.reward_bound(T, Ks), host=out["host"], device=out["device"],
           host_reward=[round(float(v), 6) for v in r_a[:, 0]])
    assert e_r <= SU.reward_bound(T, Ks)
    assert all(abs(v[1]) <= 3 * 2.0 ** -24 * 10 for v in out.values()), out                # by construction of the baseline
    assert np.isfinite(out["host"][0]) and abs(out["host"][0] - out["device"][0]) < 0.0048   # test_81's tolerance for this model's log-probs


def test_entry_script_with_three_samples(tmp_path, monkeypatch):
    from tests.test_80_scst_gpu import BASE, _ce_checkpoint
    from vlp_amd import run_img2txt_dist as R
    ckpt = _ce_checkpoint(R, tmp_path)
    T, Ks = 21, 3
    seen = {}
    real_dev, real_host, real_step = SC.self_critical_reward_group_device, SC.self_critical_reward_group, R.scst_step

    def dev(gen, refs, n, **kw):
        r, s = real_dev(gen, refs, n, **kw)
        seen.setdefault("device", []).append((gen.detach().cpu().numpy(), r.detach().cpu().numpy().copy()))
        return r, s

    def host(gen, refs, n, **kw):
        r, s = real_host(gen, refs, n, **kw)
        seen.setdefault("host", []).append((gen.detach().cpu().numpy(), r.copy()))
        return r, s

    def step(*a, **kw):
        assert kw.get("samples") == Ks
        marks = []
        out = real_step(*a, mark=marks.append, **kw)
        seen.setdefault("marks", []).append(marks)
        seen.setdefault("mean_r", []).append(float(out[1]))
        return out
    monkeypatch.setattr(SC, "self_critical_reward_group_device", dev)
    monkeypatch.setattr(SC, "self_critical_reward_group", host)
    monkeypatch.setattr(R, "scst_step", step)
    out = os.path.join(tmp_path, "scst")
    argv = BASE + ["--scst", "--scst_samples", str(Ks), "--scst_reward", "device", "--synthetic", "3", "--learning_rate", "1e-4",
                   "--model_recover_path", ckpt, "--output_dir", out, "--num_train_epochs", "2", "--stop_after_epoch", "1"]
    R.main(argv)
    log = open(os.path.join(out, "training.log")).read()
    losses = [float(x) for x in re.findall(r"Loss (\S+), Mean R", log)]
    assert len(losses) == 3 and all(np.isfinite(v) and abs(v) < 1e4 for v in losses), log
    assert all(mk == ["sample_forward", "reward_device", "backward", "optimizer"] for mk in seen["marks"]), seen["marks"]
    assert len(seen["device"]) == 3 and all(g.shape == (Ks * 4, T) for g, _ in seen["device"])
    report("entry_three_samples", losses=losses, mean_r=seen["mean_r"], reward_step1=[round(float(v), 6) for v in seen["device"][0][1][:, 0]])
    assert all(abs(v) <= 3 * 2.0 ** -24 * 10 for v in seen["mean_r"]), seen["mean_r"]           # by construction of the baseline
    R.main(argv[:-2])                                     # resume: epoch 2 from model.1.bin / optim.1.bin
    assert os.path.exists(os.path.join(out, "model.2.bin"))
    assert "Recover optimizer: 1" in open(os.path.join(out, "training.log")).read()
    # the host reward from the same start: the same samples in the first step, rewards within the bound
    out_h = os.path.join(tmp_path, "scst_host")
    R.main([out_h if a == out else ("host" if a == "device" else a) for a in argv])
    assert seen["marks"][-1] == ["sample_forward", "reward_host", "backward", "optimizer"]
    (gen_d, r_d), (gen_h, r_h) = seen["device"][0], seen["host"][0]
    assert np.array_equal(gen_d, gen_h)
    e_r = float(np.abs(r_d.astype(np.float64) - r_h).max())
    report("entry_three_samples", host_vs_device_reward_err=e_r, bound=SU.reward_bound(T, Ks))
    assert e_r <= SU.reward_bound(T, Ks)
