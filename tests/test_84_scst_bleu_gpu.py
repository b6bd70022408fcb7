"""GPU: sentence BLEU-4 in the SCST reward on the device (vlp_bleu4, csrc/reward.hip) against the project's own host scorer
(vlp_amd.scst.Bleu, fp64).

(1) the kernel against Bleu on seeded corpora with a length variation (tests/scst_bleu_util.py): the integers the score is made of (stats)
    exactly, bleu4 within 16 * 2^-24.  What the corpus must offer (matching 4-grams, brevity-penalised rows) is asserted on the host
    values before the kernel's output is looked at;
(2) hand-built hard rows inside one G = 6, R = 3, T = 8 case; garbage behind a row's first 0 and invalid reference rows change no bit;
(3) the mix and the baselines: bit for bit the stated fp32 expressions of the stored values; against the host functions within the bound;
(4) the contract: strided rows with poisoned padding, guard bands around every output, NULL optional outputs, bit-equal repeats, refusals
    by return code with nothing written;
(5) self_critical_reward_device / _group_device with weights, captured into a graph and replayed on new inputs;
(6) scst_step with reward_weights = (1, 0.5) on the host and on the device from the same state; the entry script with the two flags.

Bounds.  bleu4: a score is at most 1 and is made of about a dozen fp32 roundings plus one powf and one expf: 16 * 2^-24 (an fp32
restatement of the host class in numpy differs from fp64 by at most 7.2e-8 on these corpora; a wrong count is caught exactly by stats, also
where the score itself is tiny).  A mixed score: cider_weight * test_81's (4 T + 16) * 2^-24 * 10 + bleu_weight * 16 * 2^-24 + one ulp of
the value.  Every test prints what it measured through report() (pytest -s); the figures of an MI355X run are in profiles/scst_bleu.json."""
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

from tests import guard_util as GU                                  # noqa: E402
from tests import scst_bleu_util as BU                              # noqa: E402
from tests import scst_df_util as U                                 # noqa: E402
from tests import scst_samples_util as SU                           # noqa: E402
from vlp_amd import _lib as K                                       # noqa: E402
from vlp_amd import scst as SC                                      # noqa: E402
from vlp_amd import synthetic as S                                  # noqa: E402
from vlp_amd.input_prep import CaptionRefs                          # noqa: E402

DEV = torch.device("cuda:0")
REPORT = {}
f32 = np.float32


def report(key, **kw):
    """Prints what a test measured; with VLP_SCST_BLEU_RECORD=<json file> (profiles/scst_bleu.json when the record is taken) the figures are
    also kept under that file's "test_84" key, next to the timing runs tools/scst_bench.py writes there."""
    REPORT.setdefault(key, {}).update(kw)
    print("%s: %s" % (key, json.dumps(REPORT[key], sort_keys=True)))
    path = os.environ.get("VLP_SCST_BLEU_RECORD")
    if path:
        rec = json.load(open(path)) if os.path.exists(path) else {}
        rec.setdefault("test_84", {})[key] = REPORT[key]
        with open(path, "w") as f:
            json.dump(rec, f, indent=2, sort_keys=True)


def same_bits(a, b):
    a, b = torch.as_tensor(a), torch.as_tensor(b)
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32))


def run_kernel(hyp, ref, count, mult, base=None, w_base=1.0, w_bleu=1.0, mixed=False, reward=None):
    """vlp_bleu4 on numpy inputs -> dict of CPU tensors: bleu4, stats, and mixed / reward when asked for (reward: None, "pair" or "loo")."""
    G = ref.shape[0]
    n = mult * G
    h, r = torch.from_numpy(hyp).to(DEV), torch.from_numpy(ref).to(DEV)
    c = torch.from_numpy(count).to(DEV) if count is not None else None
    out = {"bleu4": torch.full((n,), float("nan"), device=DEV), "stats": torch.full((n, 6), -7, dtype=torch.int32, device=DEV)}
    if mixed or reward:
        out["mixed"] = torch.full((n,), float("nan"), device=DEV)
    if reward:
        out["reward"] = torch.full((n if reward == "loo" else G,), float("nan"), device=DEV)
    K.bleu4(h, r, c, mult, out["bleu4"], stats=out["stats"], base=None if base is None else torch.from_numpy(base).to(DEV), w_base=w_base, w_bleu=w_bleu,
            mixed=out.get("mixed"), reward=out.get("reward"), loo=reward == "loo")
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


_HOST = {}


def host_case(shape):
    """(hyp, ref, count, stats, bleu [4, n]) of a shape's corpus: computed once, shared, never modified."""
    if shape not in _HOST:
        corpus = BU.make_corpus(*shape, BU.seed_of(shape))
        _HOST[shape] = corpus + BU.host_bleu(*corpus, shape[3])
    return _HOST[shape]


# ---- (1) the kernel against Bleu ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", BU.SHAPES, ids=["G%d_R%d_T%d_m%d" % s for s in BU.SHAPES])
def test_kernel_against_host_scorer(shape):
    G, R, T, mult = shape
    hyp, ref, count, stats, bleu = host_case(shape)
    # on the host values alone, before the kernel's output is looked at
    c4, bp = BU.shares(stats)
    assert BU.conditions(shape, stats), (c4, bp)
    if G >= 5 and T >= 21:
        assert c4 >= 0.4 and bp >= 0.2, (c4, bp)
    got = run_kernel(hyp, ref, count, mult)
    err = float(np.abs(got["bleu4"].double().numpy() - bleu[3]).max())
    report("kernel_G%d_R%d_T%d_m%d" % shape, max_abs_err=err, bound=BU.BLEU_BOUND, rows_with_a_4gram_match=c4, rows_brevity_penalised=bp,
           max_bleu4=float(bleu[3].max()), seed=BU.seed_of(shape))
    assert np.array_equal(got["stats"].numpy(), stats), np.flatnonzero((got["stats"].numpy() != stats).any(1))
    assert err <= BU.BLEU_BOUND, (err, BU.BLEU_BOUND)


# ---- (2) hand-built hard rows ---------------------------------------------------------------------------------------------------------
def test_hard_rows():
    G = 6
    hyp, ref, count = BU.hard_case(True)
    stats, bleu = BU.host_bleu(hyp, ref, count, 2)
    # what the rows were built for, on the host values
    assert stats[0].tolist() == [1, 0, 0, 0, 1, 6]                        # just 0
    assert stats[1, 4] == 8 and not (hyp[1] == 0).any()                   # full length, no 0
    assert stats[G + 1].tolist() == [6, 5, 4, 3, 8, 7]                    # 1001 six times, the references hold it 2 and 4 times
    assert stats[2].tolist() == [4, 2, 1, 0, 4, 3]                        # lengths 3 and 5 against 4: the shorter
    assert count[0] == 1 and abs(bleu[3, G] - 1.0) < 1e-8                 # equal to its one valid reference
    got = run_kernel(hyp, ref, count, 2, mixed=True, w_bleu=0.5, reward="pair")
    err = float(np.abs(got["bleu4"].double().numpy() - bleu[3]).max())
    report("hard_rows", max_abs_err=err, bound=BU.BLEU_BOUND, host=[float("%.6g" % v) for v in bleu[3]])
    assert np.array_equal(got["stats"].numpy(), stats)
    assert err <= BU.BLEU_BOUND
    # garbage behind the first 0 and invalid reference rows change no bit
    hyp0, ref0, count0 = BU.hard_case(False)
    assert np.array_equal(count, count0) and not np.array_equal(ref, ref0) and not np.array_equal(hyp, hyp0)
    got0 = run_kernel(hyp0, ref0, count0, 2, mixed=True, w_bleu=0.5, reward="pair")
    for k in got:
        assert same_bits(got[k], got0[k]), k
    # ref_count below 1 and above R is clamped
    wild = count.copy()
    wild[0], wild[3] = -3, 99
    assert np.array_equal(run_kernel(hyp, ref, wild, 2)["stats"].numpy(), stats)


# ---- (3) mixing and baseline ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(5, 3, 21, 2), (33, 5, 20, 5), (5, 3, 21, 16)], ids=lambda s: "G%d_R%d_T%d_m%d" % s)
def test_mix_and_rewards_are_the_stated_expressions(shape):
    G, R, T, mult = shape
    hyp, ref, count, stats, bleu = host_case(shape)
    cider = U.host_scores(hyp, ref, count, mult).astype(f32)          # a base of the right scale
    assert cider.any()
    wb, wl = 0.3, 0.7                                                  # neither is an fp32 number
    plain = run_kernel(hyp, ref, count, mult)
    got = run_kernel(hyp, ref, count, mult, base=cider, w_base=wb, w_bleu=wl, reward="loo")
    assert same_bits(got["bleu4"], plain["bleu4"]) and torch.equal(got["stats"], plain["stats"])
    b = got["bleu4"].numpy()
    want = f32(wb) * cider + f32(wl) * b                               # numpy rounds every operation to fp32: no fma
    assert want.dtype == f32 and same_bits(got["mixed"], torch.from_numpy(want))
    m = got["mixed"].numpy()
    assert same_bits(got["reward"], torch.from_numpy(SU.loo(m, mult))) and np.count_nonzero(got["reward"].numpy()) >= mult * G // 2
    # base = NULL
    alone = run_kernel(hyp, ref, count, mult, w_base=123.0, w_bleu=wl, reward="loo")
    assert same_bits(alone["mixed"], torch.from_numpy(f32(wl) * b)) and same_bits(alone["reward"], torch.from_numpy(SU.loo(alone["mixed"].numpy(), mult)))
    if mult == 2:
        pair = run_kernel(hyp, ref, count, mult, base=cider, w_base=wb, w_bleu=wl, reward="pair")
        assert same_bits(pair["mixed"], got["mixed"]) and same_bits(pair["reward"], torch.from_numpy(m[:G] - m[G:]))
        assert same_bits(got["reward"][:G], pair["reward"]) and torch.equal(got["reward"][G:], -pair["reward"])
    # mixed written over base (what the device reward functions do)
    base_t = torch.from_numpy(cider).to(DEV)
    K.bleu4(torch.from_numpy(hyp).to(DEV), torch.from_numpy(ref).to(DEV), torch.from_numpy(count).to(DEV), mult, torch.empty(mult * G, device=DEV),
            base=base_t, w_base=wb, w_bleu=wl, mixed=base_t)
    assert same_bits(base_t.cpu(), got["mixed"])


def _refs(ref, count, dev=None):
    r = CaptionRefs(torch.from_numpy(np.array(ref)), torch.from_numpy(np.array(count)))
    return r.to(dev) if dev is not None else r


@pytest.mark.parametrize("weights", [(1.0, 0.5), (0.0, 1.0), (0.5, 2.0)], ids=lambda w: "w%g_%g" % w)
def test_device_reward_functions_against_the_host_functions(weights):
    cw, bw = weights
    B, R, T = 16, 5, 21
    # pair
    hyp, ref, count = BU.make_corpus(B, R, T, 2, 0)
    want_r, want_s = SC.self_critical_reward_refs(hyp[B:], _refs(ref, count), hyp[:B], cider_weight=cw, bleu_weight=bw)
    assert np.count_nonzero(want_r[:, 0]) >= B // 2
    reward, scores = SC.self_critical_reward_device(torch.from_numpy(hyp[B:]).to(DEV), _refs(ref, count, DEV), torch.from_numpy(hyp[:B]).to(DEV),
                                                    cider_weight=cw, bleu_weight=bw)
    assert tuple(reward.shape) == (B, T) and reward.dtype == torch.float32 and reward.is_cuda and tuple(scores.shape) == (2 * B,)
    e_s = np.abs(scores.double().cpu().numpy() - want_s)
    assert (e_s <= BU.mixed_bound(T, cw, bw, want_s)).all(), e_s.max()
    assert torch.equal(reward[:, 0], scores[:B] - scores[B:]) and torch.equal(reward, reward[:, :1].expand(B, T))
    # leave-one-out, with the call's own document frequencies and with a table (CIDEr-D only)
    Ks = 5
    hyp5, ref5, count5 = BU.make_corpus(B, R, T, Ks, 1)
    e_g = 0.0
    for tab in (None, U.table(T, 0)):
        want_r5, want_s5 = SC.self_critical_reward_group(hyp5, _refs(ref5, count5), Ks, df=tab, cider_weight=cw, bleu_weight=bw)
        r5, s5 = SC.self_critical_reward_group_device(torch.from_numpy(hyp5).to(DEV), _refs(ref5, count5, DEV), Ks, df=tab, cider_weight=cw, bleu_weight=bw)
        e5 = np.abs(s5.double().cpu().numpy() - want_s5)
        assert (e5 <= BU.mixed_bound(T, cw, bw, want_s5)).all(), e5.max()
        assert same_bits(r5[:, 0].contiguous().cpu(), torch.from_numpy(SU.loo(s5.cpu().numpy(), Ks)))
        e_g = max(e_g, float(e5.max()))
    # the single-reference form: [B, T] ground-truth ids as a strided view
    wide = torch.zeros(B, 102 + T, dtype=torch.long, device=DEV)
    wide[:, 102:] = torch.from_numpy(ref[:, 0])
    r1, s1 = SC.self_critical_reward_device(torch.from_numpy(hyp[B:]).to(DEV), wide[:, 102:], torch.from_numpy(hyp[:B]).to(DEV), cider_weight=cw, bleu_weight=bw)
    w1, ws1 = SC.self_critical_reward(hyp[B:], ref[:, 0], hyp[:B], B, cider_weight=cw, bleu_weight=bw)
    assert (np.abs(s1.double().cpu().numpy() - ws1) <= BU.mixed_bound(T, cw, bw, ws1)).all()
    report("device_vs_host_w%g_%g" % weights, pair_score_err=float(e_s.max()), group_score_err=e_g, bound_at_0=float(BU.mixed_bound(T, cw, bw, 0.0)))


# ---- (4) contract ---------------------------------------------------------------------------------------------------------------------
def test_contract_guards_strides_and_determinism():
    shape = (5, 3, 21, 5)
    G, R, T, mult = shape
    n = mult * G
    hyp, ref, count = BU.make_corpus(*shape, 2)
    base = U.host_scores(hyp, ref, count, mult).astype(f32)
    plain = run_kernel(hyp, ref, count, mult, base=base, w_base=1.0, w_bleu=0.5, reward="loo")
    # rows with strides larger than T; the padding and the guards hold 1000, a real word
    gh = GU.guarded(n, T, ld=T + 5, dtype=torch.int64, fill=1000, device=DEV).set(torch.from_numpy(hyp).to(DEV))
    gr = GU.guarded(G * R, T, ld=T + 3, dtype=torch.int64, fill=1000, device=DEV).set(torch.from_numpy(ref.reshape(G * R, T)).to(DEV))
    gc = GU.guarded_vec(G, dtype=torch.int32, fill=R, device=DEV)
    gc.vec.copy_(torch.from_numpy(count).to(DEV))
    gc.seal()
    gb = GU.guarded_vec(n, dtype=torch.float32, fill="nan", device=DEV)
    gb.vec.copy_(torch.from_numpy(base).to(DEV))
    gb.seal()
    ref_view = gr.full.view(G, R, T + 3)[:, :, :T]
    assert ref_view.stride() == (R * (T + 3), T + 3, 1) and gh.view.stride() == (T + 5, 1)
    outs = []
    for _ in range(2):
        go = {k: GU.guarded_vec(n, dtype=torch.float32, fill="sentinel", device=DEV) for k in ("bleu4", "mixed", "reward")}
        gs = GU.guarded_vec(6 * n, dtype=torch.int32, fill="sentinel", device=DEV)
        K.bleu4(gh.view, ref_view, gc.vec, mult, go["bleu4"].vec, stats=gs.vec, base=gb.vec, w_base=1.0, w_bleu=0.5, mixed=go["mixed"].vec,
                reward=go["reward"].vec, loo=True)
        torch.cuda.synchronize()
        for g, name, written in [(go[k], k, "logical") for k in go] + [(gs, "stats", "logical"), (gh, "hyp", None), (gr, "ref", None), (gc, "ref_count", None),
                                                                       (gb, "base", None)]:
            GU.assert_untouched(g, written=written, name=name)
            if written:
                GU.assert_written(g, name=name)
        outs.append({"bleu4": go["bleu4"].vec.cpu(), "mixed": go["mixed"].vec.cpu(), "reward": go["reward"].vec.cpu(), "stats": gs.vec.view(n, 6).cpu()})
    for k in ("bleu4", "mixed", "reward"):
        assert same_bits(outs[0][k], outs[1][k]) and same_bits(outs[0][k], plain[k]), k
    assert torch.equal(outs[0]["stats"], outs[1]["stats"]) and torch.equal(outs[0]["stats"], plain["stats"])
    # NULL optional outputs: bleu4 alone, and guards around it
    gq = GU.guarded_vec(n, dtype=torch.float32, fill="sentinel", device=DEV)
    K.bleu4(gh.view, ref_view, gc.vec, mult, gq.vec)
    torch.cuda.synchronize()
    GU.assert_untouched(gq, written="logical", name="bleu4")
    assert same_bits(gq.vec.cpu(), plain["bleu4"])
    # ref_count = NULL means all R
    full = np.full(G, R, dtype=np.int32)
    a, b = run_kernel(hyp, ref, None, mult), run_kernel(hyp, ref, full, mult)
    assert same_bits(a["bleu4"], b["bleu4"]) and torch.equal(a["stats"], b["stats"])
    assert np.array_equal(a["stats"].numpy(), BU.host_bleu(hyp, ref, full, mult)[0])


REFUSALS = {"T0": dict(T=0), "T65": dict(T=65), "R9": dict(R=9), "G1025": dict(G=1025), "mult17": dict(mult=17), "G0": dict(G=0), "mult0": dict(mult=0),
            "reward_without_mixed": dict(mixed=False, reward=True), "pair_mult3": dict(mult=3, reward=True, mode=0), "pair_mult1": dict(mult=1, reward=True, mode=0),
            "loo_mult1": dict(mult=1, reward=True, mode=1), "mode7": dict(reward=True, mode=7), "short_hyp_ld": dict(hyp_ld=3), "null_bleu4": dict(bleu4=False)}


@pytest.mark.parametrize("what", sorted(REFUSALS))
def test_refusals_by_return_code(what):
    cfg = dict(G=2, R=2, T=4, mult=2, mixed=True, reward=False, mode=0, hyp_ld=None, bleu4=True)
    cfg.update(REFUSALS[what])
    G, R, T, mult = cfg["G"], cfg["R"], cfg["T"], cfg["mult"]
    hyp = torch.full((max(mult * G, 1), max(T, 1)), 1000, dtype=torch.int64, device=DEV)
    ref = torch.full((max(G, 1), R, max(T, 1)), 1000, dtype=torch.int64, device=DEV)
    n = max(mult * G, 1)
    outs = {k: GU.guarded_vec(n, dtype=torch.float32, fill="sentinel", device=DEV) for k in ("bleu4", "mixed", "reward")}
    gs = GU.guarded_vec(6 * n, dtype=torch.int32, fill="sentinel", device=DEV)
    a = K.Bleu4Args(K.ptr(hyp), cfg["hyp_ld"] or hyp.stride(0), K.ptr(ref), ref.stride(0), ref.stride(1), None, G, R, T, mult,
                    K.ptr(outs["bleu4"].vec) if cfg["bleu4"] else None, K.ptr(gs.vec), None, 1.0, 1.0, K.ptr(outs["mixed"].vec) if cfg["mixed"] else None,
                    K.ptr(outs["reward"].vec) if cfg["reward"] else None, cfg["mode"])
    rc = K.load().vlp_bleu4(C.byref(a), K.stream_ptr())
    assert rc == -1, rc
    assert "vlp_bleu4" in K.load().vlp_last_error_string().decode()
    torch.cuda.synchronize()
    for g, name in [(outs[k], k) for k in outs] + [(gs, "stats")]:
        GU.assert_untouched(g, written=None, name=name)             # nothing was launched
    # the wrapper refuses tensors that do not fit before it calls the library
    if what == "reward_without_mixed":
        with pytest.raises(RuntimeError, match=r"vlp_bleu4.*status -1"):
            K.bleu4(hyp, ref, None, mult, outs["bleu4"].vec, reward=outs["reward"].vec)
        GU.assert_untouched(outs["bleu4"], written=None, name="bleu4")


# ---- (5) capturable -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weights", [(1.0, 0.5), (0.0, 1.0)], ids=lambda w: "w%g_%g" % w)
@pytest.mark.parametrize("group", [False, True], ids=["pair", "group"])
def test_device_reward_is_capturable_and_replays_on_new_inputs(weights, group):
    cw, bw = weights
    B, R, T, Ks = 16, 5, 21, 3
    mult = Ks if group else 2

    def call(hyp_t, refs, scores):
        if group:
            return SC.self_critical_reward_group_device(hyp_t, refs, Ks, scores_out=scores, workspace=ws, cider_weight=cw, bleu_weight=bw)
        return SC.self_critical_reward_device(hyp_t[B:], refs, hyp_t[:B], scores_out=scores, workspace=ws, cider_weight=cw, bleu_weight=bw)
    hyp, ref, count = BU.make_corpus(B, R, T, mult, 0)
    s_hyp = torch.from_numpy(hyp).to(DEV)
    refs = _refs(ref, count, DEV)
    scores = torch.zeros(mult * B, device=DEV)
    ws = torch.empty((K.cider_d_multi_workspace_bytes if group else K.cider_d_workspace_bytes)(B, R, T, mult), dtype=torch.uint8, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call(s_hyp, refs, scores)                                                        # warm-up: code objects loaded before the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):                                           # any synchronising call fails the capture
        reward, sc = call(s_hyp, refs, scores)
    assert sc is scores
    hyp2, ref2, count2 = BU.make_corpus(B, R, T, mult, 3)
    assert not np.array_equal(hyp, hyp2)
    s_hyp.copy_(torch.from_numpy(hyp2))
    refs.ids.copy_(torch.from_numpy(ref2))
    refs.count.copy_(torch.from_numpy(count2))
    graph.replay()
    torch.cuda.synchronize()
    got_r, got_s = reward.clone(), scores.clone()
    plain_r, plain_s = call(torch.from_numpy(hyp2).to(DEV), _refs(ref2, count2, DEV), torch.zeros(mult * B, device=DEV))
    assert same_bits(got_s.cpu(), plain_s.cpu()) and same_bits(got_r.contiguous().cpu(), plain_r.contiguous().cpu())
    if group:
        want_r, want_s = SC.self_critical_reward_group(hyp2, _refs(ref2, count2), Ks, cider_weight=cw, bleu_weight=bw)
    else:
        want_r, want_s = SC.self_critical_reward_refs(hyp2[B:], _refs(ref2, count2), hyp2[:B], cider_weight=cw, bleu_weight=bw)
    assert np.count_nonzero(want_r[:, 0]) >= B // 2
    e_s = np.abs(got_s.double().cpu().numpy() - want_s)
    report("graph_replay_%s_w%g_%g" % (("group" if group else "pair",) + weights), score_err=float(e_s.max()), bound_at_0=float(BU.mixed_bound(T, cw, bw, 0.0)))
    assert (e_s <= BU.mixed_bound(T, cw, bw, want_s)).all()


def test_default_weights_return_what_a_call_without_the_keywords_returns():
    B, R, T, Ks = 16, 5, 21, 3
    hyp, ref, count = BU.make_corpus(B, R, T, 2, 0)
    gen, greedy, refs = torch.from_numpy(hyp[:B]).to(DEV), torch.from_numpy(hyp[B:]).to(DEV), _refs(ref, count, DEV)
    for tab in (None, U.table(T, 0)):
        r0, s0 = SC.self_critical_reward_device(greedy, refs, gen, df=tab)
        r1, s1 = SC.self_critical_reward_device(greedy, refs, gen, df=tab, cider_weight=1.0, bleu_weight=0.0)
        assert s0.cpu().numpy().any() and same_bits(s0.cpu(), s1.cpu()) and same_bits(r0.contiguous().cpu(), r1.contiguous().cpu())
        assert r0.shape == r1.shape and r0.stride() == r1.stride()
    hyp3, ref3, count3 = BU.make_corpus(B, R, T, Ks, 1)
    h3, refs3 = torch.from_numpy(hyp3).to(DEV), _refs(ref3, count3, DEV)
    r0, s0 = SC.self_critical_reward_group_device(h3, refs3, Ks)
    r1, s1 = SC.self_critical_reward_group_device(h3, refs3, Ks, cider_weight=1, bleu_weight=0)
    assert s0.cpu().numpy().any() and same_bits(s0.cpu(), s1.cpu()) and same_bits(r0.contiguous().cpu(), r1.contiguous().cpu())
    with pytest.raises(ValueError):
        SC.self_critical_reward_device(greedy, refs, gen, cider_weight=0.0, bleu_weight=0.0)
    with pytest.raises(ValueError):
        SC.self_critical_reward_group_device(h3, refs3, Ks, cider_weight=-1.0, bleu_weight=1.0)


# ---- (6) the step and the entry script ------------------------------------------------------------------------------------------------
def test_scst_step_with_weights_host_and_device_agree(monkeypatch):
    """scst_step(reward_weights=(1, 0.5)) from the same state with the reward on the host and on the device: the same samples, rewards that
    are not all zero and agree within the bound of a mixed score, the same loss."""
    from oracle import vlp_oracle as O
    from tests.test_80_scst_gpu import _decoder
    from vlp_amd import run_img2txt_dist as R
    from vlp_amd.optimization_fp16 import FP16_Optimizer_State, FusedAdam
    V, B, max_len_b = 1024, 5, 12
    T = max_len_b + 1
    cw, bw = 1.0, 0.5
    words = list(range(300, 306))
    rng = np.random.RandomState(5)
    p = O.init_params(vocab_size=V, layers=2, seed=21, std=0.05)
    # an untrained model shares nothing with its ground truth; a bias towards the six words of the captions (and [SEP]) makes the samples
    # overlap with the references, so the rewards are not all zero (as tests/test_83_scst_samples_gpu.py does)
    p["cls.predictions.bias"][words] = 8.0
    p["cls.predictions.bias"][S.SEP_ID] = 7.0
    batch = S.batch_to(S.make_batch(B, max_len_b=max_len_b, len_vis_input=100, vocab_size=V, max_pred=0, mask_prob=0.0, seed=7), DEV, half=True)
    ids = batch.input_ids.clone()
    for b in range(B):
        row = [int(t) for t in rng.choice(words, size=rng.randint(3, max_len_b + 1))] + [S.SEP_ID]
        ids[b, 102:] = torch.tensor(row + [0] * (T - len(row)), device=DEV)
    batch = batch._replace(input_ids=ids)
    log = []
    real_host, real_dev = SC.self_critical_reward, SC.self_critical_reward_device

    def host(greedy, gt, gen, n, **kw):
        r, s = real_host(greedy, gt, gen, n, **kw)
        log.append(("host", kw, gen.detach().cpu().numpy(), greedy.detach().cpu().numpy(), r, np.asarray(s)))
        return r, s

    def dev(greedy, refs, gen, **kw):
        r, s = real_dev(greedy, refs, gen, **kw)
        log.append(("device", kw, gen.detach().cpu().numpy(), greedy.detach().cpu().numpy(), r.detach().cpu().numpy().copy(), s.detach().cpu().numpy().copy()))
        return r, s
    monkeypatch.setattr(SC, "self_critical_reward", host)
    monkeypatch.setattr(SC, "self_critical_reward_device", dev)
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
        marks[mode] = []
        loss, mean_r = R.scst_step(m, opt, batch, 1e-4, 100, SC.RewardCriterion(), mark=marks[mode].append, reward_on=mode, reward_weights=(cw, bw))
        torch.cuda.synchronize()
        out[mode] = (float(loss.detach()), float(mean_r))
    assert marks["host"] == ["greedy_decode", "sample_forward", "reward_host", "backward", "optimizer"]
    assert marks["device"] == ["greedy_decode", "sample_forward", "reward_device", "backward", "optimizer"]
    (ka, kwa, gen_a, gre_a, r_a, s_a), (kb, kwb, gen_b, gre_b, r_b, s_b) = log
    assert (ka, kb) == ("host", "device") and kwa == kwb == {"cider_weight": cw, "bleu_weight": bw}
    assert np.array_equal(gen_a, gen_b) and np.array_equal(gre_a, gre_b)                 # the same sampled ids
    assert np.count_nonzero(r_a[:, 0]) >= B // 2, r_a[:, 0]
    bound = float(BU.mixed_bound(T, cw, bw, np.abs(s_a).max()))
    e_s = float(np.abs(s_b.astype(np.float64) - s_a).max())
    e_r = float(np.abs(r_b.astype(np.float64) - r_a).max())
    report("scst_step_weights_1_0.5", score_err=e_s, reward_err=e_r, bound=bound, host=out["host"], device=out["device"],
           host_reward=[round(float(v), 6) for v in r_a[:, 0]])
    assert e_s <= bound and e_r <= bound
    assert np.isfinite(out["host"][0]) and abs(out["host"][0] - out["device"][0]) < 0.0048   # test_81's tolerance for this model's log-probs
    assert abs(out["host"][1] - out["device"][1]) <= bound                                   # the mean of rewards that agree within the bound


def test_entry_script_with_the_two_flags(tmp_path, monkeypatch):
    from tests.test_80_scst_gpu import BASE, _ce_checkpoint
    from vlp_amd import run_img2txt_dist as R
    ckpt = _ce_checkpoint(R, tmp_path)
    seen = []
    real_step = R.scst_step

    def step(*a, **kw):
        marks = []
        out = real_step(*a, mark=marks.append, **kw)
        seen.append((kw.get("reward_weights"), kw.get("samples"), kw.get("reward_on"), marks))
        return out
    monkeypatch.setattr(R, "scst_step", step)
    runs = {"device_k2": (["--scst_bleu_weight", "0.5", "--scst_reward", "device", "--scst_samples", "2"], (1.0, 0.5), 2, "device",
                          ["sample_forward", "reward_device", "backward", "optimizer"]),
            "bleu_only": (["--scst_cider_weight", "0", "--scst_bleu_weight", "1"], (0.0, 1.0), 1, "host",
                          ["greedy_decode", "sample_forward", "reward_host", "backward", "optimizer"])}
    logged = {}
    for name, (flags, weights, samples, where, marks) in runs.items():
        del seen[:]
        out = os.path.join(tmp_path, name)
        R.main(BASE + ["--scst"] + flags + ["--synthetic", "2", "--learning_rate", "1e-4", "--model_recover_path", ckpt, "--output_dir", out,
                                           "--num_train_epochs", "1"])
        log = open(os.path.join(out, "training.log")).read()
        losses = [float(x) for x in re.findall(r"Loss (\S+), Mean R", log)]
        mean_r = [float(x) for x in re.findall(r"Mean R (\S+)", log)]
        assert len(losses) == 2 and all(np.isfinite(v) and abs(v) < 1e4 for v in losses), log
        assert len(mean_r) == 2 and all(np.isfinite(v) for v in mean_r), log
        assert seen == [(weights, samples, where, marks)] * 2, seen
        assert os.path.exists(os.path.join(out, "model.1.bin"))
        logged[name] = dict(losses=losses, mean_r=mean_r)
    report("entry_script_flags", **logged)
