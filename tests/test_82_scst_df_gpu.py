"""GPU: the SCST reward with document frequencies from a resident table (vlp_cider_d_df, csrc/reward.hip) against the project's own host scorer
in its table mode (vlp_amd.scst.CiderD(df=<DocFreq>), fp64).  tests/test_scst_df_cpu.py checks that scorer against an independent
restatement; tests/scst_df_util.py holds what the two files share.

(a) the kernel against CiderD(df=table) on the seeded corpora of test_81 with two 200-image tables, one of them with every df and n_docs
    x 16 000 (n_docs 3.2 M: df that no narrow field holds).  Asserted on the host scorer alone, before the kernel's output is looked at: every
    score is non-zero for every shape -- with a table G = 1 is no longer the all-zero case it is with df='corpus' --, 5 % .. 50 % of the
    hypothesis n-grams miss the table (T >= 3; shorter strings never miss), and an fp32 restatement of the host class stays within a quarter
    of the bound;
(b) hand-built hard rows inside one G = 6, R = 3, T = 8 case (scst_df_util.hard_case says what each row is for), tables of 0, 1, 2, 3 keys and
    of a non-power of two; garbage behind a row's first 0 and invalid reference rows change no bit;
(c) the contract: strided rows with poisoned padding, guard bands around every output, the workspace and both table arrays, bit-equal repeats,
    refusals by return code, and vlp_cider_d unchanged by the neighbour;
(d) self_critical_reward_device(..., df=table) captured into a graph and replayed on new inputs;
(e) scst_step with a saved table on --scst_reward host and device from the same state; the entry script with --scst_df train --scst_refs image.

Bound: the project's (4 T + 16) * 2^-24 * 10 of test_81, for the same reason: a score is at most 10 and a sum of at most 4 T non-negative
products of a few fp32 operations each.  Every test prints what it measured through report() (pytest -s); the figures of an MI355X run are in
profiles/scst_reward_df.json."""
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
from tests import scst_df_util as U                                 # noqa: E402
from vlp_amd import _lib as K                                       # noqa: E402
from vlp_amd import scst as SC                                      # noqa: E402
from vlp_amd import synthetic as S                                  # noqa: E402
from vlp_amd.input_prep import CaptionRefs                          # noqa: E402

DEV = torch.device("cuda:0")
REPORT = {}
SEP = U.SEP
bound = U.bound


def report(key, **kw):
    """Prints what a test measured; with VLP_SCST_DF_RECORD=<json file> (profiles/scst_reward_df.json when the record is taken) the figures
    are also kept under that file's "test_82" key, next to the timing runs tools/scst_bench.py writes there."""
    REPORT.setdefault(key, {}).update(kw)
    print("%s: %s" % (key, json.dumps(REPORT[key], sort_keys=True)))
    path = os.environ.get("VLP_SCST_DF_RECORD")
    if path:
        rec = json.load(open(path)) if os.path.exists(path) else {}
        rec.setdefault("test_82", {})[key] = REPORT[key]
        with open(path, "w") as f:
            json.dump(rec, f, indent=2, sort_keys=True)


def run_kernel(hyp, ref, count, mult, tab, want_reward=None):
    G = ref.shape[0]
    want_reward = mult == 2 if want_reward is None else want_reward
    h, r = torch.from_numpy(hyp).to(DEV), torch.from_numpy(ref).to(DEV)
    c = torch.from_numpy(count).to(DEV) if count is not None else None
    keys, vals = tab.to(DEV)
    scores = torch.full((mult * G,), float("nan"), device=DEV)
    reward = torch.full((G,), float("nan"), device=DEV) if want_reward else None
    K.cider_d_df(h, r, c, mult, scores, keys, vals, tab.n_docs, reward)
    torch.cuda.synchronize()
    return scores.cpu(), (reward.cpu() if want_reward else None)


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---- (a) the kernel against the host scorer ---------------------------------------------------------------------------------------------
CORPUS_SEED = {(1, 1, 4, 2): 2}            # the others: 0 (tests/scst_df_util.py says how the seeds were chosen)


@pytest.mark.parametrize("shape", U.SHAPES, ids=["G%d_R%d_T%d_m%d" % s for s in U.SHAPES])
@pytest.mark.parametrize("which", [0, 1], ids=["n200", "n3200000"])
def test_kernel_against_host_scorer(shape, which):
    G, R, T, mult = shape
    hyp, ref, count = U.make_corpus(G, R, T, mult, CORPUS_SEED.get(shape, 0))
    tab = U.table(T, which)
    assert tab.n_docs == (200 * U.SCALE if which else 200) and (int(tab.vals.max()) > 1 << 16) == bool(which)
    want = U.host_scores(hyp, ref, count, mult, df=tab)
    # asserted on the host scorer alone, before the kernel's output is looked at
    nz = float(np.mean(want != 0))
    assert nz == 1.0, nz                              # G = 1 included: with a table it is no longer the all-zero case of df='corpus'
    r32, miss = U.restated_scores(hyp, ref, count, mult, tab, np.float32)
    assert (0.05 <= miss <= 0.5) if T >= 3 else miss == 0, miss
    e32 = float(np.abs(r32 - want).max())
    assert e32 <= bound(T) / 4, (e32, bound(T))
    got, reward = run_kernel(hyp, ref, count, mult, tab)
    err = float(np.abs(got.double().numpy() - want).max())
    report("kernel_G%d_R%d_T%d_m%d_%s" % (shape + ("n3200000" if which else "n200",)), max_abs_err=err, bound=bound(T), nonzero_scores=nz, table_misses=miss,
           fp32_restatement_err=e32, max_score=float(want.max()), table_keys=len(tab), max_df=int(tab.vals.max()))
    assert err <= bound(T), (err, bound(T))
    assert torch.equal(reward, got[:G] - got[G:])                  # one fp32 subtraction of the kernel's own scores, bit for bit


# ---- (b) hand-built hard rows ---------------------------------------------------------------------------------------------------------
def test_hard_rows():
    G, T = 6, 8
    hyp, ref, count = U.hard_case(True)
    tab = U.hard_table()
    N = len(tab)
    assert N & (N - 1) and int(tab.keys[0]) == U.key_of((0,)) and int(tab.keys[-1]) == U.key_of((65534, 65534, 1004, 1009))
    assert int(tab.keys[-1]) > 2 ** 63 > U.key_of((32766, 1001, 32767, 1009)) and U.key_of((32767,)) >= 2 ** 63
    want = U.host_scores(hyp, ref, count, 2, df=tab)
    # what the rows were built for, on the host scorer
    assert abs(want[0] - 10.0) < 1e-9                                           # equal to its one reference, 32766 / 32767 looked up
    assert want[G + 0] == 0                                                     # made of misses: nothing shared
    assert 0 < want[1] < 10 and 0 < want[G + 1] < 10 and 0 < want[2] < 10       # the largest keys; 65535 / 70000 beside n-grams that hit
    assert want[G + 2] == 0                                                     # every n-gram has df == n_docs: zero norm
    careless = U.table_from_dict({(1007,): 1, (1009, 4464): 1}, 6)              # the keys a careless packing of (1006, 65535) / (1009, 70000) forms
    assert careless.get((1006, 65535), 0) == 0 and careless.get((1009, 70000), 0) == 0 and careless.get((1007,), 0) == 1
    got, reward = run_kernel(hyp, ref, count, 2, tab)
    err = np.abs(got.double().numpy() - want)
    report("hard_rows", max_abs_err=float(err.max()), bound=bound(T), host=[round(float(v), 6) for v in want], table_keys=N)
    assert float(err.max()) <= bound(T), (err, bound(T))
    assert torch.equal(reward, got[:G] - got[G:])
    assert float(got[G + 0]) == 0.0 and float(got[G + 2]) == 0.0
    # garbage behind the first 0 and invalid reference rows change no bit
    hyp0, ref0, count0 = U.hard_case(False)
    assert np.array_equal(count, count0) and not np.array_equal(ref, ref0) and not np.array_equal(hyp, hyp0)
    assert np.array_equal(U.host_scores(hyp0, ref0, count0, 2, df=tab), want)
    got0, reward0 = run_kernel(hyp0, ref0, count0, 2, tab)
    assert same_bits(got, got0) and same_bits(reward, reward0)
    # tables of 0, 1, 2, 3 keys (the lowest) and of the three highest keys: every search length from none on
    errs = {}
    for name, sl in (("0", slice(0, 0)), ("1", slice(0, 1)), ("2", slice(0, 2)), ("3", slice(0, 3)), ("top3", slice(N - 3, N))):
        small = SC.DocFreq(tab.keys[sl], tab.vals[sl], tab.n_docs)
        want_s = U.host_scores(hyp, ref, count, 2, df=small)
        assert np.abs(want_s - want).max() > 1e-2                               # another reward than the full table's
        got_s, _ = run_kernel(hyp, ref, count, 2, small)
        errs[name] = float(np.abs(got_s.double().numpy() - want_s).max())
        assert errs[name] <= bound(T), (name, errs[name], bound(T))
    report("hard_rows", small_table_errs=errs)


# ---- (c) contract ---------------------------------------------------------------------------------------------------------------------
def _guarded_table(tab):
    gk = GU.guarded_vec(len(tab), dtype=torch.int64, fill=U.key_of((1000,)), device=DEV)          # guards: a real key
    gk.vec.copy_(torch.from_numpy(tab.keys.view(np.int64)).to(DEV))
    gv = GU.guarded_vec(len(tab), dtype=torch.int32, fill=7, device=DEV)
    gv.vec.copy_(torch.from_numpy(tab.vals).to(DEV))
    return gk.seal(), gv.seal()


def test_contract_guards_strides_and_determinism():
    G, R, T, mult = 5, 3, 21, 2
    hyp, ref, count = U.make_corpus(G, R, T, mult, 0)
    tab = U.table(T, 1)
    plain, plain_r = run_kernel(hyp, ref, count, mult, tab)
    # rows with strides larger than T; the padding and the guards hold 1000, a real word
    gh = GU.guarded(mult * G, T, ld=T + 5, dtype=torch.int64, fill=1000, device=DEV).set(torch.from_numpy(hyp).to(DEV))
    gr = GU.guarded(G * R, T, ld=T + 3, dtype=torch.int64, fill=1000, device=DEV).set(torch.from_numpy(ref.reshape(G * R, T)).to(DEV))
    gc = GU.guarded_vec(G, dtype=torch.int32, fill=R, device=DEV)
    gc.vec.copy_(torch.from_numpy(count).to(DEV))
    gc.seal()
    gk, gv = _guarded_table(tab)
    ref_view = gr.full.view(G, R, T + 3)[:, :, :T]
    assert ref_view.stride() == (R * (T + 3), T + 3, 1) and gh.view.stride() == (T + 5, 1)
    need = K.cider_d_df_workspace_bytes(G, R, T, mult)
    assert need > K.cider_d_workspace_bytes(G, R, T, mult) > 0
    # the neighbour on the same inputs, before and after
    before = torch.full((mult * G,), float("nan"), device=DEV)
    K.cider_d(gh.view, ref_view, gc.vec, mult, before)
    outs = []
    for _ in range(2):
        gs = GU.guarded_vec(mult * G, dtype=torch.float32, fill="sentinel", device=DEV)
        gw = GU.guarded_vec(G, dtype=torch.float32, fill="sentinel", device=DEV)
        ws = GU.guarded_vec(need, dtype=torch.uint8, fill="sentinel", device=DEV)
        K.cider_d_df(gh.view, ref_view, gc.vec, mult, gs.vec, gk.vec, gv.vec, tab.n_docs, gw.vec, workspace=ws.vec)
        torch.cuda.synchronize()
        for g, name, written in ((gs, "scores", "logical"), (gw, "reward", "logical"), (ws, "workspace", "logical"), (gh, "hyp", None),
                                 (gr, "ref", None), (gc, "ref_count", None), (gk, "df_keys", None), (gv, "df_vals", None)):
            GU.assert_untouched(g, written=written, name=name)
        GU.assert_written(gs, name="scores")
        GU.assert_written(gw, name="reward")
        outs.append((gs.vec.clone().cpu(), gw.vec.clone().cpu()))
    assert same_bits(outs[0][0], outs[1][0]) and same_bits(outs[0][1], outs[1][1])
    assert same_bits(outs[0][0], plain) and same_bits(outs[0][1], plain_r)
    after = torch.full((mult * G,), float("nan"), device=DEV)
    K.cider_d(gh.view, ref_view, gc.vec, mult, after)
    torch.cuda.synchronize()
    assert same_bits(before.cpu(), after.cpu())
    assert float(np.abs(after.double().cpu().numpy() - U.host_scores(hyp, ref, count, mult)).max()) <= bound(T)
    # ref_count = NULL means all R
    all_r, _ = run_kernel(hyp, ref, None, mult, tab)
    full, _ = run_kernel(hyp, ref, np.full(G, R, dtype=np.int32), mult, tab)
    assert same_bits(all_r, full)
    assert float(np.abs(full.double().numpy() - U.host_scores(hyp, ref, np.full(G, R, dtype=np.int32), mult, df=tab)).max()) <= bound(T)


REFUSALS = ["T65", "R9", "G0", "mult3", "reward_mult1", "workspace_short", "df_n_negative", "n_docs_0", "n_docs_above_2p24", "keys_null", "vals_null",
            "keys_misaligned", "vals_misaligned"]


@pytest.mark.parametrize("what", REFUSALS)
def test_refusals_by_return_code(what):
    G, R, T, mult = {"T65": (2, 1, 65, 2), "R9": (2, 9, 4, 2), "G0": (0, 1, 4, 2), "mult3": (2, 1, 4, 3)}.get(what, (2, 2, 4, 1 if what == "reward_mult1" else 2))
    hyp = torch.full((max(mult * G, 1), T), 1000, dtype=torch.int64, device=DEV)[:mult * G]
    ref = torch.full((max(G, 1), R, T), 1000, dtype=torch.int64, device=DEV)[:G]
    tab = U.table(4, 0)
    gk, gv = _guarded_table(tab)
    gs = GU.guarded_vec(max(mult * G, 1), dtype=torch.float32, fill="sentinel", device=DEV)
    gw = GU.guarded_vec(max(G, 1), dtype=torch.float32, fill="sentinel", device=DEV)
    need = K.cider_d_df_workspace_bytes(G, R, T, mult)
    if what in ("T65", "R9", "G0", "mult3"):
        assert need == 0
    else:
        assert need > 0                                                   # the shape itself is fine: the same call without the fault runs
        K.cider_d_df(hyp, ref, None, mult, gs.vec, gk.vec, gv.vec, tab.n_docs, None if mult == 1 else gw.vec,
                     workspace=torch.empty(need, dtype=torch.uint8, device=DEV))
        torch.cuda.synchronize()
        gs.fill_all("sentinel")
        gw.fill_all("sentinel")
        gs.seal()
        gw.seal()
    ws = GU.guarded_vec(max(need - 1, 16) if what == "workspace_short" else max(need, 4096), dtype=torch.uint8, fill="sentinel", device=DEV)
    if what == "workspace_short":
        assert ws.vec.numel() == need - 1
    s = K.CiderDArgs(K.ptr(hyp), hyp.stride(0), K.ptr(ref), ref.stride(0), ref.stride(1), None, G, R, T, mult, 6.0, K.ptr(gs.vec), K.ptr(gw.vec),
                     K.ptr(ws.vec), ws.vec.numel())
    kp, vp, n, n_docs = gk.vec.data_ptr(), gv.vec.data_ptr(), len(tab), tab.n_docs
    assert kp % 8 == 0 and vp % 4 == 0
    if what == "df_n_negative":
        n = -1
    elif what == "n_docs_0":
        n_docs = 0
    elif what == "n_docs_above_2p24":
        n_docs = 2 ** 24 + 1
    elif what == "keys_null":
        kp = None
    elif what == "vals_null":
        vp = None
    elif what == "keys_misaligned":
        kp, n = kp + 4, n - 1
    elif what == "vals_misaligned":
        vp, n = vp + 2, n - 1
    a = K.CiderDDfArgs(s, C.c_void_p(kp), C.c_void_p(vp), n, n_docs)
    rc = K.load().vlp_cider_d_df(C.byref(a), K.stream_ptr())
    assert rc == -1, rc
    assert "vlp_cider_d_df" in K.load().vlp_last_error_string().decode()
    torch.cuda.synchronize()
    for g, name in ((gs, "scores"), (gw, "reward"), (ws, "workspace"), (gk, "df_keys"), (gv, "df_vals")):
        GU.assert_untouched(g, written=None, name=name)             # nothing was launched
    # an empty table is legal, with or without pointers: every df is 0
    if what == "keys_null":
        empty = SC.DocFreq(tab.keys[:0], tab.vals[:0], tab.n_docs)
        out = torch.zeros(mult * G, device=DEV)
        K.cider_d_df(hyp, ref, None, mult, out, *empty.to(DEV), empty.n_docs)
        want = U.host_scores(hyp.cpu().numpy(), ref.cpu().numpy(), np.full(G, R, dtype=np.int32), mult, df=empty)
        assert float(np.abs(out.double().cpu().numpy() - want).max()) <= bound(T) and want.min() > 0


# ---- (d) no host round trip -----------------------------------------------------------------------------------------------------------
def _scst_case(B, R, T, seed):
    hyp, ref, count = U.make_corpus(B, R, T, 2, seed)
    return hyp[:B], hyp[B:], ref, count


def test_device_reward_with_table_is_capturable_and_replays_on_new_inputs():
    B, R, T = 16, 5, 21
    tab = U.table(T, 1)
    gen, greedy, ref, count = _scst_case(B, R, T, 0)
    s_gen, s_greedy = torch.from_numpy(gen).to(DEV), torch.from_numpy(greedy).to(DEV)
    refs = CaptionRefs(torch.from_numpy(ref).to(DEV), torch.from_numpy(count).to(DEV))
    scores = torch.zeros(2 * B, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        SC.self_critical_reward_device(s_greedy, refs, s_gen, scores_out=scores, df=tab)     # warm-up: code objects loaded, the table uploaded
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    resident = tab.to(DEV)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):                                           # any synchronising call fails the capture
        reward, sc = SC.self_critical_reward_device(s_greedy, refs, s_gen, scores_out=scores, df=tab)
    assert tab.to(DEV)[0] is resident[0] and tab.to(DEV)[1] is resident[1]               # uploaded once
    assert sc is scores and tuple(reward.shape) == (B, T) and reward.dtype == torch.float32 and reward.is_cuda
    gen2, greedy2, ref2, count2 = _scst_case(B, R, T, 3)
    s_gen.copy_(torch.from_numpy(gen2))
    s_greedy.copy_(torch.from_numpy(greedy2))
    refs.ids.copy_(torch.from_numpy(ref2))
    refs.count.copy_(torch.from_numpy(count2))
    graph.replay()
    torch.cuda.synchronize()
    want_r, want_s = SC.self_critical_reward_refs(greedy2, CaptionRefs(torch.from_numpy(ref2), torch.from_numpy(count2)), gen2, df=tab)
    assert np.count_nonzero(want_r[:, 0]) >= B // 2
    batch_r, _ = SC.self_critical_reward_refs(greedy2, CaptionRefs(torch.from_numpy(ref2), torch.from_numpy(count2)), gen2)
    assert float(np.abs(batch_r - want_r).max()) > 1e-2                                  # not the batch mode's reward
    e_s = float(np.abs(scores.double().cpu().numpy() - want_s).max())
    e_r = float(np.abs(reward.double().cpu().numpy() - want_r).max())
    report("graph_replay", score_err=e_s, reward_err=e_r, bound=bound(T))
    assert e_s <= bound(T) and e_r <= bound(T)
    assert torch.equal(reward[:, 0], scores[:B] - scores[B:]) and torch.equal(reward, reward[:, :1].expand(B, T))
    # the single-reference form: [B, T] ground-truth ids, a strided view like input_ids[:, Nv + 2:]
    wide = torch.zeros(B, 102 + T, dtype=torch.long, device=DEV)
    wide[:, 102:] = torch.from_numpy(ref2[:, 0])
    r1, s1 = SC.self_critical_reward_device(s_greedy, wide[:, 102:], s_gen, df=tab)
    w1, ws1 = SC.self_critical_reward(greedy2, ref2[:, 0], gen2, B, df=tab)
    assert float(np.abs(s1.double().cpu().numpy() - ws1).max()) <= bound(T)
    assert float(np.abs(r1.double().cpu().numpy() - w1).max()) <= bound(T)


# ---- (e) end to end -------------------------------------------------------------------------------------------------------------------
WORDS = list(range(300, 306))


def _captions(n_images, per_image, max_len_b, seed):
    rng = np.random.RandomState(seed)
    return [(i, [int(t) for t in rng.choice(WORDS, size=rng.randint(3, max_len_b + 1))]) for i in range(n_images) for _ in range(per_image)]


def test_scst_step_host_and_device_agree_with_a_saved_table(monkeypatch, tmp_path):
    from oracle import vlp_oracle as O
    from tests.test_80_scst_gpu import _decoder
    from vlp_amd import run_img2txt_dist as R
    from vlp_amd.optimization_fp16 import FP16_Optimizer_State, FusedAdam
    V, B, max_len_b = 1024, 4, 12
    T = max_len_b + 1
    examples = _captions(40, 3, max_len_b, 5)
    path = os.path.join(tmp_path, "df.npz")
    SC.DocFreq.from_examples(examples, max_len_b, SEP).save(path)
    tab = SC.DocFreq.load(path)
    p = O.init_params(vocab_size=V, layers=2, seed=21, std=0.05)
    # an untrained model draws from all 1024 words and shares nothing with its ground truth; a bias towards the six words of the captions
    # (and [SEP]) makes samples, greedy captions and references overlap, so the rewards are not all zero
    p["cls.predictions.bias"][WORDS] = 8.0
    p["cls.predictions.bias"][SEP] = 7.0
    batch = S.batch_to(S.make_batch(B, max_len_b=max_len_b, len_vis_input=100, vocab_size=V, max_pred=0, mask_prob=0.0, seed=7), DEV, half=True)
    ids = batch.input_ids.clone()
    for b in range(B):                                 # the ground truth: the first caption of image b, as the loader lays it out
        row = examples[3 * b][1][:max_len_b] + [SEP]
        ids[b, 102:] = torch.tensor(row + [0] * (T - len(row)), device=DEV)
    batch = batch._replace(input_ids=ids)
    log = []
    real_host, real_dev = SC.self_critical_reward, SC.self_critical_reward_device

    def host(greedy, gt, gen, n, scorer=None, df=None):
        r, s = real_host(greedy, gt, gen, n, scorer, df=df)
        log.append(("host", df, gen.detach().cpu().numpy(), greedy.detach().cpu().numpy(), gt.detach().cpu().numpy(), r))
        return r, s

    def dev(greedy, rf, gen, scores_out=None, df=None):
        r, s = real_dev(greedy, rf, gen, scores_out, df=df)
        log.append(("device", df, gen.detach().cpu().numpy(), greedy.detach().cpu().numpy(), rf.detach().cpu().numpy(), r.detach().clone()))
        return r, s
    monkeypatch.setattr(SC, "self_critical_reward", host)
    monkeypatch.setattr(SC, "self_critical_reward_device", dev)
    losses, marks = {}, {}
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
        loss, mean_r = R.scst_step(m, opt, batch, 1e-4, 100, SC.RewardCriterion(), mark=marks[mode].append, reward_on=mode, df=tab)
        torch.cuda.synchronize()
        losses[mode] = (float(loss.detach()), float(mean_r))
    (ka, dfa, gen_a, greedy_a, gt_a, r_a), (kb, dfb, gen_b, greedy_b, gt_b, r_b) = log
    assert (ka, kb) == ("host", "device") and dfa is tab and dfb is tab
    assert marks["host"][2] == "reward_host" and marks["device"][2] == "reward_device"
    assert np.array_equal(gen_a, gen_b) and np.array_equal(greedy_a, greedy_b) and np.array_equal(gt_a, gt_b)      # the same sampled ids
    assert gen_a.shape[1] == T
    # on the host scorer first: the rewards are not all zero, and they are not the batch mode's on the same samples
    batch_r, _ = real_host(greedy_a, gt_a, gen_a, B)
    differ = float(np.abs(batch_r - r_a).max())
    report("scst_step_host_vs_device", host_reward=[round(float(v), 6) for v in r_a[:, 0]], batch_mode_reward=[round(float(v), 6) for v in batch_r[:, 0]])
    assert np.count_nonzero(r_a[:, 0]) >= 1 and differ > 1e-2, (r_a[:, 0], batch_r[:, 0])
    e_r = float(np.abs(r_b.double().cpu().numpy() - r_a).max())
    report("scst_step_host_vs_device", reward_err=e_r, bound=bound(T), loss_host=losses["host"][0], loss_device=losses["device"][0],
           mean_r_host=losses["host"][1], mean_r_device=losses["device"][1], differs_from_batch_mode_by=differ)
    assert e_r <= bound(T)
    assert abs(losses["host"][0] - losses["device"][0]) < 0.0048                        # test_81's tolerance for this model's log-probs
    assert abs(losses["host"][1] - losses["device"][1]) <= bound(T)                     # the mean of rewards that agree within the bound


def test_entry_script_with_a_table_of_the_training_set(tmp_path, monkeypatch):
    from tests.test_60_data_gpu import make_store
    from tests.test_80_scst_gpu import BASE, _ce_checkpoint
    from vlp_amd import run_img2txt_dist as R
    monkeypatch.setenv("VLP_ALLOW_RANDOM_FC7", "1")
    ckpt = _ce_checkpoint(R, tmp_path)
    store_dir = os.path.join(tmp_path, "store")
    os.makedirs(store_dir)
    _, examples, *_ = make_store(store_dir, n=4, seed=2)
    tok = os.path.join(tmp_path, "tokens.json")
    json.dump([[i, t] for i, t in examples[:8]], open(tok, "w"))                      # 4 images x 2 captions: two steps of 4
    want = SC.DocFreq.from_examples([(i, t) for i, t in examples[:8]], 20, SEP)
    seen = []
    real = R.scst_step

    def spy(*a, **kw):
        seen.append(kw.get("df"))
        return real(*a, **kw)
    monkeypatch.setattr(R, "scst_step", spy)
    logged = {}
    for mode in ("device", "host"):
        out = os.path.join(tmp_path, mode)
        R.main(BASE + ["--scst", "--scst_reward", mode, "--scst_refs", "image", "--scst_df", "train", "--learning_rate", "1e-4", "--model_recover_path", ckpt,
                       "--output_dir", out, "--num_train_epochs", "1", "--packed_features", store_dir, "--token_file", tok, "--always_truncate_tail",
                       "--num_workers", "1"])
        log = open(os.path.join(out, "training.log")).read()
        assert "--scst_df train: %d n-grams over %d images" % (len(want), want.n_docs) in log, log
        losses = [float(x) for x in re.findall(r"Loss (\S+), Mean R", log)]
        mean_r = re.findall(r"Mean R (\S+)", log)
        assert len(losses) == 2 and all(np.isfinite(v) and abs(v) < 1e4 for v in losses), log
        assert len(mean_r) == 2 and all(np.isfinite(float(v)) for v in mean_r), log
        logged[mode] = (losses, mean_r)
    assert len(seen) == 4 and all(isinstance(d, SC.DocFreq) and np.array_equal(d.keys, want.keys) and np.array_equal(d.vals, want.vals) for d in seen)
    report("entry_scst_df_train", device=logged["device"], host=logged["host"])
    assert logged["device"][1] == logged["host"][1]                                  # the same mean reward to the printed precision
