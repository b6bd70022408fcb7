"""GPU: the SCST reward on the device (vlp_cider_d, csrc/reward.hip) against the project's own host scorer (vlp_amd.scst.CiderD, fp64).

(1) the kernel against CiderD.compute_score on seeded corpora whose scores are not trivially zero (asserted on the host scorer first);
(2) hand-built hard rows inside one G = 6, R = 3, T = 8 case; garbage behind a row's first 0 and invalid reference rows change no bit;
(3) the contract: strided rows with poisoned padding, guard bands around every output and the workspace, bit-equal repeats, refusals by
    return code;
(4) self_critical_reward_device captured into a graph (no host round trip, no synchronisation) and replayed on new inputs;
(5) scst_step with --scst_reward host and device from the same state: same samples, rewards within the bound, same loss; the entry script
    with --scst_refs image on either side.

Bound: every score within (4 T + 16) * 2^-24 * 10 of the fp64 host value -- a score is at most 10 and a sum of at most 4 T non-negative
products of a few fp32 operations each; a wrong count moves a score by 1e-2 or more.  An fp32 restatement of the host class differs from fp64
by at most 1.4e-6 on these corpora.  Every test prints what it measured through report() (pytest -s); the figures of an MI355X run are in profiles/scst_reward_device.json."""
import json
import os
import re
from collections import OrderedDict

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from tests import guard_util as GU                                  # noqa: E402
from vlp_amd import _lib as K                                       # noqa: E402
from vlp_amd import scst as SC                                      # noqa: E402
from vlp_amd import synthetic as S                                  # noqa: E402
from vlp_amd.input_prep import CaptionRefs                          # noqa: E402

DEV = torch.device("cuda:0")
REPORT = {}
SEP = 102


def report(key, **kw):
    """Prints what a test measured; with VLP_SCST_REWARD_RECORD=<json file> (profiles/scst_reward_device.json when the record is taken) the
    figures are also kept under that file's "test_81" key, next to the timing runs tools/scst_bench.py writes there."""
    REPORT.setdefault(key, {}).update(kw)
    print("%s: %s" % (key, json.dumps(REPORT[key], sort_keys=True)))
    path = os.environ.get("VLP_SCST_REWARD_RECORD")
    if path:
        rec = json.load(open(path)) if os.path.exists(path) else {}
        rec.setdefault("test_81", {})[key] = REPORT[key]
        with open(path, "w") as f:
            json.dump(rec, f, indent=2, sort_keys=True)


def bound(T):
    return (4 * T + 16) * 2.0 ** -24 * 10


# ---- corpus and host scorer -----------------------------------------------------------------------------------------------------------
def make_corpus(G, R, T, mult, seed):
    """12-word vocabulary 1000..1011; reference lengths uniform in 1..T, [SEP] as the last kept token of a reference shorter than T, then
    zeros; ref_count uniform in 1..R; a hypothesis is a copy of one valid reference of its group with 30 % of its non-zero ids redrawn."""
    rng = np.random.RandomState(seed)
    ref = np.zeros((G, R, T), dtype=np.int64)
    count = rng.randint(1, R + 1, size=G).astype(np.int32)
    for g in range(G):
        for r in range(R):
            n = rng.randint(1, T + 1)
            ref[g, r, :n] = rng.randint(1000, 1012, size=n)
            if n < T:
                ref[g, r, n - 1] = SEP
    hyp = np.zeros((mult * G, T), dtype=np.int64)
    for i in range(mult * G):
        g = i % G
        row = ref[g, rng.randint(count[g])].copy()
        redraw = (rng.rand(T) < 0.3) & (row != 0)
        row[redraw] = rng.randint(1000, 1012, size=int(redraw.sum()))
        hyp[i] = row
    return hyp, ref, count


def host_scores(hyp, ref, count, mult):
    """CiderD.compute_score on the strings array_to_str makes: hypothesis i against the first count[g] references of group g = i % G."""
    G = ref.shape[0]
    gts, res = OrderedDict(), OrderedDict()
    for i in range(mult * G):
        g = i % G
        res[i] = [SC.array_to_str(hyp[i].tolist())]
        gts[i] = [SC.array_to_str(r) for r in ref[g, :count[g]].tolist()]
    return SC.CiderD(df="corpus").compute_score(gts, res)[1]


def run_kernel(hyp, ref, count, mult, want_reward=None):
    G = ref.shape[0]
    want_reward = mult == 2 if want_reward is None else want_reward
    h, r = torch.from_numpy(hyp).to(DEV), torch.from_numpy(ref).to(DEV)
    c = torch.from_numpy(count).to(DEV) if count is not None else None
    scores = torch.full((mult * G,), float("nan"), device=DEV)
    reward = torch.full((G,), float("nan"), device=DEV) if want_reward else None
    K.cider_d(h, r, c, mult, scores, reward)
    torch.cuda.synchronize()
    return scores.cpu(), (reward.cpu() if want_reward else None)


# (G, R, T, mult) -> corpus seed.  The seed is chosen on the HOST scorer alone: the first of 0, 1, 2, ... whose corpus meets the condition
# asserted below (at least 90 % non-zero scores for G >= 3).
CASES = [((1, 1, 4, 2), 0), ((3, 1, 5, 2), 0), ((5, 3, 21, 2), 2), ((16, 1, 21, 1), 0), ((64, 5, 21, 2), 0), ((65, 2, 64, 2), 1), ((2, 8, 1, 2), 0),
         ((4, 2, 2, 2), 0), ((4, 2, 3, 2), 1)]


@pytest.mark.parametrize("shape,seed", CASES, ids=["G%d_R%d_T%d_m%d" % c[0] for c in CASES])
def test_kernel_against_host_scorer(shape, seed):
    G, R, T, mult = shape
    hyp, ref, count = make_corpus(G, R, T, mult, seed)
    want = host_scores(hyp, ref, count, mult)
    # the comparison is not one of zeros with zeros (looked at before the kernel's output)
    nz = float(np.mean(want != 0))
    if G >= 3:
        assert nz >= 0.9, nz
    if G == 1:
        assert not want.any()                      # df equals the number of sets: every weight is 0 -- the zero-norm case
    got, reward = run_kernel(hyp, ref, count, mult)
    err = float(np.abs(got.double().numpy() - want).max())
    nz_r = float(np.mean((want[:G] - want[G:]) != 0)) if mult == 2 else None
    report("kernel_G%d_R%d_T%d_m%d" % shape, max_abs_err=err, bound=bound(T), nonzero_scores=nz, nonzero_rewards=nz_r, max_score=float(want.max()))
    assert err <= bound(T), (err, bound(T))
    if mult == 2:
        assert torch.equal(reward, got[:G] - got[G:])            # one fp32 subtraction of the kernel's own scores, bit for bit


# ---- hand-built hard rows -------------------------------------------------------------------------------------------------------------
def hard_case(garbage=True):
    """G = 6, R = 3, T = 8, mult = 2.  Word 1009 occurs in every group's valid references.  garbage=False: the same case with everything
    behind a row's first 0, and every invalid reference row, zeroed."""
    G, R, T = 6, 3, 8
    _, ref, count = make_corpus(G, R, T, 2, 5)
    hyp = np.zeros((2 * G, T), dtype=np.int64)
    count[:] = [1, 2, 2, 3, 1, 2]
    ref[0, 0] = [1000, 1001, 1002, 1009, SEP, 0, 0, 0]
    ref[1, 0] = [1001, 1001, 1004, 1009, SEP, 0, 0, 0]
    ref[1, 1] = [1005, 1001, 1001, 1001, 1001, SEP, 0, 0]
    ref[2, 0] = [1006, 1007, 1008, 1009, 1010, 1011, 1006, 1007]            # no 0 at all
    ref[2, 1] = [1011, 1010, 1009, 1008, 1007, 1006, 1011, 1010]
    for g in (3, 4, 5):
        ref[g, 0, 0] = 1009
    hyp[0] = ref[0, 0]                                                      # equal to its reference
    hyp[G + 0] = [1001, 1001, 1001, 1001, 1001, SEP, 0, 0]                  # one repeated word against group 0: tf 5, clipped to the reference's 1
    hyp[1] = [1001] * 8                                                     # one repeated word, no 0 at all: tf 8 against tf 2 and tf 4
    hyp[G + 1] = [0, 1001, 1001, 1004, 1009, SEP, 1001, 1001]               # starts with 0: one unigram, no bigram, length 0
    hyp[2] = [1004, 1005, 1004, 1005, 1003, 1002, 1004, 1005]               # words of other groups' references only: df > 0, r_g = 0
    hyp[G + 2] = [1009, 1009, 1009, SEP, 0, 0, 0, 0]                        # the word of every group: weight exactly 0
    for g in (3, 4, 5):
        hyp[g] = ref[g, 0]
        hyp[G + g] = ref[g, count[g] - 1]
        hyp[G + g, 1] = 1003
    # garbage behind the first 0: ids that occur in the references
    for row in (hyp[0], hyp[G + 0], hyp[G + 2], ref[0, 0], ref[1, 0], ref[1, 1]):
        z = int(np.flatnonzero(row == 0)[0])
        row[z + 1:] = ([1001, 1009, 1000, 1004, SEP, 1002, 1005] * 2)[:T - z - 1] if garbage else 0
    if not garbage:
        hyp[G + 1, 1:] = 0
    # invalid reference rows r >= count[g]: the group's own hypotheses
    for g in range(G):
        for r in range(count[g], R):
            ref[g, r] = hyp[g if r % 2 else G + g] if garbage else 0
    return hyp, ref, count


def test_hard_rows():
    G, T = 6, 8
    hyp, ref, count = hard_case(True)
    want = host_scores(hyp, ref, count, 2)
    got, reward = run_kernel(hyp, ref, count, 2)
    err = np.abs(got.double().numpy() - want)
    report("hard_rows", max_abs_err=float(err.max()), bound=bound(T), host=[round(float(v), 6) for v in want])
    assert float(err.max()) <= bound(T), (err, bound(T))
    assert torch.equal(reward, got[:G] - got[G:])
    # what the rows were built for, on the host scorer
    assert abs(want[0] - 10.0) < 1e-9                       # equal to its one reference
    assert 0 < want[G + 0] < 10 and 0 < want[1] < 10        # clipped repeats
    assert want[2] == 0 and float(got[2]) == 0.0            # no n-gram of its own group's references
    assert want[G + 2] == 0 and float(got[G + 2]) == 0.0    # only the everywhere-word and [SEP] 0 ... : every shared weight is exactly 0
    # garbage behind the first 0 and invalid reference rows change no bit
    hyp0, ref0, count0 = hard_case(False)
    assert np.array_equal(count, count0) and not np.array_equal(ref, ref0) and not np.array_equal(hyp, hyp0)
    assert np.array_equal(host_scores(hyp0, ref0, count0, 2), want)
    got0, reward0 = run_kernel(hyp0, ref0, count0, 2)
    assert torch.equal(got.view(torch.int32), got0.view(torch.int32)) and torch.equal(reward.view(torch.int32), reward0.view(torch.int32))


# ---- contract -------------------------------------------------------------------------------------------------------------------------
def test_contract_guards_strides_and_determinism():
    G, R, T, mult = 5, 3, 21, 2
    hyp, ref, count = make_corpus(G, R, T, mult, 2)
    plain, plain_r = run_kernel(hyp, ref, count, mult)
    # rows with strides larger than T; the padding and the guards hold 1000, a real word
    gh = GU.guarded(mult * G, T, ld=T + 5, dtype=torch.int64, fill=1000, device=DEV).set(torch.from_numpy(hyp).to(DEV))
    gr = GU.guarded(G * R, T, ld=T + 3, dtype=torch.int64, fill=1000, device=DEV).set(torch.from_numpy(ref.reshape(G * R, T)).to(DEV))
    gc = GU.guarded_vec(G, dtype=torch.int32, fill=R, device=DEV)
    gc.vec.copy_(torch.from_numpy(count).to(DEV))
    gc.seal()
    ref_view = gr.full.view(G, R, T + 3)[:, :, :T]
    assert ref_view.stride() == (R * (T + 3), T + 3, 1) and gh.view.stride() == (T + 5, 1)
    need = K.cider_d_workspace_bytes(G, R, T, mult)
    assert need > 0
    outs = []
    for _ in range(2):
        gs = GU.guarded_vec(mult * G, dtype=torch.float32, fill="sentinel", device=DEV)
        gw = GU.guarded_vec(G, dtype=torch.float32, fill="sentinel", device=DEV)
        ws = GU.guarded_vec(need, dtype=torch.uint8, fill="sentinel", device=DEV)
        K.cider_d(gh.view, ref_view, gc.vec, mult, gs.vec, gw.vec, workspace=ws.vec)
        torch.cuda.synchronize()
        for g, name, written in ((gs, "scores", "logical"), (gw, "reward", "logical"), (ws, "workspace", "logical"), (gh, "hyp", None),
                                 (gr, "ref", None), (gc, "ref_count", None)):
            GU.assert_untouched(g, written=written, name=name)
        GU.assert_written(gs, name="scores")
        GU.assert_written(gw, name="reward")
        outs.append((gs.vec.clone().cpu(), gw.vec.clone().cpu()))
    assert torch.equal(outs[0][0].view(torch.int32), outs[1][0].view(torch.int32)) and torch.equal(outs[0][1].view(torch.int32), outs[1][1].view(torch.int32))
    assert torch.equal(outs[0][0].view(torch.int32), plain.view(torch.int32)) and torch.equal(outs[0][1].view(torch.int32), plain_r.view(torch.int32))
    # ref_count = NULL means all R
    all_r, _ = run_kernel(hyp, ref, None, mult)
    full, _ = run_kernel(hyp, ref, np.full(G, R, dtype=np.int32), mult)
    assert torch.equal(all_r.view(torch.int32), full.view(torch.int32))
    assert float(np.abs(full.double().numpy() - host_scores(hyp, ref, np.full(G, R, dtype=np.int32), mult)).max()) <= bound(T)


@pytest.mark.parametrize("what", ["T65", "R9", "G0", "mult3", "reward_mult1", "workspace_short"])
def test_refusals_by_return_code(what):
    G, R, T, mult = {"T65": (2, 1, 65, 2), "R9": (2, 9, 4, 2), "G0": (0, 1, 4, 2), "mult3": (2, 1, 4, 3)}.get(what, (2, 2, 4, 1 if what == "reward_mult1" else 2))
    hyp = torch.full((max(mult * G, 1), T), 1000, dtype=torch.int64, device=DEV)[:mult * G]
    ref = torch.full((max(G, 1), R, T), 1000, dtype=torch.int64, device=DEV)[:G]
    gs = GU.guarded_vec(max(mult * G, 1), dtype=torch.float32, fill="sentinel", device=DEV)
    gw = GU.guarded_vec(max(G, 1), dtype=torch.float32, fill="sentinel", device=DEV)
    need = K.cider_d_workspace_bytes(G, R, T, mult)
    if what in ("reward_mult1", "workspace_short"):
        assert need > 0
        K.cider_d(hyp, ref, None, mult, gs.vec, None if mult == 1 else gw.vec, workspace=torch.empty(need, dtype=torch.uint8, device=DEV))      # the shape itself is fine
        gs.fill_all("sentinel")
        gw.fill_all("sentinel")
        gs.seal()
        gw.seal()
    else:
        assert need == 0
    ws = GU.guarded_vec(max(need - 1, 16) if what == "workspace_short" else max(need, 4096), dtype=torch.uint8, fill="sentinel", device=DEV)
    if what == "workspace_short":
        assert ws.vec.numel() == need - 1
    with pytest.raises(RuntimeError, match=r"vlp_cider_d.*status -1"):
        K.cider_d(hyp, ref, None, mult, gs.vec, gw.vec, workspace=ws.vec)
    torch.cuda.synchronize()
    for g, name in ((gs, "scores"), (gw, "reward"), (ws, "workspace")):
        GU.assert_untouched(g, written=None, name=name)             # nothing was launched


# ---- no host round trip ---------------------------------------------------------------------------------------------------------------
def _scst_case(B, R, T, seed):
    hyp, ref, count = make_corpus(B, R, T, 2, seed)
    return hyp[:B], hyp[B:], ref, count


def test_device_reward_is_capturable_and_replays_on_new_inputs():
    B, R, T = 16, 5, 21
    gen, greedy, ref, count = _scst_case(B, R, T, 0)
    s_gen, s_greedy = torch.from_numpy(gen).to(DEV), torch.from_numpy(greedy).to(DEV)
    refs = CaptionRefs(torch.from_numpy(ref).to(DEV), torch.from_numpy(count).to(DEV))
    scores = torch.zeros(2 * B, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        SC.self_critical_reward_device(s_greedy, refs, s_gen, scores_out=scores)        # warm-up: code objects loaded before the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):                                           # any synchronising call fails the capture
        reward, sc = SC.self_critical_reward_device(s_greedy, refs, s_gen, scores_out=scores)
    assert sc is scores and tuple(reward.shape) == (B, T) and reward.dtype == torch.float32 and reward.is_cuda
    # new inputs into the static tensors, then replay
    gen2, greedy2, ref2, count2 = _scst_case(B, R, T, 3)
    s_gen.copy_(torch.from_numpy(gen2))
    s_greedy.copy_(torch.from_numpy(greedy2))
    refs.ids.copy_(torch.from_numpy(ref2))
    refs.count.copy_(torch.from_numpy(count2))
    graph.replay()
    torch.cuda.synchronize()
    want_r, want_s = SC.self_critical_reward_refs(greedy2, CaptionRefs(torch.from_numpy(ref2), torch.from_numpy(count2)), gen2)
    assert np.count_nonzero(want_r[:, 0]) >= B // 2
    e_s = float(np.abs(scores.double().cpu().numpy() - want_s).max())
    e_r = float(np.abs(reward.double().cpu().numpy() - want_r).max())
    report("graph_replay", score_err=e_s, reward_err=e_r, bound=bound(T))
    assert e_s <= bound(T) and e_r <= bound(T)
    assert torch.equal(reward[:, 0], scores[:B] - scores[B:]) and torch.equal(reward, reward[:, :1].expand(B, T))
    # the single-reference form: [B, T] ground-truth ids, a strided view like input_ids[:, Nv + 2:]
    wide = torch.zeros(B, 102 + T, dtype=torch.long, device=DEV)
    wide[:, 102:] = torch.from_numpy(ref2[:, 0])
    r1, s1 = SC.self_critical_reward_device(s_greedy, wide[:, 102:], s_gen)
    w1, ws1 = SC.self_critical_reward(greedy2, ref2[:, 0], gen2, B)
    assert float(np.abs(s1.double().cpu().numpy() - ws1).max()) <= bound(T)
    assert float(np.abs(r1.double().cpu().numpy() - w1).max()) <= bound(T)


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
OFFSET = (0.5, -0.75)          # the signed offset of test_80's _signed_reward: an untrained model's true reward is mostly 0


def _install_signed_rewards(monkeypatch, log=None):
    """Both reward paths + the same signed offset per sample (added on the device for the device path)."""
    real_host, real_refs, real_dev = SC.self_critical_reward, SC.self_critical_reward_refs, SC.self_critical_reward_device

    def off_np(B):
        return np.where(np.arange(B) % 2 == 0, OFFSET[0], OFFSET[1])[:, None]

    def host(greedy, gt, gen, B, scorer=None):
        r, s = real_host(greedy, gt, gen, B, scorer)
        if log is not None:
            log.append(("host", gen.detach().clone(), greedy.detach().clone(), r + off_np(B)))
        return r + off_np(B), s

    def refs(greedy, rf, gen):
        r, s = real_refs(greedy, rf, gen)
        return r + off_np(len(gen)), s

    def dev(greedy, rf, gen, scores_out=None):
        r, s = real_dev(greedy, rf, gen, scores_out)
        B = gen.shape[0]
        off = torch.where(torch.arange(B, device=gen.device) % 2 == 0, OFFSET[0], OFFSET[1]).to(torch.float32).unsqueeze(1)
        if log is not None:
            log.append(("device", gen.detach().clone(), greedy.detach().clone(), r + off))
        return r + off, s
    monkeypatch.setattr(SC, "self_critical_reward", host)
    monkeypatch.setattr(SC, "self_critical_reward_refs", refs)
    monkeypatch.setattr(SC, "self_critical_reward_device", dev)


def test_scst_step_host_and_device_agree(monkeypatch):
    from oracle import vlp_oracle as O
    from tests.test_80_scst_gpu import _decoder
    from vlp_amd import run_img2txt_dist as R
    from vlp_amd.optimization_fp16 import FP16_Optimizer_State, FusedAdam
    V, B, max_len_b = 1024, 5, 12
    p = O.init_params(vocab_size=V, layers=2, seed=21, std=0.05)
    batch = S.batch_to(S.make_batch(B, max_len_b=max_len_b, len_vis_input=100, vocab_size=V, max_pred=0, mask_prob=0.0, seed=7), DEV, half=True)
    log = []
    _install_signed_rewards(monkeypatch, log)
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
        loss, mean_r = R.scst_step(m, opt, batch, 1e-4, 100, SC.RewardCriterion(), mark=marks[mode].append, reward_on=mode)
        torch.cuda.synchronize()
        losses[mode] = (float(loss.detach()), float(mean_r))
    (ka, gen_a, greedy_a, r_a), (kb, gen_b, greedy_b, r_b) = log
    assert (ka, kb) == ("host", "device")
    assert marks["host"][2] == "reward_host" and marks["device"][2] == "reward_device"
    assert torch.equal(gen_a, gen_b) and torch.equal(greedy_a, greedy_b)                # the same sampled ids
    T = gen_a.shape[1]
    e_r = float(np.abs(r_b.double().cpu().numpy() - r_a).max())
    report("scst_step_host_vs_device", reward_err=e_r, bound=bound(T), loss_host=losses["host"][0], loss_device=losses["device"][0],
           mean_r_host=losses["host"][1], mean_r_device=losses["device"][1])
    assert e_r <= bound(T)
    assert abs(losses["host"][0] - losses["device"][0]) < 0.0048                        # test_80's bound for this model's log-probs (small case)
    assert abs(losses["host"][1] - losses["device"][1]) <= bound(T)                     # the mean of rewards that agree within the bound


def test_entry_script_image_references_on_host_and_device(tmp_path, monkeypatch):
    from tests.test_60_data_gpu import make_store
    from tests.test_80_scst_gpu import BASE, _ce_checkpoint
    from vlp_amd import run_img2txt_dist as R
    monkeypatch.setenv("VLP_ALLOW_RANDOM_FC7", "1")
    ckpt = _ce_checkpoint(R, tmp_path)
    _install_signed_rewards(monkeypatch)
    store_dir = os.path.join(tmp_path, "store")
    os.makedirs(store_dir)
    _, examples, *_ = make_store(store_dir, n=4, seed=2)
    tok = os.path.join(tmp_path, "tokens.json")
    json.dump([[i, t] for i, t in examples[:8]], open(tok, "w"))                      # 4 images x 2 captions: two steps of 4
    logged = {}
    for mode in ("device", "host"):
        out = os.path.join(tmp_path, mode)
        R.main(BASE + ["--scst", "--scst_reward", mode, "--scst_refs", "image", "--learning_rate", "1e-4", "--model_recover_path", ckpt, "--output_dir", out,
                       "--num_train_epochs", "1", "--packed_features", store_dir, "--token_file", tok, "--always_truncate_tail", "--num_workers", "1"])
        log = open(os.path.join(out, "training.log")).read()
        losses = [float(x) for x in re.findall(r"Loss (\S+), Mean R", log)]
        mean_r = re.findall(r"Mean R (\S+)", log)
        assert len(losses) == 2 and all(np.isfinite(v) and abs(v) < 1e4 for v in losses), log
        assert len(mean_r) == 2 and all(np.isfinite(float(v)) for v in mean_r), log
        logged[mode] = (losses, mean_r)
    report("entry_scst_image_refs", device=logged["device"], host=logged["host"])
    assert logged["device"][1] == logged["host"][1]                                  # the same mean reward to the printed precision

