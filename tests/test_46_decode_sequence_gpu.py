"""GPU: a USED caption decoder must equal a FRESH one.

Every other decoder test builds a BertForSeq2SeqDecoder, makes the same call three times (plain run, graph capture, replay) and drops it.
decode_img2txt, sample_img2txt and --scst keep one Engine alive through thousands of calls whose kind, shape and options change, with an
optimizer moving the parameters in between, and the decode side of the engine carries state between them: workspaces keyed ("dec", B, T0,
Lcap, Kb[, "group"]) and kept for life, ws["calls"] (plain run / capture / replay), the captured graphs of ws["plans"] -- which hold by
ADDRESS the parameters, the static input copies, the seed cell, the two beam caches, the n-gram candidate lists and the ignore-list tensors --,
ws["plan_stream"], the n-best and filter outputs, and invalidate().  Here a `used` decoder lives through a scenario; after each of its
calls a `fresh` decoder of the same configuration (a deepcopy of a template that never ran) receives the used one's parameters by copying
engine.flat (bit for bit, asserted) and the same engine.step_seed, and makes only that call -- the plain, uncaptured path.  The decode
path has no atomics, so everything the call returns must be equal BIT FOR BIT (tests/step_seq_util.first_difference): ids and scores /
log-probabilities, the frame tensors and pred_seq of a beam search, every nbest_* entry, filter_cutoff[:T] / filter_kept[:T] of a
filtered draw, and engine.step_seed after the call.  A fresh engine's single call is what test_40 / 41 / 44 / 45 tie to the fp32 oracle
for initial weights; scenario D adds the anchor for UPDATED weights (test_40's rule, its MARGIN_TOL / SCORE_TOL, unchanged).  Skipped
under VLP_AUTOTUNE=1 (timed kernel choices are not reproducible and not the product configuration).

Shapes: vocabulary 1024, 2 layers, hidden 768 (the fused token steps), 100 regions; B = 3 / T = 6 and B = 2 / T = 4 generated tokens; beam 3
and one beam 2; K = 1 and K = 3 samples.  Inputs are tests/decode_seq_util.varied_inputs: besides the image tensors, the number of visible
regions per sample and the position ids change with the seed, so that a stale copy of ANY per-call input shows.  Weights: "peaked"
(std 0.05, six words at bias 8 and [SEP] at 7: beams repeat words and meet eos early, so blocking, min_len and eos_id change the search)
and, for D, "flat" (std 0.1, no bias: wide top-1 / top-2 margins).

Scenarios: A kinds on one engine (greedy, sampling greedy, K = 3, K = 1 tempered, K = 3 filtered, in three rounds); B beam options across
replays, and the plan keys they must leave; C leave a workspace key and come back; D parameters that move (FusedAdam plain / pipelined,
load_state_dict, half() / to()), with the oracle anchor; E another stream; F results belong to the caller.

Oracle anchor (D): seed 461 of varied_inputs(3, 6, .) was picked on the CPU with oracle.greedy_decode on the fp16-rounded "flat" weights:
0 of 18 positions (share 0.000) have a top-1 / top-2 margin under MARGIN_TOL = 1.5e-2 (smallest margin 0.122; seeds 462: 0.000, 463:
0.056, 464: 0.000).  The test asserts share <= 0.2 for the initial AND the updated weights and reports both (profiles/decode_sequence.json:
on an MI355X 18 of 18 tokens compared and no flip either time; after the three updates the share is 0.000 again, the smallest margin
12.8 -- three Adam steps of lr 1e-4 without bias correction move every logit by whole units).

What the scenarios found: Engine.decode_sample_group returned, at K = 1, VIEWS of the workspace's out_ids / out_val (its sample-major
`reshape` is a copy only for K > 1), so model(..., sample_mode="sample", temperature=0.7) or n_samples=1, top_k=5 handed the caller rows
the next call at the same shapes overwrote (test_f, "samples K=1 T=0.7").  Fixed in the engine (vlp_amd.engine.sample_major: one owned
copy for every K).  And Engine._run_planned, on a stream other than the one its plans were made on, made only the FIRST plan it met
again and replayed the others as they were (scenario E): harmless for a captured graph, which launches on the current stream, but a
recorded launch plan -- the fall-back when capture is unavailable -- carries its stream in every launch.  Fixed: a workspace's plans
are set aside as a whole with their stream and come back with it.

MUTATIONS (each made in a scratch copy of vlp_amd/engine.py or modeling.py, never committed; decided from the code beforehand that each
yields a wrong value and no access out of bounds; what this module reports, first failing test and tensor):
  1. `block_eos` dropped from the beam plan key: test_b fails at call 3 (the first min_len = 3 search, which replays the unblocked frames
     1 and 2) -- scores, 2 of 972 elements.
  2. `plan_tag` (n-gram size and ignore list) dropped from the beam plan key: test_b fails at call 5 (the first ngram_size = 2 search,
     which replays unblocked steps) -- pred_seq, 8 of 324 elements.
  3. `filt` dropped from the sample_group plan key: test_a fails at call 8 (K = 3 unfiltered in round 2, which replays the filtered
     steps round 1 captured) -- ids, 7 of 54 elements.
  4. `_decode_static_inputs` returns early once ws["calls"] > 1: test_a fails at call 3 (sampling greedy, the first call on new inputs
     of a workspace that has been called twice: mask and position ids of call 2 stay) -- ids, 5 of 18 elements.
  5. `seed_cell` not refilled once plans exist: test_a fails at call 8 (K = 3 in round 2 draws with round 1's seed) -- ids, 39 of 54.
  6. `invalidate()` keeps self._ws: NOT run.  pack() allocates new flat buffers and drops the old ones, while the kept graphs hold the
     old parameter addresses: a replay would read freed memory, which is a use after free and not merely a wrong value.
  7. the fix of decode_sample_group taken back (`reshape` in sample_major): test_f[samples K=1 T=0.7] fails, the first n_samples = 1
     entry -- held ids, 15 of 18 elements overwritten by the second call (A - E and the three entries in front of it pass).
  8. the `.clone()` of pred_seq / the nbest_* entries in beam_search dropped: test_f[beam n_best=3] fails -- held nbest_score, 9 of 9.
  9. the stream fix of _run_planned taken back (only the plan that meets a new stream is made again): test_e fails after the side-stream
     calls -- the plans ('greedy', 2) .. ('greedy', 5) of the default stream were replayed there.
  With the engine as committed the module passes: 15 tests, about 6.5 s of test time in one process on an MI355X.  Alone it runs on
  captured graphs; inside the whole suite it runs on recorded launch plans (a spy of test_41 reads a tensor back during a capture, the
  capture fails and the engine turns graphs off for the process) -- it passes either way, scenario E included.
"""
import collections
import copy
import functools
import json
import os
import time

import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from oracle import vlp_oracle as O                                              # noqa: E402  (checker only)
from vlp_amd import scst as SC                                                  # noqa: E402
from vlp_amd import synthetic as S                                              # noqa: E402
from vlp_amd import tuning                                                      # noqa: E402
from tests.decode_seq_util import (Call, attrs_of, beam_plan_keys, calls_until_replayed, greedy_plan_keys, margin_share,   # noqa: E402
                                   named_outputs, sample_plan_keys, snapshot, varied_inputs)
from tests.step_seq_util import bit_diff, first_difference                      # noqa: E402
from tests.test_40_decode_gpu import MARGIN_TOL, SCORE_TOL, compare_decodes     # noqa: E402
from tests.test_80_scst_gpu import _decoder                                     # noqa: E402
from tests.test_86_scst_policy_gpu import _optimizer                            # noqa: E402

if tuning.AUTOTUNE:
    pytest.skip("VLP_AUTOTUNE=1: timed kernel choices are not bit-reproducible", allow_module_level=True)

DEV = torch.device("cuda:0")
V, NV, EOS = 1024, 100, S.SEP_ID
REPORT = {}
CLOCK = {}


@pytest.fixture(scope="module", autouse=True)
def _module_clock():
    CLOCK["t0"] = time.time()                # in front of the module's first test (templates, first kernel loads and all)
    yield


def report(key, **kw):
    """Prints what a test measured; with VLP_DECODE_SEQUENCE_RECORD=<json file> (profiles/decode_sequence.json when the record is taken) the
    figures are also kept in that file, with the module's wall time up to the latest report."""
    REPORT.setdefault(key, {}).update(kw)
    print("%s: %s" % (key, json.dumps(REPORT[key], sort_keys=True)))
    path = os.environ.get("VLP_DECODE_SEQUENCE_RECORD")
    if path:
        rec = json.load(open(path)) if os.path.exists(path) else {}
        rec.setdefault("test_46", {})[key] = REPORT[key]
        rec["test_46"]["module"] = {"wall_s": round(time.time() - CLOCK["t0"], 2), "reports": len(REPORT)}
        with open(path, "w") as f:
            json.dump(rec, f, indent=2, sort_keys=True)


# =====================================================================================================================================
# models, inputs, one call
# =====================================================================================================================================
@functools.lru_cache(maxsize=None)
def _params(kind):
    if kind == "flat":
        return O.init_params(vocab_size=V, layers=2, tasks="img2txt", seed=46, std=0.1)
    p = O.init_params(vocab_size=V, layers=2, tasks="img2txt", seed=46, std=0.05)
    p["cls.predictions.bias"][300:306] = 8.0
    p["cls.predictions.bias"][EOS] = 7.0
    return p


@functools.lru_cache(maxsize=None)
def _template(kind, train=False):
    """One model per configuration, built once and never run: every used / fresh decoder is a deepcopy (a new Engine each)."""
    m = _decoder(_params(kind), V, 2)
    return m.train() if train else m.eval()


def _new(template):
    m = copy.deepcopy(template)
    m.engine.pack()
    return m


def _fresh_from(template, used, what):
    """A fresh decoder holding `used`'s current parameters: the flat buffers are copied (fp16 -> fp16, no arithmetic)."""
    m = _new(template)
    used.engine.wait_params()                # (a pipelined optimizer step writes them on its own stream)
    for k, t in used.engine.flat.items():
        m.engine.flat[k].copy_(t)
    for (n, a), (_, b) in zip(m.named_parameters(), used.named_parameters()):
        assert bit_diff(a.data, b.data) == 0, "%s: parameter %s of the fresh decoder differs from the used one's" % (what, n)
    return m


@functools.lru_cache(maxsize=None)
def _inputs(B, T, seed):
    t = varied_inputs(B, T, seed, NV)
    return (t[0].half().to(DEV), t[1].half().to(DEV)) + tuple(x.to(DEV) for x in t[2:])


def _ws(model, B, T, Kb=1, group=False):
    return model.engine._ws[("dec", B, NV + 3, NV + 2 + T, Kb) + (("group",) if group else ())]


def _filtered(kw):
    return (float(kw.get("temperature", 1.0)), int(kw.get("top_k", 0)), float(kw.get("top_p", 1.0))) != (1.0, 0, 1.0)


def _run(model, call, seed):
    """One call of `model`; returns what the call returned (NOT cloned: the caller's own tensors) as an ordered {name: tensor | value}."""
    for k, v in attrs_of(call, EOS).items():
        setattr(model, k, v)
    model.engine.step_seed = seed
    with torch.no_grad():
        res = model(*_inputs(*call.case), task_idx=None, **call.kwargs)
    extra = collections.OrderedDict()
    if _filtered(call.kwargs):               # the kept sets of the draws, which belong to the workspace of the call
        B, T, _ = call.case
        ws = _ws(model, B, T, call.kwargs.get("n_samples", 1), True)
        extra["filter_cutoff"], extra["filter_kept"] = ws["filter_cutoff"][:T], ws["filter_kept"][:T]
    extra["step_seed after the call"] = model.engine.step_seed
    torch.cuda.synchronize()
    return named_outputs(res, extra)


COUNTS = collections.Counter()


def _used_vs_fresh(scenario, i, call, used, template, seed=None):
    """The call on `used`, then alone on a fresh decoder with used's parameters; everything bit-equal."""
    seed = 4600 + 37 * i if seed is None else seed
    what = "scenario %s, call %d (%s, B = %d, T = %d)" % ((scenario, i, call.what) + call.case[:2])
    got = _run(used, call, seed)
    want = _run(_fresh_from(template, used, what), call, seed)
    d = first_difference(got, want)
    assert d is None, "%s: the used decoder differs from a fresh one -- %s" % (what, d)
    COUNTS[scenario] += 1
    return got, want


def _walk(scenario, template, calls, used=None, start=0):
    used = used if used is not None else _new(template)
    outs = [_used_vs_fresh(scenario, start + i, c, used, template)[0] for i, c in enumerate(calls)]
    return used, outs


def _plan_keys(ws):
    return sorted(map(str, ws["plans"]))


def _differ(a, b, keys):
    return any(bit_diff(a[k], b[k]) != 0 for k in keys)


GREEDY = dict()
SAMPLE = dict(sample_mode="sample")
K3 = dict(sample_mode="sample", n_samples=3)
K1_T = dict(sample_mode="sample", n_samples=1, temperature=0.7)
K1_TOPK = dict(sample_mode="sample", n_samples=1, top_k=5)
K3_FILT = dict(sample_mode="sample", n_samples=3, temperature=0.8, top_k=20, top_p=0.9)


def _call(what, case, kwargs=None, **attrs):
    return Call(what, case, attrs, kwargs or {})


# =====================================================================================================================================
# A. kinds on one engine
# =====================================================================================================================================
def test_a_kinds_on_one_engine():
    """search_beam_size = 1, B = 3 / T = 6: greedy x 3 (plain, capture, replay); then three rounds of sampling greedy (never captured, shares
    greedy's workspace), K = 3, K = 1 at temperature 0.7, K = 3 filtered (0.8, 20, 0.9) -- plain run, capture and replay of each, with the
    other kinds in between and other inputs and seeds every round --; then greedy on new inputs."""
    tpl = _template("peaked")
    kinds = [("sampling greedy", SAMPLE), ("samples K=3", K3), ("samples K=1 T=0.7", K1_T), ("samples K=3 T=0.8 k=20 p=0.9", K3_FILT)]
    calls = [_call("greedy", (3, 6, 101), GREEDY)] * 3
    for rnd in range(3):
        calls += [_call(what, (3, 6, 102 + rnd), kw) for what, kw in kinds]
    calls.append(_call("greedy", (3, 6, 105), GREEDY))
    used, outs = _walk("A", tpl, calls)
    assert _differ(outs[4], outs[8], ("ids", "values")) and _differ(outs[3], outs[7], ("ids", "values"))      # other rounds, other draws
    plans = {"greedy": _ws(used, 3, 6), "K=3": _ws(used, 3, 6, 3, True), "K=1": _ws(used, 3, 6, 1, True)}
    assert set(plans["greedy"]["plans"]) == greedy_plan_keys(6)
    assert set(plans["K=3"]["plans"]) == sample_plan_keys(6) | sample_plan_keys(6, 0.8, 20, 0.9)
    assert set(plans["K=1"]["plans"]) == sample_plan_keys(6, 0.7)
    assert plans["greedy"]["calls"] == 7 and plans["K=3"]["calls"] == 6 and plans["K=1"]["calls"] == 3
    report("A", calls=COUNTS["A"], plan_keys={k: _plan_keys(w) for k, w in plans.items()})


# =====================================================================================================================================
# B. beam options across replays
# =====================================================================================================================================
def test_b_beam_options_across_replays():
    """One search_beam_size = 3 decoder whose attributes change between calls the way decode_img2txt sets them.  Each variant is called
    until it has replayed (three calls the first time the workspace is met, two afterwards; host blocking and the variants that share the
    unblocked keys are called twice all the same), on two input sets in turn; the unblocked search comes back last.  Before anything is
    compared the FRESH results on the first input set must show that the options matter: min_len, either blocking, the ignore list and the
    other eos each change the frames."""
    tpl = _template("peaked")
    A, Bc = (3, 6, 473), (3, 6, 471)
    frames = ("scores", "wids", "ptrs")

    def fresh(what, **attrs):
        return _run(_new(tpl), _call(what, A, GREEDY, search_beam_size=3, **attrs), 4600)
    free = fresh("beam")
    ign, eos2 = int(free["pred_seq"][0, 0]), int(free["pred_seq"][0, 2])
    assert ign not in (0, EOS) and eos2 not in (0, EOS), free["pred_seq"]
    ng = dict(forbid_duplicate_ngrams=True)
    variants = [("beam", {}), ("beam min_len=3", dict(min_len=3)), ("beam ngram 2", dict(ng, ngram_size=2)),
                ("beam ngram 2 ignoring %d" % ign, dict(ng, ngram_size=2, forbid_ignore_set={ign})), ("beam ngram 3", dict(ng, ngram_size=3)),
                ("beam ngram 3 on the host", dict(ng, ngram_size=3, ngram_blocking="host")), ("beam eos_id=%d" % eos2, dict(eos_id=eos2)),
                ("beam n_best=3", dict(n_best=3)), ("beam backtrack=device", dict(backtrack="device"))]
    f = collections.OrderedDict((what, fresh(what, **attrs)) for what, attrs in variants)
    assert (f["beam"]["wids"][:, :3] == EOS).any(), "no hypothesis of the unblocked search meets eos in the frames min_len = 3 blocks"
    ign_name, eos_name = variants[3][0], variants[6][0]
    for a, b in (("beam min_len=3", "beam"), ("beam ngram 2", "beam"), (ign_name, "beam ngram 2"), ("beam ngram 3", "beam"),
                 ("beam ngram 3", "beam ngram 2"), (eos_name, "beam")):
        assert _differ(f[a], f[b], frames), "the searches %r and %r do not differ on these inputs: comparing them shows nothing" % (a, b)
    assert first_difference(f["beam ngram 3 on the host"], f["beam ngram 3"]) is None
    for k in frames:
        assert bit_diff(f["beam n_best=3"][k], f["beam"][k]) == 0 and bit_diff(f["beam backtrack=device"][k], f["beam"][k]) == 0
    assert bit_diff(f["beam backtrack=device"]["pred_seq"], f["beam"]["pred_seq"]) == 0        # device rank 0 is the host's hypothesis
    assert tuple(f["beam n_best=3"]["nbest_seq"].shape) == (3, 3, NV + 2 + 6)

    used = _new(tpl)
    calls, expected, met = [], set(), 0
    for what, attrs in variants:
        attrs = dict(attrs, search_beam_size=3)
        for j in range(calls_until_replayed(met)):
            calls.append(_call(what, (A, Bc)[j % 2], GREEDY, **attrs))
            met += 1
        expected |= beam_plan_keys(6, attrs_of(calls[-1], EOS))
    calls.append(_call("beam", A, GREEDY, search_beam_size=3))
    _, outs = _walk("B", tpl, calls, used=used)
    for k in frames + ("pred_seq",):                           # the unblocked search, last, on the inputs of its first call
        assert bit_diff(outs[-1][k], outs[0][k]) == 0, k
    ws = _ws(used, 3, 6, 3)
    assert set(ws["plans"]) == expected, (sorted(map(str, set(ws["plans"]) ^ expected)))
    assert set(ws["ngram_ignore"]) == {(ign,)} and set(ws["nbest"]) == {1, 3} and ws["calls"] == len(calls)
    assert len(expected) == 5 + 2 + 3 * 5 + 5                  # unblocked, min_len's two blocked frames, three device blockings, the other eos
    report("B", calls=COUNTS["B"], plan_keys=_plan_keys(ws), ignore_id=ign, other_eos_id=eos2)


# =====================================================================================================================================
# C. leave a workspace key and come back
# =====================================================================================================================================
@pytest.mark.parametrize("kind", ["greedy", "samples K=3"])
def test_c_leave_a_workspace_key_and_come_back(kind):
    """(B = 3, T = 6) to replay, (B = 2, T = 4) to replay, (B = 3, T = 6) again with new inputs, beam 2 at (B = 3, T = 6), and the first kind
    once more: the graphs of a key must survive the other keys' calls, and follow new inputs when the key returns."""
    tpl = _template("peaked")
    kw = GREEDY if kind == "greedy" else K3
    cases = [(3, 6, 301), (3, 6, 302), (3, 6, 303), (2, 4, 304), (2, 4, 305), (2, 4, 306), (3, 6, 307)]
    calls = [_call(kind, c, kw) for c in cases] + [_call("beam 2", (3, 6, 308), GREEDY, search_beam_size=2), _call(kind, (3, 6, 309), kw)]
    used, outs = _walk("C/" + kind, tpl, calls)
    grp = (3, True) if kind != "greedy" else (1, False)
    big, small = _ws(used, 3, 6, *grp), _ws(used, 2, 4, *grp)
    keys = greedy_plan_keys if kind == "greedy" else sample_plan_keys
    assert set(big["plans"]) == keys(6) and set(small["plans"]) == keys(4) and (big["calls"], small["calls"]) == (5, 3)
    assert _ws(used, 3, 6, 2)["calls"] == 1 and not _ws(used, 3, 6, 2)["plans"]
    assert _differ(outs[2], outs[6], ("values",))
    report("C/" + kind, calls=COUNTS["C/" + kind], plan_keys={"B=3 T=6": _plan_keys(big), "B=2 T=4": _plan_keys(small)})


# =====================================================================================================================================
# D. parameters that move
# =====================================================================================================================================
D_CASE = (3, 6, 461)


def _oracle_greedy(pd, inp):
    """oracle.greedy_decode in fp32 on the weights `pd`, with the top-1 / top-2 margin of every position (the lm_head spy of
    test_40::test_greedy_decode_vs_oracle_ragged_mask)."""
    top2 = []
    orig = O.lm_head

    def spy(pp, x):
        out = orig(pp, x)
        top2.append(torch.topk(out[:, -1, :], 2, dim=-1).values)
        return out
    O.lm_head = spy
    try:
        with torch.no_grad():
            oids, ovals = O.greedy_decode(pd, inp[0].float(), inp[1].float(), *inp[2:], S.MASK_ID, len_vis_input=NV)
    finally:
        O.lm_head = orig
    t2 = torch.stack(top2, dim=1)
    return oids.cpu(), ovals.cpu(), (t2[..., 0] - t2[..., 1]).cpu()


def _anchor(model, got, tag):
    """test_40's rule for the greedy decode `got` of `model` against the oracle on the model's current (fp16) weights evaluated in fp32."""
    B, T, _ = D_CASE
    pd = {k: v.float() for k, v in model.state_dict().items()}
    oids, ovals, margin = _oracle_greedy(pd, _inputs(*D_CASE))
    share = margin_share(margin, MARGIN_TOL)
    assert share <= 0.2, "%s: %.3f of the oracle's positions have a margin under %g: these inputs compare too little" % (tag, share, MARGIN_TOL)
    compared, flips = compare_decodes(got["ids"].cpu(), got["values"].cpu(), oids, ovals, margin)
    assert compared >= 0.8 * B * T, (tag, compared, flips)
    return dict(share_under_margin_tol=share, compared=compared, of=B * T, flips=flips, smallest_margin=float(margin.min()),
                margin_tol=MARGIN_TOL, score_tol=SCORE_TOL)


@pytest.mark.parametrize("pipelined", ["0", "1"], ids=["plain", "pipelined"])
def test_d_parameters_that_move(pipelined, monkeypatch):
    """A decoder in train() under FP16_Optimizer_State(FusedAdam) (test_86's): greedy and K = 3 decodes taken to replay under no_grad; three
    rounds of one SCST-style step (sampled K = 3 forward with gradients, policy_loss against a fixed reward, backward, step, zero_grad) and the
    two decodes again -- the replayed graphs read the parameters by address, and under the pipelined step the update runs on another stream
    --; the oracle anchor on the updated weights; load_state_dict of the original weights (the very first results come back); half() / to(),
    which invalidates and repacks."""
    monkeypatch.setenv("VLP_ADAM_PIPELINE", pipelined)
    tag = "D/" + ("pipelined" if pipelined == "1" else "plain")
    tpl = _template("flat", True)
    used = _new(tpl)
    opt = _optimizer(used)
    assert used.training and opt.pipeline_with_forward == (pipelined == "1")
    sd0 = used.state_dict()
    two = [_call("greedy", D_CASE, GREEDY), _call("samples K=3", D_CASE, K3)]
    inp = _inputs(*D_CASE)
    first, i, greedy_after = {}, 0, None
    for rep in range(3):                                         # 1. plain, capture, replay
        for c in two:
            got, _ = _used_vs_fresh(tag, i, c, used, tpl)
            if rep == 0:
                first[c.what] = (4600 + 37 * i, snapshot(got))
            greedy_after = got if c.what == "greedy" else greedy_after
            i += 1
    anchors = {"initial weights": _anchor(used, greedy_after, tag + ", initial weights")}
    B, T, _ = D_CASE
    reward = (torch.linspace(-1.0, 1.0, 3 * B * T, device=DEV) + 0.25).view(3 * B, T)
    assert bool(reward.ne(0).all())
    for rnd in range(3):                                         # 2. the parameters move between the decodes
        before = {k: t.clone() for k, t in used.engine.flat.items()}
        used.engine.step_seed = 900 + rnd
        ids, logp = used(*inp, task_idx=None, sample_mode="sample", n_samples=3)
        assert logp.requires_grad and tuple(ids.shape) == (3 * B, T)
        loss, _ = SC.policy_loss(logp, SC.clean_captions(ids, EOS), reward)
        opt.backward(loss)
        opt.step()
        opt.zero_grad()
        greedy_after = None
        for c in two:                                            # (first: through the engine's own wait for the parameters)
            got, _ = _used_vs_fresh(tag, i, c, used, tpl)
            greedy_after = got if c.what == "greedy" else greedy_after
            i += 1
        moved = {k: bit_diff(before[k], t) for k, t in used.engine.flat.items()}
        assert all(n > 0 for n in moved.values()), "round %d: the optimizer step changed no parameter (%r)" % (rnd, moved)
        assert opt.skipped_steps == 0, "round %d: the step was skipped for an overflow" % rnd
    anchors["updated weights"] = _anchor(used, greedy_after, tag + ", updated weights")
    assert first_difference(greedy_after, first["greedy"][1]) is not None       # three updates move at least the scores
    used.load_state_dict(sd0)                                    # 3. the original weights, in place under the graphs
    for c in two:
        seed, want = first[c.what]
        got, _ = _used_vs_fresh(tag + ", original weights loaded", i, c, used, tpl, seed=seed)
        d = first_difference(got, want)
        assert d is None, "%s, call %d (%s): after load_state_dict of the original weights the first result does not come back -- %s" % (tag, i, c.what, d)
        i += 1
    old = used.engine._ws                                        # 4. new parameter storage: everything captured is void
    old_ws = _ws(used, B, T)
    assert old_ws["plans"] and old_ws["calls"] > 3
    used.half()
    used.to(DEV)
    assert not used.engine.packed and used.engine._ws == {} and used.engine._ws is not old
    for c in two:
        seed, want = first[c.what]
        got, _ = _used_vs_fresh(tag + ", after half() / to()", i, c, used, tpl, seed=seed)
        d = first_difference(got, want)
        assert d is None, "%s, call %d (%s): after half() / to() -- %s" % (tag, i, c.what, d)
        i += 1
    new_ws = _ws(used, B, T)
    assert new_ws is not old_ws and new_ws["calls"] == 1 and not new_ws["plans"] and used.engine.packed
    report(tag, calls=COUNTS[tag] + COUNTS[tag + ", original weights loaded"] + COUNTS[tag + ", after half() / to()"], optimizer_steps=3,
           oracle_anchor=anchors)


# =====================================================================================================================================
# E. another stream
# =====================================================================================================================================
def test_e_another_stream():
    """Greedy and beam 3 taken to replay on the default stream, the same calls inside torch.cuda.stream(side), then on the default stream once
    more.  The plans of a workspace belong to one stream (a recorded launch plan carries the stream in its arguments): on the side stream
    EVERY step must be planned anew -- none of the default stream's plan objects may be replayed there --, and the default stream finds its
    own plans again when it returns."""
    tpl = _template("peaked")
    used = _new(tpl)

    def pair(seed):
        return [_call("greedy", (3, 6, seed), GREEDY), _call("beam", (3, 6, seed + 1), GREEDY, search_beam_size=3)]
    first, on_side, back = pair(501) + pair(503) + pair(505), pair(507) + pair(509), pair(511) + pair(513)
    for c in first + on_side + back:                             # (every input is resident before any stream is switched)
        _inputs(*c.case)
    _walk("E", tpl, first, used=used)
    wss = (_ws(used, 3, 6), _ws(used, 3, 6, 3))
    keys = (greedy_plan_keys(6), beam_plan_keys(6, attrs_of(first[1], EOS)))
    main = torch.cuda.current_stream()
    on_main = [dict(ws["plans"]) for ws in wss]
    assert all(ws["plan_stream"] == main.cuda_stream and set(ws["plans"]) == k for ws, k in zip(wss, keys))
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(main)
    with torch.cuda.stream(side):
        _walk("E/side stream", tpl, on_side, used=used, start=6)
    main.wait_stream(side)
    for ws, k, old in zip(wss, keys, on_main):                   # EVERY step was planned again for the side stream, not only the first one
        assert ws["plan_stream"] == side.cuda_stream and set(ws["plans"]) == k
        stale = [str(key) for key in k if ws["plans"][key] is old[key]]
        assert not stale, "plans made on the default stream were replayed on the side stream: %s" % stale
    _walk("E/default stream again", tpl, back, used=used, start=10)
    for ws, k, old in zip(wss, keys, on_main):                   # and the default stream has its own back
        assert ws["plan_stream"] == main.cuda_stream and set(ws["plans"]) == k and all(ws["plans"][key] is old[key] for key in k)
    report("E", calls=COUNTS["E"] + COUNTS["E/side stream"] + COUNTS["E/default stream again"])


# =====================================================================================================================================
# F. results belong to the caller
# =====================================================================================================================================
F_KINDS = [("greedy", GREEDY, {}), ("sampling greedy", SAMPLE, {}), ("samples K=1 T=0.7", K1_T, {}), ("samples K=1 top_k=5", K1_TOPK, {}),
           ("samples K=3", K3, {}), ("beam", GREEDY, dict(search_beam_size=3)), ("beam n_best=3", GREEDY, dict(search_beam_size=3, n_best=3)),
           ("beam backtrack=device", GREEDY, dict(search_beam_size=3, backtrack="device"))]


@pytest.mark.parametrize("what,kw,attrs", F_KINDS, ids=[k[0] for k in F_KINDS])
def test_f_results_belong_to_the_caller(what, kw, attrs):
    """The first call's results are HELD, not cloned (a cloned snapshot lies beside them); a second call at the same workspace key with other
    inputs and another seed must differ from them and must leave them as they were.  The filter records are the workspace's by design
    and are not held."""
    used = _new(_template("peaked"))
    held = _run(used, _call(what, (3, 6, 601), kw, **attrs), 4601)
    held = collections.OrderedDict((k, v) for k, v in held.items() if torch.is_tensor(v) and not k.startswith("filter_"))
    kept = snapshot(held)
    n_ws = len(used.engine._ws)
    second = _run(used, _call(what, (3, 6, 602), kw, **attrs), 4777)
    assert len(used.engine._ws) == n_ws                                          # the same workspace key
    differing = [k for k in held if bit_diff(second[k], kept[k]) != 0]
    # what must differ: the scores of a search or of an argmax; of a draw also the ids (18 draws among seven likely words)
    main_keys = ("scores",) if "scores" in held else ("values",) if what == "greedy" else ("ids", "values")
    assert all(k in differing for k in main_keys), "scenario F (%s): the second call returned the first call's %s" % (what, main_keys)
    d = first_difference(held, kept)
    assert d is None, "scenario F (%s): a result the caller still held was overwritten by the next call -- %s" % (what, d)
    COUNTS["F"] += 2
    report("F/" + what, calls=2, held=sorted(held), differing_in_the_second_call=differing)
