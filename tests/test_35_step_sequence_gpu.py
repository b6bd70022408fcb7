"""GPU: a USED engine must equal a FRESH one.

Every other model-level test builds a model, runs one step (or identical ones) and drops it.  Training drives one Engine through
thousands of steps whose kind, shape and packing change, and the engine carries state between them: workspaces keyed (B, L, P) and
reused for life, gradient buffers that zero_grad() does not clear, the W^T shadows, stream events, the packing caches.  Here a `used`
model lives through a scenario; after each of its steps a `fresh` model of the same configuration receives the used model's
parameters (bit for bit, asserted), the same varlen setting and step_seed, and runs only that step.  The step is bit-reproducible by
design (no atomics, committed tuning table), so losses, logits, pooled output, last_packed_rows and EVERY param.grad -- the parameters
the step does not reach included -- must be equal BIT FOR BIT; with an optimizer in the loop so must parameters, fp32 masters, both
Adam moments and the loss-scale state after the update.  A fresh engine's single step is what test_10 / test_15 / test_20 / test_25
tie to the fp32 oracle.  Only two comparisons use bounds: C's accumulated gradients (derived ulp count, step_seq_util.
accumulation_excess) and E's packed-against-dense gradients (test_25's 2e-4 rel-L2).  Skipped under VLP_AUTOTUNE=1 (timed kernel
choices are not reproducible and not the product configuration).

Scenarios: A kinds alternate on one workspace key; B shapes walk and return (both grouped-wgrad thresholds, L = 192, L = 256, and one
length tuple at two L); C accumulation across kinds and what it leaves behind; D optimizer in the loop (FusedAdam plain / pipelined,
BertAdam); E packing caches under 70 distinct length tuples; F other forwards (eval, score_samples, sampling decoder, answer()) in
between.  Label smoothing is an attribute of the model that Engine.mlm_loss reads per call, so A's step 6 switches it per call.

What the scenarios found: Engine.backward cleared `_pooler_dirty` after EVERY backward without the pretext branch, also an accumulating
one that had not zeroed the buffer -- after (pretext, MLM accumulated, zero_grad, MLM) bert.pooler.dense.{weight,bias}.grad still held
the pretext gradient and entered the gradient norm (test_c, pair 0, "plain step after the pair").  Fixed in the engine: the flag now
means "the buffer holds something a beta == 0 backward must clear".

MUTATIONS (each made in a scratch copy of vlp_amd/engine.py, never committed; what this module reports, first failing test and tensor):
  1. drop `ws["dctx"][:M].zero_()` from the live prologue: test_a[dense] fails at step 2 (the MLM step after the pretext step, whose full
     path filled dctx) -- grad bert.embeddings.word_embeddings.weight, 34851 of 786432 elements differ.
  2. drop `dense.zero_()` in front of rows_unpack: test_a[packed] fails at step 1 (pretext) -- grad bert.embeddings.word_embeddings.weight,
     725 of 786432 elements (ws["dx_alt"] is also the scratch of the dense steps; its dropped rows were never written as zeros).
  3. `_refresh_shadows` returns early once the shadows exist: test_d_fused_adam_in_the_loop[plain] fails at step 3, the step after the
     first applied update (two skipped at 2^24 and 2^20) -- grad vis_embed.0.weight, 186312 of 4194304 elements (dgrad through a stale v2T).
  4. the old line `self._pooler_dirty = pt is not None` behind the fixed block: test_c fails in pair 0 (pretext, mlm) at the plain step after
     the pair -- grad bert.pooler.dense.weight, 538368 of 589824 elements: the pretext gradient survived zero_grad().
  5. `_pk_cache` keyed without L: test_b fails at step 6 (the B = 4 batch inside L = 131 after the same length tuple at L = 123: the
     cached row_map of L = 123 stays inside [0, 4 x 131), so the run is wrong, not out of bounds) -- loss[0], 1 of 1 elements.
  With the engine as committed the module passes.
"""
import collections
import copy
import functools
import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from oracle import vlp_oracle as O                                      # noqa: E402
from vlp_amd import synthetic as S                                      # noqa: E402
from vlp_amd import tuning                                              # noqa: E402
from vlp_amd.engine import VlpPerformanceWarning                        # noqa: E402
from vlp_amd.input_prep import MaskSpec, SparseAnswers                  # noqa: E402
from vlp_amd.loss import LabelSmoothingLoss                             # noqa: E402
from vlp_amd.modeling import BertConfig, BertForPreTrainingLossMask     # noqa: E402
from vlp_amd.optimization import BertAdam                               # noqa: E402
from vlp_amd.optimization_fp16 import FP16_Optimizer_State, FusedAdam   # noqa: E402
from tests.step_seq_util import accumulation_excess, bit_diff, first_difference   # noqa: E402

if tuning.AUTOTUNE:
    pytest.skip("VLP_AUTOTUNE=1: timed kernel choices are not bit-reproducible", allow_module_level=True)

DEV = torch.device("cuda:0")
V = 1024
ND = ["bias", "LayerNorm.bias", "LayerNorm.weight"]
SCALE = 1024.0          # upstream gradient of the img2txt losses (test_25's loss scale); the VQA loss (BCE x 3129, ~2000) takes 1.0

# kind: mlm | pretext (mask_image_regions) | empty (empty masked_pos, pretext loss only) | smooth (label-smoothed MLM) | vqa | logprob
# (score_samples + log-probability backward) | eval (eval() + no_grad forward) | decode (sampling decoder) | answer (model.answer)
Step = collections.namedtuple("Step", ["kind", "batch", "varlen", "zero"])
Step.__new__.__defaults__ = (False, True)
NO_BACKWARD = ("eval", "decode", "answer")


@functools.lru_cache(maxsize=None)
def _template(tasks, layers, Nv=100):
    """One model per configuration, built once and never run: every used / fresh model is a deepcopy (a new Engine each)."""
    p = O.init_params(vocab_size=V, layers=layers, tasks=tasks, seed=35)
    cfg = BertConfig(V, num_hidden_layers=layers, type_vocab_size=6, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1)
    m = BertForPreTrainingLossMask(cfg, enable_butd=True, len_vis_input=Nv, tasks=tasks, allow_random_fc7=True)
    sd = dict(p)
    sd["cls.predictions.decoder.weight"] = p["bert.embeddings.word_embeddings.weight"]
    m.load_state_dict(sd, strict=True)
    return m.half().to(DEV).train()


@functools.lru_cache(maxsize=None)
def _smooth_crit():
    return LabelSmoothingLoss(0.1, V, ignore_index=0, reduction="none").half().to(DEV)


def _new(template, varlen=False):
    m = copy.deepcopy(template)
    m.engine.pack()
    m.engine.varlen = varlen
    return m


def _fresh_from(template, used, what):
    """A fresh model holding `used`'s current parameters: the flat buffers are copied (fp16 -> fp16, no arithmetic)."""
    m = _new(template)
    for k, t in used.engine.flat.items():
        m.engine.flat[k].copy_(t)
    for (n, a), (_, b) in zip(m.named_parameters(), used.named_parameters()):
        assert bit_diff(a.data, b.data) == 0, "%s: parameter %s of the fresh model differs from the used model's" % (what, n)
    return m


def _raw(B, max_len_b, seed, Nv=100, tasks="img2txt", min_len_b=6, pad_to=None):
    raw = S.make_batch(B, max_len_b=max_len_b, len_vis_input=Nv, vocab_size=V, max_pred=3 if tasks != "vqa2" else 1, s2s_prob=0.75, tasks=tasks,
                       seed=seed, vis_mask_prob=0.25, min_len_b=min_len_b)
    if pad_to is not None:           # the same samples in a longer sequence: ids, segments and mask padded with zeros
        L = raw.input_ids.shape[1]
        e = pad_to - L
        assert e > 0
        pad = torch.nn.functional.pad
        raw = raw._replace(input_ids=pad(raw.input_ids, (0, e)), segment_ids=pad(raw.segment_ids, (0, e)), input_mask=pad(raw.input_mask, (0, e, 0, e)))
    return raw


def _kept(raw):
    """Kept length of every sample: 1 + the last key column any query attends (test_25's expectation of last_packed_rows)."""
    return [int(m.any(dim=0).nonzero().max()) + 1 for m in raw.input_mask]


def _batch(*a, **k):
    return S.batch_to(_raw(*a, **k), DEV, half=True)


def _emptied(b):
    return b._replace(masked_pos=b.masked_pos[:, :0].contiguous(), lm_label_ids=b.lm_label_ids[:, :0].contiguous(),
                      masked_weights=b.masked_weights[:, :0].contiguous())


def _decoder_inputs(B, max_len_b, seed, Nv=100):
    """(img, vis_pe, prefix ids, segment ids, position ids, mask, sampled ids) of a scoring / decoding call, explicit position ids (+2)."""
    raw = S.make_batch(B, max_len_b=max_len_b, len_vis_input=Nv, vocab_size=V, max_pred=0, mask_prob=0.0, seed=seed, min_len_b=4)
    L = raw.input_ids.shape[1]
    pos = torch.arange(L).unsqueeze(0).expand(B, L).contiguous() + 2
    sample = torch.randint(1, V, (B, L - (Nv + 2)), generator=torch.Generator().manual_seed(seed + 7))
    t = (raw.img.half(), raw.vis_pe.half(), raw.input_ids[:, :Nv + 2].contiguous(), raw.segment_ids, pos, raw.input_mask, sample)
    return tuple(x.to(DEV) for x in t)


def _call(model, b, mir):
    return model(b.img, b.vis_pe, b.input_ids, b.segment_ids, b.input_mask, b.lm_label_ids, b.ans_labels, b.is_next, masked_pos=b.masked_pos,
                 masked_weights=b.masked_weights, task_idx=b.task_idx, vis_masked_pos=b.vis_masked_pos, mask_image_regions=mir, drop_worst_ratio=0)


def _run(model, step, seed, opt=None, scale=SCALE):
    """One step of `model`; returns everything the step left behind as an ordered {name: tensor | value}."""
    eng = model.engine
    kind, b = step.kind, step.batch
    eng.varlen = step.varlen
    if step.zero and kind not in NO_BACKWARD:
        (opt if opt is not None else eng).zero_grad()
    eng.step_seed = seed
    _SNAP["eng"], _SNAP["word"] = eng, None
    out = collections.OrderedDict()
    if kind == "logprob":
        st, logp = eng.score_samples(*b, S.MASK_ID)
        out["logp"], out["logits"] = logp.clone(), eng.mlm_logits(st).clone()
        out["last_packed_rows"] = eng.last_packed_rows
        eng.backward(st, None, "logprob", g_rows=torch.full((logp.numel(),), -scale / logp.numel(), device=DEV, dtype=torch.float32))
    elif kind == "decode":
        with torch.no_grad():
            ids, lp = eng.decode_greedy(*b[:6], S.MASK_ID, sample=True)
        out["ids"], out["logp"] = ids.clone(), lp.clone()
    elif kind == "answer":
        ids, val, _ = model.answer(b.img, b.vis_pe, b.input_ids, b.segment_ids, b.input_mask)
        out["ids"], out["logit"], out["logits"] = ids.clone(), val.clone(), model.last_vqa_logits.clone()
        out["last_packed_rows"] = eng.last_packed_rows
    else:
        mir = kind in ("pretext", "empty")
        model.crit_mask_lm_smoothed = _smooth_crit() if kind == "smooth" else None      # read by Engine.mlm_loss on every call
        if kind == "eval":
            model.eval()
            with torch.no_grad():
                lt = _call(model, b, False)
            model.train()
        else:
            lt = _call(model, b, mir)
        for i, x in enumerate(lt):
            out["loss[%d]" % i] = x.detach().clone()
        if kind == "vqa":
            out["logits"] = model.last_vqa_logits.clone()
        elif kind != "empty":
            out["logits"] = model.last_mlm_logits.clone()
        if mir:
            out["pooled"] = model.last_pooled_output.clone()
        out["last_packed_rows"] = eng.last_packed_rows
        if kind != "eval":
            total = lt[0] + lt[1] + lt[2]
            if isinstance(opt, FP16_Optimizer_State):
                opt.backward(total)
            else:
                (total * scale).backward()
    if kind not in NO_BACKWARD:
        out["last_live_rows"] = eng.last_live_rows
        for n, q in model.named_parameters():
            out["grad " + n] = q.grad.detach().clone()
        if _SNAP["on"]:
            out[PRE_SCATTER] = _SNAP["word"]
    return out


def _same(scenario, i, kind, got, want, keys=None):
    if keys is not None:
        got, want = collections.OrderedDict((k, got[k]) for k in keys(got)), collections.OrderedDict((k, want[k]) for k in keys(want))
    d = first_difference(got, want)
    assert d is None, "scenario %s, step %d (%s): the used engine differs from a fresh one -- %s" % (scenario, i, kind, d)


def _not_grads(d):
    return [k for k in d if not k.startswith("grad ")]


def _used_vs_fresh(scenario, i, step, used, template, scale=SCALE):
    """The step on `used`, then alone on a fresh engine with used's parameters; everything bit-equal."""
    seed = 1000 + 17 * i
    got = _run(used, step, seed, scale=scale)
    fresh = _fresh_from(template, used, "scenario %s, step %d (%s)" % (scenario, i, step.kind))
    want = _run(fresh, step._replace(zero=True), seed, scale=scale)
    _same(scenario, i, step.kind, got, want, keys=None if step.zero else _not_grads)
    return got, want


def _walk(scenario, template, steps, scale=SCALE, used=None):
    used = used if used is not None else _new(template)
    outs = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", VlpPerformanceWarning)      # (fresh dense masks on a packed engine: what scenario E is about)
        for i, step in enumerate(steps):
            outs.append(_used_vs_fresh(scenario, i, step, used, template, scale)[0])
    return used, outs


# =====================================================================================================================================
# A. kinds alternate on one workspace key
# =====================================================================================================================================
@pytest.mark.parametrize("packed", [False, True], ids=["dense", "packed"])
def test_a_kinds_alternate_on_one_workspace_key(packed):
    """B = 4, L = 123, 3 layers: MLM (listed-row last layer), pretext, MLM, empty masked_pos, MLM, label-smoothed MLM, MLM on another batch
    -- zero_grad() in front of every step.  The live path must find dctx / dpre1 cleared after a full-path step filled them; the packed
    steps touch only the first M' rows of buffers the previous step wrote with other lengths."""
    tpl = _template("img2txt", 3)
    b1, b2 = _batch(4, 20, 101), _batch(4, 20, 102)
    plan = [("mlm", b1), ("pretext", b1), ("mlm", b1), ("empty", _emptied(b1)), ("mlm", b1), ("smooth", b1), ("mlm", b2)]
    used, outs = _walk("A/" + ("packed" if packed else "dense"), tpl, [Step(k, b, packed) for k, b in plan])
    for (kind, _), o in zip(plan, outs):
        assert (o["last_live_rows"] is not None) == (kind in ("mlm", "smooth")), (kind, o["last_live_rows"])
        assert (o["last_packed_rows"] is not None) == packed
    assert 0 < outs[0]["last_live_rows"] <= 12


# =====================================================================================================================================
# B. shapes walk and return
# =====================================================================================================================================
def test_b_shapes_walk_and_return():
    """One packed engine, 2 layers: B = 4 / L = 123; B = 21 (M' >= 2048 and Mv = 2100: grouped layer and region wgrads, the other stream
    join); B = 3 / L = 192 (key-tile boundary); B = 2 / L = 256 (kept dense); B = 4 and B = 21 again with new contents; then the B = 4 batch
    once more inside L = 131 -- the same kept-length tuple at another L, which _pk_cache must not confuse."""
    tpl = _template("img2txt", 2)
    shapes = [dict(B=4, max_len_b=20, seed=201), dict(B=21, max_len_b=20, seed=202), dict(B=3, max_len_b=89, seed=203),
              dict(B=2, max_len_b=153, seed=204, min_len_b=100), dict(B=4, max_len_b=20, seed=205), dict(B=21, max_len_b=20, seed=206),
              dict(B=4, max_len_b=20, seed=205, pad_to=131)]
    raws = [_raw(**s) for s in shapes]
    assert [r.input_ids.shape[1] for r in raws] == [123, 123, 192, 256, 123, 123, 131] and _kept(raws[4]) == _kept(raws[6])
    used, outs = _walk("B", tpl, [Step("mlm", S.batch_to(r, DEV, half=True), True) for r in raws])
    for r, o in zip(raws, outs):
        L = r.input_ids.shape[1]
        assert o["last_packed_rows"] == (sum(_kept(r)) if L <= 192 else None)
    assert outs[1]["last_packed_rows"] >= 2048 and outs[5]["last_packed_rows"] >= 2048 and outs[0]["last_packed_rows"] < 2048


# =====================================================================================================================================
# C. accumulation across kinds, and what it leaves behind
# =====================================================================================================================================
WORD = "bert.embeddings.word_embeddings.weight"
PRE_SCATTER = "grad (word table before the embedding scatter)"
_SNAP = {"on": False, "eng": None, "word": None}


def _snapshot_word_table(monkeypatch):
    """The word-embedding gradient is the one tensor two accumulating launches write per backward: the tied-decoder wgrad (vlp_gemm_tn,
    beta) and the embedding scatter (embed_word_reduce_kernel, +=).  Its first rounding happens at the magnitude of the value BETWEEN
    the two, so _run records that value: a clone taken where the table kernels are issued (same stream, behind the head wgrad)."""
    from vlp_amd import _lib as K

    def wrap(fn):
        def call(*a, **k):
            if _SNAP["on"] and k.get("parts") == 2:
                _SNAP["word"] = _SNAP["eng"].G(WORD).clone()
            return fn(*a, **k)
        return call
    monkeypatch.setattr(K, "embed_bwd", wrap(K.embed_bwd))
    monkeypatch.setattr(K, "embed_bwd_pos", wrap(K.embed_bwd_pos))
    monkeypatch.setitem(_SNAP, "on", True)


def test_c_accumulation_across_kinds_and_what_it_leaves_behind(monkeypatch):
    """Pairs of steps accumulated without zero_grad between them: (pretext, MLM) -- the pooler sequence --, (MLM, empty masked_pos),
    (packed MLM, dense MLM of another length), (MLM, score_samples + log-probability backward).  The forward of every step and the first
    step's gradients are bit-equal to fresh; the accumulated gradient meets g1 + g2 (fp32 sum of the two fresh single-step gradients)
    within the derived ulp count; zero_grad() + a plain MLM step after each pair is bit-equal to fresh again.

    Roundings per backward, counted in Engine.backward and the kernels: ONE for every tensor but the word table -- a weight and its bias
    by one vlp_gemm_tn / grouped launch (bias_out fused) or its split-M reduce (gemm_tn.hip: `(f16)(beta ? (float)o + v : v)`); the
    LayerNorm sums by one partial-row reduce, deferred or not (layernorm.hip reduce_partial_rows); the position / type tables by one +=
    kernel each (elementwise.hip); vis_pe_embed.0.weight by copy2d(beta) of an fp16 GEMM result, which IS g2, and its bias by colsum's
    reduce.  Bound: ulp(acc) / 2 + ulp(g2) / 2, i.e. at most the 1 ulp at max(|acc|, |g2|).  TWO for the word table (_snapshot_word_table):
    with t, u the table between the two launches in the accumulating and in the fresh second step, ulp(t) / 2 + ulp(acc) / 2 +
    ulp(u) / 2 + ulp(g2) / 2 -- 2 ulps, each half taken where its rounding happens (62 elements whose two contributions cancel miss
    "2 ulps at max(|acc|, |g2|)" by up to 8x: the roundings happened at the larger intermediate)."""
    _snapshot_word_table(monkeypatch)
    tpl = _template("img2txt", 3)
    b1, b3 = _batch(4, 20, 301), _batch(4, 30, 303)
    dec = _decoder_inputs(4, 8, 304)
    pairs = [(Step("pretext", b1), Step("mlm", b1)), (Step("mlm", b1), Step("empty", _emptied(b1))),
             (Step("mlm", b1, True), Step("mlm", b3, False)), (Step("mlm", b1), Step("logprob", dec))]
    used = _new(tpl)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", VlpPerformanceWarning)
        for k, (s1, s2) in enumerate(pairs):
            tag = "C/pair %d (%s, %s)" % (k, s1.kind, s2.kind)
            _, w1 = _used_vs_fresh(tag, 0, s1, used, tpl)
            g2, w2 = _used_vs_fresh(tag, 1, s2._replace(zero=False), used, tpl)
            worst = ("", 0.0)
            for key in g2:
                if not key.startswith("grad ") or key == PRE_SCATTER:
                    continue
                rounded = (g2[key], w2[key]) + ((g2[PRE_SCATTER], w2[PRE_SCATTER]) if key == "grad " + WORD else ())
                ratio, bad = accumulation_excess(g2[key], w1[key], w2[key], rounded)
                if ratio > worst[1]:
                    worst = (key, ratio)
                assert bad == 0, ("scenario %s: accumulated %s differs from g1 + g2 by more than its %d half ulps in %d of %d elements (worst %.3f x the bound)"
                                  % (tag, key, len(rounded), bad, g2[key].numel(), ratio))
            print("%s: worst accumulated tensor %s at %.3f of its bound" % (tag, worst[0], worst[1]))
            _used_vs_fresh(tag + ", plain step after the pair", 2, Step("mlm", b1), used, tpl)


# =====================================================================================================================================
# D. optimizer in the loop
# =====================================================================================================================================
def _groups(model):
    named = list(model.named_parameters())
    return [{"params": [q for n, q in named if not any(x in n for x in ND)], "weight_decay": 0.01},
            {"params": [q for n, q in named if any(x in n for x in ND)], "weight_decay": 0.0}]


def _fused_adam(model):
    # scale_factor 16 (the start, 2^24, and the eight steps are given): a backward of this model overflows fp16 down to a scale of about
    # 2^16, so the default factor 2 would skip all eight steps and no update would ever move the weights under the W^T shadows; 16 reaches
    # 2^12 after three skips and leaves five applied updates (asserted below)
    return FP16_Optimizer_State(FusedAdam(_groups(model), lr=3e-4, bias_correction=False, max_grad_norm=1.0), dynamic_loss_scale=True,
                                dynamic_loss_args={"init_scale": 2.0 ** 24, "scale_factor": 16.0}, verbose=False)


def _fused_state(model, opt):
    eng = model.engine
    d = collections.OrderedDict(("param " + k, t) for k, t in eng.flat.items())
    for i, k in enumerate(opt._group_key):
        d["master " + k], d["exp_avg " + k], d["exp_avg_sq " + k] = opt.fp32_groups_flat[i], opt._m[i], opt._v[i]
    d["loss-scale state"], d["overflow"] = opt._scale_state, opt._ovf          # (cur_scale, cur_iter, last_overflow_iter, ..., skipped_steps)
    return d


def _bert_state(model, opt):
    d = collections.OrderedDict(("param " + k, t) for k, t in model.engine.flat.items())
    for j, fg in enumerate(opt._flat):
        d["master %d" % j], d["next_m %d" % j], d["next_v %d" % j] = fg.p32, fg.m, fg.v
    d["step"] = opt._step
    return d


def _optimizer_loop(scenario, steps, make_opt, copy_state, state_of):
    tpl = _template("img2txt", 3)
    used = _new(tpl)
    opt = make_opt(used)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", VlpPerformanceWarning)
        for i, step in enumerate(steps):
            seed = 1000 + 17 * i
            got = _run(used, step, seed, opt=opt)              # through used's own parameter / shadow waits, before anything else touches them
            fresh = _fresh_from(tpl, used, "scenario %s, step %d" % (scenario, i))
            fopt = make_opt(fresh)
            copy_state(opt, fopt)
            _same(scenario, i, step.kind + ", optimizer state handed to the fresh model", state_of(fresh, fopt), state_of(used, opt))
            want = _run(fresh, step, seed, opt=fopt)
            _same(scenario, i, step.kind, got, want)
            opt.step()
            fopt.step()
            torch.cuda.synchronize()
            _same(scenario, i, step.kind + ", after optimizer.step()", state_of(used, opt), state_of(fresh, fopt))
    return used, opt


@pytest.mark.parametrize("pipelined", ["0", "1"], ids=["plain", "pipelined"])
def test_d_fused_adam_in_the_loop(pipelined, monkeypatch):
    """Eight steps MLM / pretext / packed MLM / empty masked_pos under FP16_Optimizer_State(FusedAdam), dynamic loss scale from 2^24 (the
    first steps overflow and are skipped).  The step after every opt.step() must equal a fresh model loaded from used's weights: a W^T
    shadow that lags an update, or a parameter event consumed twice, would show in the first gradient the dgrad chain produces."""
    monkeypatch.setenv("VLP_ADAM_PIPELINE", pipelined)
    b1, b2 = _batch(4, 20, 401), _batch(4, 20, 402)
    cycle = [Step("mlm", b1), Step("pretext", b2), Step("mlm", b2, True), Step("empty", _emptied(b1))]

    def copy_state(src, dst):
        assert dst.pipeline_with_forward == (pipelined == "1") and dst._group_key == src._group_key
        for a, b in zip(dst.fp32_groups_flat + dst._m + dst._v + [dst._scale_state, dst._ovf],
                        src.fp32_groups_flat + src._m + src._v + [src._scale_state, src._ovf]):
            a.copy_(b)
    used, opt = _optimizer_loop("D/FusedAdam " + ("pipelined" if pipelined == "1" else "plain"), [cycle[i % 4] for i in range(8)], _fused_adam,
                                copy_state, _fused_state)
    assert opt.skipped_steps >= 1 and opt.applied_steps >= 2, (opt.skipped_steps, opt.applied_steps)


def test_d_bert_adam_in_the_loop():
    """Three steps on the BertAdam path (fp32 masters, fp16 compute, static gradient scale: the --allow_fp16_compute configuration)."""
    b1, b2 = _batch(4, 20, 411), _batch(4, 20, 412)

    def make(model):
        opt = BertAdam(_groups(model), lr=1e-3, warmup=0.1, t_total=20)
        opt.grad_scale = SCALE
        opt._build()
        return opt
    used, opt = _optimizer_loop("D/BertAdam", [Step("mlm", b1), Step("pretext", b2), Step("mlm", b2)], make,
                                lambda src, dst: dst.load_state_dict(src.state_dict()), _bert_state)
    assert opt._step == 3


# =====================================================================================================================================
# E. packing caches under churn
# =====================================================================================================================================
E_NV, E_MAXB, E_STEPS = 8, 32, 70
E_FULL = (1, 9, 64, 65, 66, 70)     # 1-based: first step, staging-ring wrap (8 slots), around the _pk_cache clear at 64 entries, last


@functools.lru_cache(maxsize=None)
def _churn_raws():
    """70 batches (B = 3, 8 regions, L = 43) with 70 DISTINCT kept-length tuples, each shorter than 3 x L."""
    raws, seen, seed = [], set(), 3500
    while len(raws) < E_STEPS:
        r = _raw(3, E_MAXB, seed, Nv=E_NV)
        seed += 1
        lens = tuple(_kept(r))
        if lens in seen or sum(lens) >= 3 * r.input_ids.shape[1]:
            continue
        seen.add(lens)
        raws.append(r)
    return raws


def _as_spec(raw):
    nb = [n - (E_NV + 3) for n in _kept(raw)]
    return MaskSpec.from_lengths(E_NV, nb, [int(t) == 3 for t in raw.task_idx], device=DEV)


@pytest.mark.parametrize("form", ["dense_mask", "mask_spec"])
def test_e_packing_caches_under_churn(form, monkeypatch):
    """70 steps, 70 distinct length tuples, varlen = True: a new dense int64 mask tensor every step (_pk_lens pruning, the read-back
    streak warning -- once) or MaskSpec.  Every step: loss and logits bit-equal to a long-lived dense engine and every gradient within
    test_25's 2e-4 rel-L2; full bit equality with a fresh packed engine at steps 1, 9, 64, 65, 66 and 70.  Then (dense masks) the
    resident tensors are overwritten in place with shorter captions -- last_packed_rows follows, the step equals fresh -- and handed over
    again unmodified: no second read-back."""
    tpl = _template("img2txt", 2, E_NV)
    raws = _churn_raws()
    L = raws[0].input_ids.shape[1]
    used, dense = _new(tpl, True), _new(tpl, False)
    batches = []
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        for i, raw in enumerate(raws):
            b = S.batch_to(raw, DEV, half=True)
            if form == "mask_spec":
                b = b._replace(input_mask=_as_spec(raw))
                if i == 0:
                    assert torch.equal(b.input_mask.dense(L).cpu(), raw.input_mask)
            batches.append(b)                                   # (kept alive: 70 live entries for _pk_lens to prune)
            tag, step, seed = "E/" + form, Step("mlm", b, True), 1000 + 17 * i
            if i + 1 in E_FULL:
                got, _ = _used_vs_fresh(tag, i, step, used, tpl)
            else:
                got = _run(used, step, seed)
            assert got["last_packed_rows"] == sum(_kept(raw)), (i, got["last_packed_rows"], _kept(raw))
            ref = _run(dense, step._replace(varlen=False), seed)
            assert ref["last_packed_rows"] is None
            _same(tag, i, "mlm, packed against the long-lived dense engine", got, ref, keys=lambda d: [k for k in d if k.startswith("loss") or k == "logits"])
            names = [k for k in got if k.startswith("grad ")]
            # (a tensor whose dense gradient is all zero -- the pooler -- must be all zero in the packed run too)
            rel = torch.stack([(got[k].float() - ref[k].float()).norm() / ref[k].float().norm().clamp(min=1e-30) for k in names]).tolist()
            for k, v in zip(names, rel):
                assert v <= 2e-4, "scenario %s, step %d: %s packed against dense rel-L2 %.3e" % (tag, i, k, v)
    perf = [w for w in caught if issubclass(w.category, VlpPerformanceWarning)]
    assert len(perf) == (1 if form == "dense_mask" else 0), [str(w.message) for w in perf]
    if form != "dense_mask":
        return
    # ---- resident tensors overwritten in place with shorter captions -------------------------------------------------------------------
    b, raw_old = batches[-1], raws[-1]
    raw_new = _raw(3, 10, 3400, Nv=E_NV, pad_to=L)
    assert sum(_kept(raw_new)) < sum(_kept(raw_old))
    version = b.input_mask._version
    for dst, src in zip(b, S.batch_to(raw_new, DEV, half=True)):
        dst.copy_(src)
    assert b.input_mask._version > version
    calls = []
    real = torch.Tensor.tolist
    monkeypatch.setattr(torch.Tensor, "tolist", lambda self: (calls.append(1), real(self))[1])
    got, _ = _used_vs_fresh("E/dense_mask, mask overwritten in place", E_STEPS, Step("mlm", b, True), used, tpl)
    assert got["last_packed_rows"] == sum(_kept(raw_new))
    assert len(calls) >= 2                                       # used and fresh each read the lengths back
    del calls[:]
    again = _run(used, Step("mlm", b, True), 1000 + 17 * E_STEPS)
    assert len(calls) == 0, "the same unmodified mask tensor was read back again"
    monkeypatch.undo()
    _same("E/dense_mask, same tensors again", E_STEPS + 1, "mlm", again, got)


# =====================================================================================================================================
# F. other forwards in between
# =====================================================================================================================================
def test_f_other_forwards_between_training_steps():
    """img2txt: MLM step, eval() + no_grad forward, score_samples with explicit position ids + log-probability backward, the sampling
    decoder (Engine.decode_greedy(sample=True), as the SCST step draws), MLM step -- each bit-equal to a fresh engine; a backward whose
    activations a later forward overwrote still raises, and the engine is fit for the next step."""
    tpl = _template("img2txt", 3)
    b1, b2 = _batch(4, 20, 601), _batch(4, 20, 602)
    dec = _decoder_inputs(4, 8, 603)
    used, _ = _walk("F/img2txt", tpl, [Step("mlm", b1), Step("eval", b2), Step("logprob", dec), Step("decode", dec), Step("mlm", b2)])
    lt = _call(used, b1, False)
    _call(used, b2, False)
    with pytest.raises(RuntimeError, match="activations of this forward were overwritten"):
        ((lt[0] + lt[1] + lt[2]) * SCALE).backward()
    _walk("F/img2txt after the refused backward", tpl, [Step("mlm", b1)], used=used)


def test_f_vqa_steps_around_inference():
    """vqa2: dense-label step, SparseAnswers step, answer() (padding-free: MaskSpec with host lengths), dense-label step."""
    tpl = _template("vqa2", 3)
    raw = _raw(5, 20, 611, tasks="vqa2")
    b = S.batch_to(raw, DEV, half=True)
    rows = [[-1] * 10, [1 + 7 * k for k in range(10)], [3128] * 9 + [0], [5, 6] * 5, [17] * 10]
    sparse = SparseAnswers.from_answer_ids(rows, unk_index=-1).to(DEV)
    spec = MaskSpec.from_lengths(100, [n - 103 for n in _kept(raw)], False, device=DEV)
    assert torch.equal(spec.dense(raw.input_mask.shape[1]).cpu(), raw.input_mask)
    steps = [Step("vqa", b), Step("vqa", b._replace(ans_labels=sparse)), Step("answer", b._replace(input_mask=spec), True), Step("vqa", b)]
    used, outs = _walk("F/vqa2", tpl, steps, scale=1.0)
    assert outs[2]["last_packed_rows"] == sum(_kept(raw))
