"""Helpers of the decoder call-sequence tests (tests/test_46_decode_sequence_gpu.py) that need no GPU: the description of one decoder
call, inputs that differ from seed to seed in EVERY tensor a captured token step reads, the launch-plan keys a sequence of calls must
leave in a decode workspace, and the small bookkeeping of the comparisons.  Only torch, the synthetic ids and oracle/make_golden's
decode_inputs are imported; the CPU tests of this file are in tests/test_decode_seq_util_cpu.py."""
import collections

import torch

from oracle.make_golden import decode_inputs

# what: the call kind as a failure message names it ("greedy", "sample", "samples K=3 T=0.8 k=20 p=0.9", "beam min_len=3", ...)
# case: (B, T, seed) of varied_inputs
# attrs: attributes set on the model in front of the call, the way decode_img2txt sets them (search_beam_size, min_len, ngram_size, ...)
# kwargs: keywords of model.forward (sample_mode, n_samples, temperature, top_k, top_p)
Call = collections.namedtuple("Call", ["what", "case", "attrs", "kwargs"])
Call.__new__.__defaults__ = ({}, {})

# every attribute of BertForSeq2SeqDecoder a call of the scenarios may move, at its resting value: a Call's attrs are laid over these, so
# that no call inherits what the one before it set
BEAM_DEFAULTS = dict(search_beam_size=1, min_len=0, forbid_duplicate_ngrams=False, forbid_ignore_set=None, ngram_size=3,
                     ngram_blocking="device", backtrack="host", n_best=1)


def attrs_of(call, eos_id):
    a = dict(BEAM_DEFAULTS, eos_id=eos_id)
    a.update(call.attrs)
    return a


def varied_inputs(B, T, seed, Nv=100):
    """decode_inputs(B, T, seed) with a per-sample number of visible regions and an offset on the position ids, both drawn from the seed:
    decode_inputs alone varies only the image tensors, and a stale copy of mask, segment or position ids would go unseen."""
    img, vis_pe, input_ids, token_type, pos, am = decode_inputs(B, T, seed, Nv)
    g = torch.Generator().manual_seed(seed + 1)
    valid = torch.randint(Nv // 2, Nv + 1, (B,), generator=g).tolist()
    for b, n in enumerate(valid):
        am[b, :, 1 + n:1 + Nv] = 0
    return img, vis_pe, input_ids, token_type, pos + 1 + seed % 7, am


def calls_until_replayed(workspace_calls):
    """How often a call kind must be made until its token steps were replayed: the first call of a workspace runs plainly, the second
    captures (and replays what it captured), the third replays; a kind that is new to a used workspace captures at once."""
    return 3 if workspace_calls == 0 else 2


def greedy_plan_keys(n_steps):
    return {("greedy", s) for s in range(1, n_steps)}


def sample_plan_keys(n_steps, temperature=1.0, top_k=0, top_p=1.0):
    filt = (float(temperature), int(top_k), float(top_p))
    return {("sample_group", s) + (() if filt == (1.0, 0, 1.0) else filt) for s in range(1, n_steps)}


def beam_plan_keys(n_steps, attrs):
    """The plan keys one beam search with these model attributes leaves behind once captured (Engine.decode_beam): frame s blocks eos while
    s + 1 <= min_len; device n-gram blocking adds its size and the sorted ignore list; host blocking captures nothing."""
    if attrs["forbid_duplicate_ngrams"] and (attrs["ngram_blocking"] == "host" or attrs["ngram_size"] < 2):
        return set()
    tag = ()
    if attrs["forbid_duplicate_ngrams"]:
        tag = ("ngram", int(attrs["ngram_size"]), tuple(sorted(int(t) for t in (attrs["forbid_ignore_set"] or ()))))
    min_len = attrs["min_len"]
    return {("beam", s, int(attrs["eos_id"]), bool(min_len) and s + 1 <= min_len) + tag for s in range(1, n_steps)}


def named_outputs(result, extra=None):
    """What a decoder call returned -- an (ids, values) pair or beam_search's traces dict -- as an ordered {name: tensor}."""
    if isinstance(result, dict):
        out = collections.OrderedDict((k, result[k]) for k in sorted(result))
    else:
        out = collections.OrderedDict(zip(("ids", "values"), result))
        assert len(out) == len(result) == 2
    for k, v in (extra or {}).items():
        out[k] = v
    return out


def snapshot(outputs):
    return collections.OrderedDict((k, v.clone() if torch.is_tensor(v) else v) for k, v in outputs.items())


def margin_share(margin, tol):
    """Share of the positions of a greedy decode whose top-1 / top-2 logit margin lies under `tol`: the positions at which a decoder in
    another precision may pick the other token."""
    m = torch.as_tensor(margin)
    return float((m < tol).sum()) / m.numel()
