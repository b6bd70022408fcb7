"""CPU: the helpers of the decoder call-sequence tests (tests/decode_seq_util.py), and the ownership of what vlp_amd.engine.sample_major
returns (the expression Engine.decode_sample_group hands its results over with)."""
import torch

from oracle.make_golden import decode_inputs
from tests.decode_seq_util import (BEAM_DEFAULTS, Call, attrs_of, beam_plan_keys, calls_until_replayed, greedy_plan_keys, margin_share,
                                   named_outputs, sample_plan_keys, snapshot, varied_inputs)
from vlp_amd.engine import sample_major


def test_sample_major_permutes_and_owns_its_memory_for_every_k():
    B, n, Lcap = 3, 4, 7
    for Ks in (1, 2, 3):
        src = torch.arange(B * Ks * Lcap).view(B * Ks, Lcap)
        out = sample_major(src, B, Ks, n)
        assert tuple(out.shape) == (Ks * B, n) and out.is_contiguous()
        for b in range(B):
            for k in range(Ks):
                assert torch.equal(out[k * B + b], src[b * Ks + k, :n])
        lo, hi = src.data_ptr(), src.data_ptr() + src.numel() * src.element_size()
        assert not lo <= out.data_ptr() < hi, "K = %d: the result lies inside its source" % Ks
        kept = out.clone()
        src.zero_()
        assert torch.equal(out, kept)
    # the expression this replaced: a copy at K = 2, the source's own memory at K = 1
    src = torch.arange(B * Lcap).view(B, Lcap)
    assert src[:, :n].view(B, 1, n).transpose(0, 1).reshape(B, n).data_ptr() == src.data_ptr()


def test_decoder_names_resolve_on_the_engine():
    """The decoders are a base class of Engine (vlp_amd/decoder.py); what tests, tools and modeling.py use stays on Engine, and a switch
    assigned on Engine is the one the decoders read."""
    import vlp_amd.engine as E
    from vlp_amd.decoder import Decoder
    assert issubclass(E.Engine, Decoder) and E.sample_major is sample_major
    for name in ("decode_greedy", "decode_sample_group", "decode_beam", "beam_nbest", "_run_planned", "_decode_static_inputs", "score_samples"):
        assert callable(getattr(E.Engine, name)), name
    assert E.Engine.DEC_SPLITS == 4 and E.Engine.NGRAM_MAX_FRAMES == 256
    assert isinstance(E.Engine.DECODE_FUSED, bool) and isinstance(E.Engine.DECODE_GRAPHS, bool)


def test_decode_steps_runs_or_plans_every_step_once():
    """The token-step loop with the model step and the planner replaced by recorders: step 0 and its selection are run; a step whose
    plan_key is None is run, any other goes to _run_planned under that key; the host hook follows every step; the workspace counts
    the call once, at the end."""
    from vlp_amd.decoder import Decoder, _Call

    class Rec(Decoder):
        def __init__(self):
            self.log = []

        def _decode_model_step(self, ws, caches, Lcap, xids, tt, pid, mask_view, R, T, st, first, prefix=None):
            self.log.append(("model", caches, R, T, st, first, prefix, tuple(mask_view.shape), ws["calls"]))

        def _run_planned(self, ws, key, fn):
            self.log.append(("planned", key))
            fn()

    B, Kb, in_len, n = 2, 3, 5, 4
    out_len = in_len + n
    ws = dict(kv="kv", xids=None, tt_steps=[None] * out_len, pid_steps=[None] * out_len, calls=0)
    ids = torch.zeros(B, out_len, dtype=torch.long)
    call = _Call(ws, B, B * Kb, in_len, out_len, n, in_len + 1, 11, torch.zeros(B * Kb, out_len, out_len), ids, ids, torch.zeros(B, out_len, out_len),
                 None)
    d = Rec()
    d._decode_steps(call, lambda s, first: d.log.append(("select", s, first)), lambda s: "cache%d" % (s & 1), "prefix",
                    lambda s: None if s == 2 else ("kind", s), between=lambda s: d.log.append(("between", s)))
    assert d.log == [("model", "kv", B, in_len + 1, 0, True, None, (B, in_len + 1, in_len + 1), 0), ("select", 0, True), ("between", 0),
                     ("planned", ("kind", 1)), ("model", "cache1", B * Kb, 2, in_len, False, "prefix", (B * Kb, 2, in_len + 2), 0),
                     ("select", 1, False), ("between", 1),
                     ("model", "cache0", B * Kb, 2, in_len + 1, False, "prefix", (B * Kb, 2, in_len + 3), 0), ("select", 2, False), ("between", 2),
                     ("planned", ("kind", 3)), ("model", "cache1", B * Kb, 2, in_len + 2, False, "prefix", (B * Kb, 2, in_len + 4), 0),
                     ("select", 3, False), ("between", 3)]
    assert ws["calls"] == 1


def test_varied_inputs_vary_every_per_call_input():
    a, b = varied_inputs(3, 6, 101), varied_inputs(3, 6, 102)
    plain = decode_inputs(3, 6, 101)
    assert torch.equal(a[0], plain[0]) and torch.equal(a[1], plain[1]) and torch.equal(a[2], plain[2]) and torch.equal(a[3], plain[3])
    assert not torch.equal(a[0], b[0]) and not torch.equal(a[4], b[4]) and not torch.equal(a[5], b[5])
    for inp in (a, b):
        img, vis_pe, ids, tt, pos, am = inp
        assert tuple(am.shape) == (3, 108, 108) and tuple(pos.shape) == (3, 108) and int(pos.max()) < 512 and int(pos.min()) >= 1
        visible = am[:, 0, 1:101].sum(dim=1)
        assert bool((visible >= 50).all()) and bool((visible <= 100).all())
        assert bool((am[:, :, 0] == 1).all()) and bool((am[:, :, 101] == 1).all())          # [CLS] and [SEP] stay visible
        assert torch.equal(am[:, 102:, 102:], torch.tril(torch.ones(6, 6, dtype=torch.long)).expand(3, 6, 6))
    again = varied_inputs(3, 6, 101)
    assert all(torch.equal(x, y) for x, y in zip(a, again))


def test_plan_keys_follow_the_engine_rules():
    assert greedy_plan_keys(4) == {("greedy", 1), ("greedy", 2), ("greedy", 3)}
    assert sample_plan_keys(3) == {("sample_group", 1), ("sample_group", 2)}
    assert sample_plan_keys(3, 1.0, 0, 1.0) == sample_plan_keys(3)
    assert sample_plan_keys(3, 0.7) == {("sample_group", 1, 0.7, 0, 1.0), ("sample_group", 2, 0.7, 0, 1.0)}
    a = attrs_of(Call("beam", (3, 6, 1), dict(search_beam_size=3)), 102)
    assert a["eos_id"] == 102 and a["search_beam_size"] == 3 and a["min_len"] == 0
    assert beam_plan_keys(4, a) == {("beam", 1, 102, False), ("beam", 2, 102, False), ("beam", 3, 102, False)}
    # min_len blocks eos in the frames s with s + 1 <= min_len; frame 0 is never planned
    assert beam_plan_keys(4, dict(a, min_len=2)) == {("beam", 1, 102, True), ("beam", 2, 102, False), ("beam", 3, 102, False)}
    ng = dict(a, forbid_duplicate_ngrams=True, ngram_size=2)
    assert beam_plan_keys(3, ng) == {("beam", 1, 102, False, "ngram", 2, ()), ("beam", 2, 102, False, "ngram", 2, ())}
    assert beam_plan_keys(2, dict(ng, forbid_ignore_set={9, 4})) == {("beam", 1, 102, False, "ngram", 2, (4, 9))}
    assert beam_plan_keys(3, dict(ng, ngram_blocking="host")) == set() and beam_plan_keys(3, dict(ng, ngram_size=1)) == set()
    assert beam_plan_keys(2, dict(a, eos_id=7, n_best=3, backtrack="device")) == {("beam", 1, 7, False)}
    assert attrs_of(Call("greedy", (3, 6, 1)), 5) == dict(BEAM_DEFAULTS, eos_id=5)            # a call sets every attribute back
    assert calls_until_replayed(0) == 3 and calls_until_replayed(1) == 2 and calls_until_replayed(7) == 2


def test_named_outputs_snapshot_and_margin_share():
    pair = (torch.tensor([[1, 2]]), torch.tensor([[0.5, 0.25]]))
    out = named_outputs(pair, {"filter_kept": torch.tensor([3])})
    assert list(out) == ["ids", "values", "filter_kept"] and out["ids"] is pair[0]
    traces = {"wids": torch.zeros(1), "pred_seq": torch.ones(1), "scores": torch.zeros(1)}
    assert list(named_outputs(traces)) == ["pred_seq", "scores", "wids"]
    snap = snapshot(named_outputs(pair, {"seed": 7}))
    assert snap["seed"] == 7 and snap["ids"] is not pair[0] and torch.equal(snap["ids"], pair[0])
    pair[0].zero_()
    assert int(snap["ids"].sum()) == 3
    assert margin_share(torch.tensor([[0.5, 0.001], [0.02, 0.0149]]), 1.5e-2) == 0.5
    assert margin_share(torch.tensor([1.0, 2.0]), 1.5e-2) == 0.0
