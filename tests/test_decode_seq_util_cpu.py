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
