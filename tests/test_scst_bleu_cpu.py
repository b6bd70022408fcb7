"""CPU: sentence BLEU-4 as the second metric of the SCST reward -- the host class vlp_amd.scst.Bleu on hand-worked cases, the cider_weight /
bleu_weight keywords of the three host reward functions, and the entry script's two flags.  The kernel's twin is
tests/test_84_scst_bleu_gpu.py."""
import math
from collections import OrderedDict

import numpy as np
import pytest
import torch

from tests import scst_bleu_util as BU
from tests import scst_samples_util as SU
from vlp_amd import scst as SC
from vlp_amd.input_prep import CaptionRefs

TINY, SMALL = 1e-15, 1e-9


def score(hyp, refs):
    """(stats, bleu_1..4) of one hypothesis string against its reference strings, through compute_score."""
    b = SC.Bleu()
    mean, scores = b.compute_score(OrderedDict([(0, list(refs))]), OrderedDict([(0, [hyp])]))
    assert scores.shape == (4, 1) and scores.dtype == np.float64 and mean == scores[3, 0]
    correct, len_h, reflen = b.sentence_stats(hyp, refs)
    return tuple(correct) + (len_h, reflen), scores[:, 0]


# ---- Bleu on hand-worked cases --------------------------------------------------------------------------------------------------------
def test_hypothesis_equal_to_its_only_reference():
    stats, b = score("5 6 7 8 0", ["5 6 7 8 0"])
    assert stats == (5, 4, 3, 2, 5, 5)                         # the terminating 0 is a token
    # every ratio is (c + 1e-15) / (c + 1e-9), and the length ratio is below 1 by 2e-10: 1 up to the tiny / small terms
    assert np.all(np.abs(b - 1.0) < 2e-9) and np.all(b < 1.0)


def test_one_token_hypothesis_has_no_higher_order_guess():
    stats, b = score("0", ["0"])
    assert stats == (1, 0, 0, 0, 1, 1)
    # guess_2..4 = 0: p_k = p_(k-1) * 1e-15 / 1e-9
    want = [1.0, (1e-6) ** (1 / 2), (1e-12) ** (1 / 3), (1e-18) ** (1 / 4)]
    assert np.allclose(b, want, rtol=1e-8, atol=0)
    assert abs(b[3] - 3.1622776e-5) < 1e-11


def test_hypothesis_shorter_than_every_reference_is_brevity_penalised():
    stats, b = score("5 6 0", ["5 6 7 8 0", "9 9 9 9 9 0"])
    # unigrams 5, 6, 0 all occur; bigrams (5 6) yes, (6 0) no; the trigram (5 6 0) no; closest length 5
    assert stats == (3, 1, 0, 0, 3, 5)
    bp = math.exp(1 - 5 / 3)
    want = [1.0 * bp, (1 / 2) ** (1 / 2) * bp, (1 / 2 * TINY / 1) ** (1 / 3) * bp, (1 / 2 * TINY / 1 * TINY / SMALL) ** (1 / 4) * bp]
    assert np.allclose(b, want, rtol=1e-8, atol=0)
    assert abs(b[0] - 0.5134171) < 1e-7 and abs(b[1] - 0.3630407) < 1e-7


def test_two_references_equally_far_the_shorter_is_taken():
    stats, b = score("1 2 3 0", ["1 2 3 4 0", "1 2 0"])
    # 1, 2, 3, 0; (1 2), (2 3) but not (3 0); (1 2 3) but not (2 3 0); no 4-gram.  Lengths 5 and 3 are both 1 away from 4: reflen 3
    assert stats == (4, 2, 1, 0, 4, 3)
    want = [1.0, (2 / 3) ** (1 / 2), (2 / 3 * 1 / 2) ** (1 / 3), (2 / 3 * 1 / 2 * TINY / 1) ** (1 / 4)]
    assert np.allclose(b, want, rtol=1e-8, atol=0)             # no brevity penalty: 4 > 3 (with reflen 5 bleu_1 would be exp(-1/4) = 0.7788)
    assert score("1 2 3 0", ["1 2 0", "1 2 3 4 0"])[0] == stats          # whichever comes first


def test_clipping_a_word_repeated_beyond_every_reference():
    stats, b = score("7 7 7 7 0", ["7 7 1 0"])
    # 7 counts min(4, 2), 0 counts 1; (7 7) counts min(3, 1), (7 0) is not in the reference; no trigram
    assert stats == (3, 1, 0, 0, 5, 4)
    want = [3 / 5, (3 / 5 * 1 / 4) ** (1 / 2), (3 / 5 * 1 / 4 * TINY / 3) ** (1 / 3), (3 / 5 * 1 / 4 * TINY / 3 * TINY / 2) ** (1 / 4)]
    assert np.allclose(b, want, rtol=1e-8, atol=0)


def test_the_maximum_across_references_not_the_sum():
    stats, b = score("7 7 7 0", ["7 7 0", "7 1 0"])
    # 7: max(2, 1) = 2 (the sum would be 3), 0: 1; (7 7): min(2, 1), (7 0): 1; (7 7 0): 1; lengths 3 and 3
    assert stats == (3, 2, 1, 0, 4, 3)
    want = [3 / 4, (3 / 4 * 2 / 3) ** (1 / 2), (3 / 4 * 2 / 3 * 1 / 2) ** (1 / 3), (3 / 4 * 2 / 3 * 1 / 2 * TINY / 1) ** (1 / 4)]
    assert np.allclose(b, want, rtol=1e-8, atol=0)


def test_corpus_builder_offers_matches_and_penalised_rows():
    """The length variation is what brings brevity-penalised rows: test_81's generator alone has none."""
    shape = (5, 3, 21, 2)
    plain = BU.U.make_corpus(*shape, 0)
    assert BU.shares(BU.host_bleu(*plain, 2)[0])[1] == 0.0
    seed = BU.seed_of(shape)
    c4, bp = BU.shares(BU.host_bleu(*BU.make_corpus(*shape, seed), 2)[0])
    assert c4 >= 0.4 and bp >= 0.2
    stats, bleu = BU.host_bleu(*BU.hard_case(True), 2)
    stats0, bleu0 = BU.host_bleu(*BU.hard_case(False), 2)
    assert np.array_equal(stats, stats0) and np.array_equal(bleu, bleu0)
    G = 6
    assert stats[0].tolist() == [1, 0, 0, 0, 1, 6]                         # just 0, against 1000 1001 1002 1009 [SEP] 0
    assert stats[G + 0].tolist() == [6, 5, 4, 3, 6, 6]                     # the reference itself
    assert stats[1].tolist()[4:] == [8, 7] and stats[1, 0] == 4 + 1 + 1 + 1              # no 0: 1001 x5 clipped to 4, 1004, 1009, 1005
    assert stats[G + 1].tolist() == [4 + 1 + 1, 3 + 1 + 1, 2 + 1 + 1, 1 + 1 + 1, 8, 7]   # 1001 six times against four, then [SEP] 0
    assert stats[2].tolist() == [4, 2, 1, 0, 4, 3]                         # the tie: 3, not 5
    assert stats[G + 2].tolist() == [2, 0, 0, 0, 2, 3]


# ---- the host reward functions --------------------------------------------------------------------------------------------------------
def _case(K=2):
    B, R, T = 6, 3, 21
    hyp, ref, count = BU.make_corpus(B, R, T, K, 1)
    return hyp, ref, count, B, T


def _bleu4(hyp, ref, count, mult):
    return BU.host_bleu(hyp, ref, count, mult)[1][3]


def test_pair_reward_functions_with_weights():
    hyp, ref, count, B, T = _case()
    gen, greedy = hyp[:B], hyp[B:]
    refs = CaptionRefs(torch.from_numpy(ref), torch.from_numpy(count))
    one = np.ones(B, dtype=np.int32)
    for fn, args, cnt in ((lambda **kw: SC.self_critical_reward(greedy, ref[:, 0], gen, B, **kw), None, one),
                          (lambda **kw: SC.self_critical_reward_refs(greedy, refs, gen, **kw), None, count),
                          (lambda **kw: SC.self_critical_reward_refs(greedy, ref[:, 0], gen, **kw), None, one)):
        r0, s0 = fn()
        r1, s1 = fn(cider_weight=1.0, bleu_weight=0.0)
        assert np.array_equal(r0, r1) and np.array_equal(s0, s1) and r0.dtype == r1.dtype and s0.dtype == s1.dtype
        rr = ref if cnt is count else ref[:, :1]
        b4 = _bleu4(hyp, rr, cnt, 2)
        assert np.count_nonzero(b4[:B] - b4[B:]) >= B // 2
        rb, sb = fn(cider_weight=0, bleu_weight=1)
        assert np.array_equal(sb, b4) and np.array_equal(rb, np.repeat((b4[:B] - b4[B:])[:, None], T, 1))
        rm, sm = fn(cider_weight=0.5, bleu_weight=2.0)
        want = 0.5 * np.asarray(s0) + 2.0 * b4
        assert np.allclose(sm, want, rtol=0, atol=1e-12) and np.allclose(rm[:, 0], want[:B] - want[B:], rtol=0, atol=1e-12)
        for bad in ((-1.0, 1.0), (1.0, -0.5), (0.0, 0.0), (float("nan"), 1.0), (1.0, float("inf"))):
            with pytest.raises(ValueError):
                fn(cider_weight=bad[0], bleu_weight=bad[1])


def test_group_reward_function_with_weights():
    K = 3
    hyp, ref, count, B, T = _case(K)
    refs = CaptionRefs(torch.from_numpy(ref), torch.from_numpy(count))
    r0, s0 = SC.self_critical_reward_group(hyp, refs, K)
    r1, s1 = SC.self_critical_reward_group(hyp, refs, K, cider_weight=1, bleu_weight=0)
    assert np.array_equal(r0, r1) and np.array_equal(s0, s1)
    b4 = _bleu4(hyp, ref, count, K)
    rb, sb = SC.self_critical_reward_group(hyp, refs, K, cider_weight=0, bleu_weight=1)
    assert np.array_equal(sb, b4) and np.array_equal(rb[:, 0], SU.loo(b4, K)) and np.count_nonzero(rb[:, 0]) >= K * B // 2
    rm, sm = SC.self_critical_reward_group(hyp, refs, K, cider_weight=1.0, bleu_weight=0.5)
    want = np.asarray(s0) + 0.5 * b4
    assert np.allclose(sm, want, rtol=0, atol=1e-12) and np.allclose(rm[:, 0], SU.loo(want, K), rtol=0, atol=1e-12)
    for bad in ((-1.0, 1.0), (0.0, 0.0), (float("nan"), 1.0)):
        with pytest.raises(ValueError):
            SC.self_critical_reward_group(hyp, refs, K, cider_weight=bad[0], bleu_weight=bad[1])


def test_a_scorer_with_weight_zero_is_not_called(monkeypatch):
    hyp, ref, count, B, T = _case()
    calls = []

    class Spy(object):
        def __init__(self, real, name):
            self.real, self.name = real, name

        def compute_score(self, gts, res):
            calls.append(self.name)
            return self.real.compute_score(gts, res)
    monkeypatch.setattr(SC, "_scorer", Spy(SC._scorer, "cider"))
    monkeypatch.setattr(SC, "_bleu", Spy(SC._bleu, "bleu"))
    SC.self_critical_reward(hyp[B:], ref[:, 0], hyp[:B], B)
    SC.self_critical_reward(hyp[B:], ref[:, 0], hyp[:B], B, cider_weight=1, bleu_weight=0)
    assert calls == ["cider", "cider"]
    del calls[:]
    SC.self_critical_reward(hyp[B:], ref[:, 0], hyp[:B], B, cider_weight=0, bleu_weight=1)
    assert calls == ["bleu"]
    del calls[:]
    SC.self_critical_reward_group(hyp, ref[:, 0], 2, cider_weight=2, bleu_weight=1)
    assert sorted(calls) == ["bleu", "cider"]


# ---- entry script -------------------------------------------------------------------------------------------------------------------
def test_parser_flags_defaults_and_refusals():
    from vlp_amd import run_img2txt_dist as R
    base = ["--enable_butd", "--fp16"]
    args = R.derive_args(R.build_parser().parse_args(base))
    assert args.scst_cider_weight == 1.0 and args.scst_bleu_weight == 0.0
    assert isinstance(args.scst_cider_weight, float) and isinstance(args.scst_bleu_weight, float)
    for flag in ("--scst_cider_weight", "--scst_bleu_weight"):
        with pytest.raises(ValueError, match="need --scst"):
            R.derive_args(R.build_parser().parse_args(base + [flag, "0.5"]))                                           # no --scst
    scst = base + ["--scst", "--max_pred", "0", "--mask_prob", "0"]
    args = R.derive_args(R.build_parser().parse_args(scst + ["--scst_bleu_weight", "0.5", "--scst_reward", "device", "--scst_samples", "3"]))
    assert (args.scst_cider_weight, args.scst_bleu_weight) == (1.0, 0.5)
    args = R.derive_args(R.build_parser().parse_args(scst + ["--scst_cider_weight", "0", "--scst_bleu_weight", "1"]))
    assert (args.scst_cider_weight, args.scst_bleu_weight) == (0.0, 1.0)
    for bad in (["--scst_bleu_weight", "-1"], ["--scst_cider_weight", "-0.5"], ["--scst_cider_weight", "0"], ["--scst_bleu_weight", "nan"],
                ["--scst_cider_weight", "inf"]):
        with pytest.raises(ValueError):
            R.derive_args(R.build_parser().parse_args(scst + bad))
    with pytest.raises(SystemExit):
        R.build_parser().parse_args(scst + ["--scst_bleu_weight", "half"])


def test_scst_step_passes_the_weights_only_when_they_are_set(monkeypatch):
    from tests.test_scst_reward_cpu import _Model, _Opt, _stub_batch
    from vlp_amd import run_img2txt_dist as R
    B, Nv, T = 3, 4, 6
    batch = _stub_batch(B, Nv, T)
    seen = []

    def host(greedy, gt, gen, n, **kw):
        seen.append(kw)
        return np.zeros((n, gen.shape[1])), np.zeros(2 * n)
    monkeypatch.setattr(SC, "self_critical_reward", host)

    def crit(logp, seq, reward):
        return logp.sum()
    marks = []
    R.scst_step(_Model(B, T), _Opt(), batch, 1e-5, Nv, crit)
    R.scst_step(_Model(B, T), _Opt(), batch, 1e-5, Nv, crit, reward_weights=(1.0, 0.0))
    R.scst_step(_Model(B, T), _Opt(), batch, 1e-5, Nv, crit, reward_weights=(1, 0.5), mark=marks.append)
    assert seen == [{}, {}, {"cider_weight": 1.0, "bleu_weight": 0.5}]
    assert marks == ["greedy_decode", "sample_forward", "reward_host", "backward", "optimizer"]          # the phase marks do not change
