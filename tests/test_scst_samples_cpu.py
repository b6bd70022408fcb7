"""CPU: the host specification of SCST with K samples per image and a leave-one-out baseline (vlp_amd.scst.self_critical_reward_group) and
the command line of --scst_samples.  tests/test_83_scst_samples_gpu.py checks the kernels, the decoder and the step against it."""
import numpy as np
import pytest
import torch

from tests import scst_df_util as U
from tests import scst_samples_util as SU
from vlp_amd import scst as SC
from vlp_amd.input_prep import CaptionRefs


def test_hand_worked_case():
    """B = 2 images with the one-token references "5" and "6", K = 3 samples each (T = 1: a string is its one id, there are no bigrams, so
    the length penalty is 1 and the orders 2..4 contribute 0).  The 6 hypotheses list their image's reference: 6 reference sets, df("5") =
    df("6") = 3, idf = log 6 - log 3 = log 2 for both.  A sample equal to its reference has cosine 1 in order 1: score 10 * (1 + 0 + 0 + 0) / 4
    = 2.5; any other sample shares nothing: 0.
      rows (k*B + b):  k0 = ("5", "5"), k1 = ("6", "6"), k2 = ("5", "5")   ->  scores (2.5, 0, 0, 2.5, 2.5, 0)
      image 0 has (2.5, 0, 2.5): 2.5 - (0 + 2.5) / 2 = 1.25, 0 - (2.5 + 2.5) / 2 = -2.5, 1.25
      image 1 has (0, 2.5, 0):   0 - (2.5 + 0) / 2 = -1.25,  2.5 - 0 = 2.5,              -1.25"""
    gen = np.array([[5], [5], [6], [6], [5], [5]])
    refs = np.array([[5], [6]])
    reward, scores = SC.self_critical_reward_group(gen, refs, 3)
    assert reward.shape == (6, 1) and reward.dtype == np.float64 and scores.shape == (6,)
    assert np.abs(scores - [2.5, 0, 0, 2.5, 2.5, 0]).max() <= 1e-12, scores
    assert np.abs(reward[:, 0] - [1.25, -1.25, -2.5, 2.5, 1.25, -1.25]).max() <= 1e-12, reward
    # tensors are accepted like arrays, the reward is repeated over the columns
    gen3 = np.concatenate([gen, np.zeros((6, 2), dtype=np.int64)], 1)
    r3, _ = SC.self_critical_reward_group(torch.from_numpy(gen3), torch.from_numpy(np.array([[5, 0, 0], [6, 0, 0]])), 3)
    assert r3.shape == (6, 3) and np.array_equal(r3, np.repeat(r3[:, :1], 3, 1))


def test_two_samples_are_each_other_s_baseline():
    G, R, T = 5, 3, 21
    hyp, ref, count = U.make_corpus(G, R, T, 2, 0)
    refs = CaptionRefs(torch.from_numpy(ref), torch.from_numpy(count))
    reward, scores = SC.self_critical_reward_group(hyp, refs, 2)
    assert np.count_nonzero(reward[:G, 0]) >= G // 2 + 1
    assert np.array_equal(reward[:G, 0], scores[:G] - scores[G:]) and np.array_equal(reward[G:, 0], scores[G:] - scores[:G])
    # the scores are those of the one-sample estimator's call with the same 2G hypotheses
    _, s2 = SC.self_critical_reward_refs(hyp[G:], refs, hyp[:G])
    assert np.array_equal(scores, s2)


@pytest.mark.parametrize("K", [2, 3, 5, 16])
def test_rewards_of_a_group_sum_to_zero(K):
    G, R, T = 4, 2, 9
    hyp, ref, count = U.make_corpus(G, R, T, K, 3)
    reward, scores = SC.self_critical_reward_group(hyp, CaptionRefs(torch.from_numpy(ref), torch.from_numpy(count)), K)
    assert np.count_nonzero(reward[:, 0]) >= K * G // 2
    sums = reward[:, 0].reshape(K, G).sum(0)
    assert np.abs(sums).max() <= K * 2.0 ** -52 * 10, sums
    assert np.array_equal(reward[:, 0], SU.loo(scores, K))


@pytest.mark.parametrize("ragged", [False, True], ids=["ids", "caption_refs"])
def test_row_k_B_plus_b_is_scored_against_image_b(ragged):
    K, B, T = 3, 4, 7
    R = 3 if ragged else 1
    hyp, ref, count = U.make_corpus(B, R, T, K, 4)
    if ragged:
        count[:] = [1, 3, 2, 3]
        ref[0, 1:] = ref[1, :2]                      # invalid rows hold another image's captions: never read
        refs = CaptionRefs(torch.from_numpy(ref), torch.from_numpy(count))
    else:
        refs = torch.from_numpy(ref[:, 0])
    reward, scores = SC.self_critical_reward_group(hyp, refs, K)
    want = U.host_scores(hyp, ref, count, K)                                   # hypothesis i against group i % B
    assert np.abs(scores - want).max() <= 1e-12
    assert np.count_nonzero(want) >= K * B // 2
    assert np.abs(reward[:, 0] - SU.loo(want, K)).max() <= 1e-12
    # image-major rows are another call: the scores move
    wrong = hyp.reshape(K, B, T).transpose(1, 0, 2).reshape(K * B, T)
    _, s_wrong = SC.self_critical_reward_group(wrong, refs, K)
    assert np.abs(np.sort(s_wrong) - np.sort(scores)).max() > 1e-3


def test_table_mode_agrees_with_the_restatement():
    G, R, T, K = 5, 3, 21, 5
    hyp, ref, count = U.make_corpus(G, R, T, K, 2)
    tab = U.table(T, 0)
    reward, scores = SC.self_critical_reward_group(hyp, CaptionRefs(torch.from_numpy(ref), torch.from_numpy(count)), K, df=tab)
    want, _ = U.restated_scores(hyp, ref, count, K, tab)
    assert np.count_nonzero(want) == K * G
    assert np.abs(scores - want).max() <= 1e-9, np.abs(scores - want).max()
    assert np.abs(reward[:, 0] - SU.loo(want, K)).max() <= 1e-9
    # no K anywhere in table mode: a sample's score does not depend on how many samples its image has
    _, s2 = SC.self_critical_reward_group(hyp[:2 * G], CaptionRefs(torch.from_numpy(ref), torch.from_numpy(count)), 2, df=tab)
    assert np.array_equal(s2, scores[:2 * G])
    batch, _ = SC.self_critical_reward_group(hyp, CaptionRefs(torch.from_numpy(ref), torch.from_numpy(count)), K)
    assert np.abs(batch - reward).max() > 1e-2                                  # another reward than the batch mode's


def test_bad_sample_counts_are_refused():
    gen = np.ones((6, 3), dtype=np.int64)
    refs = np.ones((2, 3), dtype=np.int64)
    for K in (0, 1, 17):
        with pytest.raises(ValueError):
            SC.self_critical_reward_group(gen, refs, K)
    with pytest.raises(ValueError):
        SC.self_critical_reward_group(gen[:5], refs, 2)                         # 5 rows are not 2 samples of every image


def _args(extra):
    from vlp_amd import run_img2txt_dist as R
    return R.derive_args(R.build_parser().parse_args(["--enable_butd", "--fp16"] + extra))


def test_scst_samples_command_line():
    scst = ["--scst", "--max_pred", "0", "--mask_prob", "0"]
    assert _args([]).scst_samples == 1 and _args(scst).scst_samples == 1
    assert _args(scst + ["--scst_samples", "2"]).scst_samples == 2 and _args(scst + ["--scst_samples", "16"]).scst_samples == 16
    for bad in ("0", "17", "-1"):
        with pytest.raises(ValueError, match="scst_samples"):
            _args(scst + ["--scst_samples", bad])
    with pytest.raises(ValueError, match="needs --scst"):
        _args(["--scst_samples", "2"])
    # K x images per step is bounded by the decode: 1024 sequences
    assert _args(scst + ["--scst_samples", "16", "--train_batch_size", "64"]).scst_samples == 16
    with pytest.raises(ValueError, match="at most 1024"):
        _args(scst + ["--scst_samples", "16", "--train_batch_size", "65"])
    a = _args(scst + ["--scst_samples", "16", "--train_batch_size", "128", "--gradient_accumulation_steps", "2"])
    assert a.train_batch_size == 64
