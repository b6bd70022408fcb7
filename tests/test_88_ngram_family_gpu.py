"""GPU: identities between the entries of the n-gram scoring family (csrc/reward.hip, csrc/caption_eval.hip).  The kernels are compositions of
the same device pieces (csrc/reward_common.h), so wherever two entries are given the same strings they must agree bit for bit, not within a
tolerance.  At (G, R, T) = (5, 3, 7) and (3, 8, 64):

(a) rows without a 0 -- the one thing the reward's strings (ids up to and including the first 0) and the caption metrics' word strings (ids
    before it) differ in does not occur: caption_eval's cider equals cider_d_df's scores at mult = 1 and its bleu_stats equal bleu4's stats;
(b) cider_d_consensus at K = 2 against cider_d_df at mult = 1, R = 1 with the other sample as the only reference: utility[k*G + g] and
    pair[g][k][1 - k] equal its scores, on rows with and without a 0;
(c) bleu4 with weights (1, 0), base = cider_d_multi's scores and the leave-one-out reward against cider_d_multi's own reward.

All three held on the build before the pieces were shared (whose kernels repeated each other by hand).  That the scores compared are not all
zero is asserted on the host scorer before a kernel output is read."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from tests import scst_df_util as U                                 # noqa: E402
from vlp_amd import _lib as K                                       # noqa: E402

DEV = torch.device("cuda:0")
SHAPES = [(5, 3, 7), (3, 8, 64)]
IDS = ["G%d_R%d_T%d" % s for s in SHAPES]


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def full_rows(G, R, T, mult, seed):
    """A corpus of U.make_corpus's kind in which no row holds a 0: every reference has T words, a hypothesis is a valid reference of its
    group with 30 % of its words redrawn."""
    rng = np.random.RandomState(seed)
    ref = rng.randint(1000, 1012, size=(G, R, T)).astype(np.int64)
    count = rng.randint(1, R + 1, size=G).astype(np.int32)
    hyp = np.zeros((mult * G, T), dtype=np.int64)
    for i in range(mult * G):
        g = i % G
        row = ref[g, rng.randint(count[g])].copy()
        redraw = rng.rand(T) < 0.3
        row[redraw] = rng.randint(1000, 1012, size=int(redraw.sum()))
        hyp[i] = row
    return hyp, ref, count


def cider_d_df(hyp, ref, count, tab):
    """scores f32 [G] of cider_d_df at mult = 1."""
    keys, vals = tab.to(DEV)
    scores = torch.full((hyp.shape[0],), float("nan"), device=DEV)
    K.cider_d_df(torch.from_numpy(hyp).to(DEV), torch.from_numpy(ref).to(DEV), None if count is None else torch.from_numpy(count).to(DEV), 1, scores,
                 keys, vals, tab.n_docs)
    return scores


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_caption_eval_equals_the_reward_entries_on_rows_without_a_zero(shape):
    G, R, T = shape
    hyp, ref, count = full_rows(G, R, T, 1, 3)
    assert not (hyp == 0).any() and not (ref == 0).any()
    tab = U.table(T, 0)
    assert float(np.max(U.host_scores(hyp, ref, count, 1, df=tab))) > 0
    h, r, c = torch.from_numpy(hyp).to(DEV), torch.from_numpy(ref).to(DEV), torch.from_numpy(count).to(DEV)
    keys, vals = tab.to(DEV)
    cider = torch.full((G,), float("nan"), device=DEV)
    stats = torch.full((G, 6), -7, dtype=torch.int32, device=DEV)
    lcs = torch.full((G, R, 2), -7, dtype=torch.int32, device=DEV)
    K.caption_eval(h, r, c, cider, stats, lcs, keys, vals, tab.n_docs)
    b = torch.full((G,), float("nan"), device=DEV)
    want_stats = torch.full((G, 6), -7, dtype=torch.int32, device=DEV)
    K.bleu4(h, r, c, 1, b, stats=want_stats)
    want = cider_d_df(hyp, ref, count, tab)
    torch.cuda.synchronize()
    print("G%d R%d T%d: max cider %.4f, correct_1 %s" % (G, R, T, float(cider.max()), stats[:, 0].tolist()))
    assert float(want.max()) > 0 and int(want_stats[:, 0].max()) > 0
    assert same_bits(cider, want)
    assert torch.equal(stats, want_stats)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_consensus_of_two_equals_cider_d_df_with_the_other_sample_as_reference(shape):
    G, _, T = shape
    ids = U.make_corpus(G, 1, T, 2, 1)[0]                           # [2G, T]: two edited copies of one caption per image, most with a 0
    ids[0] = 1000 + (np.arange(T) * 5) % 12                         # image 0: two rows without a 0
    ids[G] = ids[0]
    ids[G, T // 2] = 1003 if ids[0, T // 2] != 1003 else 1004
    assert (ids[[0, G]] != 0).all() and (ids == 0).any()
    tab = U.table(T, 0)
    other = np.empty((2 * G, 1, T), dtype=np.int64)                 # row k*G + g holds sample 1 - k of image g
    other[:, 0] = np.concatenate([ids[G:], ids[:G]])
    assert float(np.max(U.host_scores(ids, other, np.ones(2 * G, dtype=np.int32), 1, df=tab))) > 0
    keys, vals = tab.to(DEV)
    utility = torch.full((2 * G,), float("nan"), device=DEV)
    pick = torch.full((G,), -7, dtype=torch.int32, device=DEV)
    pair = torch.full((G, 2, 2), float("nan"), device=DEV)
    K.cider_d_consensus(torch.from_numpy(ids).to(DEV), 2, keys, vals, tab.n_docs, utility, pick, pair=pair)
    want = cider_d_df(ids, other, None, tab)
    torch.cuda.synchronize()
    print("G%d T%d: utilities %s" % (G, T, utility.tolist()))
    assert float(want.max()) > 0
    assert same_bits(utility, want)
    assert same_bits(pair[:, 0, 1], want[:G]) and same_bits(pair[:, 1, 0], want[G:])


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_bleu4_at_weights_one_zero_gives_cider_d_multis_reward(shape):
    G, R, T = shape
    mult = 3
    hyp, ref, count = U.make_corpus(G, R, T, mult, 0)
    assert float(np.max(U.host_scores(hyp, ref, count, mult))) > 0
    h, r, c = torch.from_numpy(hyp).to(DEV), torch.from_numpy(ref).to(DEV), torch.from_numpy(count).to(DEV)
    n = mult * G
    scores, want = torch.full((n,), float("nan"), device=DEV), torch.full((n,), float("nan"), device=DEV)
    K.cider_d_multi(h, r, c, mult, scores, reward=want)
    b, mixed, reward = [torch.full((n,), float("nan"), device=DEV) for _ in range(3)]
    K.bleu4(h, r, c, mult, b, base=scores, w_base=1.0, w_bleu=0.0, mixed=mixed, reward=reward, loo=True)
    torch.cuda.synchronize()
    print("G%d R%d T%d: rewards %s" % (G, R, T, reward.tolist()))
    assert float(scores.max()) > 0 and float(want.abs().max()) > 0
    assert same_bits(mixed, scores)
    assert same_bits(reward, want)
