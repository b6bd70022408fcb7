"""Shared by tests/test_consensus_cpu.py and tests/test_87_consensus_gpu.py (no test in here): the cases of the consensus selection, its error
bound, the host results (computed once per case and left unchanged) and the hard rows regrouped as samples.  The samples, the tables and the
independent restatement of CIDEr-D are tests/scst_df_util.py's."""
import functools

import numpy as np

from tests import scst_df_util as U
from vlp_amd import consensus as CS

# (G, T, K), all with seed 0: one other sample; the 1024-thread block; T = 1 (no bigram, zero lengths); T = 64 (no idle lane); rows without a
# 0; an odd group count
CASES = [(1, 4, 2), (3, 5, 4), (5, 21, 5), (65, 64, 3), (4, 3, 16), (2, 1, 16), (16, 21, 16), (3, 64, 16)]
CASE_IDS = ["G%d_T%d_K%d" % c for c in CASES]
SEED = 0


def bound(T, K):
    """Of a utility against fp64: the project's per-score bound plus one rounding per accumulated reference and per penalty product, on values
    <= 10."""
    return U.bound(T) + 2 * (K + 1) * 2.0 ** -24 * 10


def samples(G, T, K, seed=SEED):
    """int64 [K*G, T], row k*G + g = sample k of image g: scst_df_util's hypotheses, copies of a reference of their group with 30 % redrawn."""
    return U.make_corpus(G, 5, T, K, seed)[0]


def others(ids, K):
    """[K*G, K-1, T]: each row's other samples in ascending j, and the counts (all K - 1)."""
    KG, T = ids.shape
    G = KG // K
    ref = np.zeros((KG, K - 1, T), dtype=np.int64)
    for i in range(KG):
        k, g = divmod(i, G)
        ref[i] = np.stack([ids[j * G + g] for j in range(K) if j != k])
    return ref, np.full(KG, K - 1, dtype=np.int32)


def restated(ids, K, tab, dtype=np.float64):
    """The utilities by scst_df_util.restated_scores: K*G groups of one hypothesis, the other samples as references."""
    ref, count = others(ids, K)
    return U.restated_scores(ids, ref, count, 1, tab, dtype)[0]


def pair_host(ids, K, tab):
    """[G, K, K] float64: the host scorer's score of sample k with sample j as its only reference; 0 on the diagonal."""
    KG, T = ids.shape
    G = KG // K
    idx = [(g, k, j) for g in range(G) for k in range(K) for j in range(K) if j != k]
    hyp = np.stack([ids[k * G + g] for g, k, j in idx])
    ref = np.stack([ids[j * G + g] for g, k, j in idx])[:, None, :]
    s = U.host_scores(hyp, ref, np.ones(len(idx), dtype=np.int32), 1, df=tab)
    out = np.zeros((G, K, K))
    for (g, k, j), v in zip(idx, s):
        out[g, k, j] = v
    return out


@functools.lru_cache(maxsize=None)
def host(case, which):
    """(ids, table, utility float64 [K*G], pick [G]) of a case against table(T, which), by consensus_utility; computed once.  Read only."""
    G, T, K = case
    ids, tab = samples(G, T, K), U.table(T, which)
    utility, pick = CS.consensus_utility(ids, K, tab)
    for a in (ids, utility, pick):
        a.setflags(write=False)
    return ids, tab, utility, pick


def first_argmax(values, K):
    """The lowest k with the largest value per image, by a plain loop (independent of numpy's argmax)."""
    v = np.asarray(values).reshape(K, -1)
    out = []
    for g in range(v.shape[1]):
        best = 0
        for k in range(1, K):
            if v[k, g] > v[best, g]:
                best = k
        out.append(best)
    return np.array(out)


def decisive(utility, K, margin):
    """bool [G]: the two largest utilities of the image differ by more than `margin`."""
    s = np.sort(np.asarray(utility).reshape(K, -1), axis=0)
    return (s[-1] - s[-2]) > margin


def check_pick(pick, dev_utility, host_utility, K, T):
    """The three rules of a pick: (a) the first argmax of the device's own stored utilities, exactly; (b) the host utility of the picked sample
    is within 2 bound of the host maximum; (c) where the host's two largest differ by more than 2 bound, the host's pick."""
    pick = np.asarray(pick)
    G = len(pick)
    assert np.array_equal(pick, first_argmax(dev_utility, K)), (pick, first_argmax(dev_utility, K))
    hu = np.asarray(host_utility).reshape(K, G)
    b = bound(T, K)
    assert (hu[pick, np.arange(G)] >= hu.max(axis=0) - 2 * b).all()
    sure = decisive(host_utility, K, 2 * b)
    assert np.array_equal(pick[sure], first_argmax(host_utility, K)[sure])
    return int(sure.sum())


def hard_rows(garbage=True):
    """24 rows of scst_df_util.hard_case (T = 8): its 12 hypotheses and 12 of its valid reference rows, read as K = 2 (G = 12) or K = 4 (G = 6)
    samples.  garbage=False: the same rows with everything behind a row's first 0 zeroed -- the two differ in nothing else."""
    hyp, ref, count = U.hard_case(garbage)
    assert list(count) == [1, 2, 2, 3, 1, 2]
    rows = list(hyp) + [ref[g, 0] for g in range(6)] + [ref[g, 1] for g in (1, 2, 3, 5)] + [ref[3, 2], hyp[6 + 2]]
    return np.stack(rows).astype(np.int64)
