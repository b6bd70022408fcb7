"""Shared by tests/test_caption_metrics_cpu.py and tests/test_85_caption_eval_gpu.py (no test in here): the seeded corpus of test_84 read as
WORD STRINGS (the ids of a row before its first 0; [SEP] = 102 is then just a word), the host values of the three metrics on id rows, the
conditions a corpus of the kernel comparison must meet, a hand-built case of hard rows, and the 7-image source file of the CLI tests."""
import json
from collections import OrderedDict

import numpy as np

from tests import scst_bleu_util as BU
from tests import scst_df_util as U
from vlp_amd import caption_metrics as CM
from vlp_amd import scst as SC

bound = U.bound
# (G, R, T) of the kernel comparison
SHAPES = [(1, 1, 1), (2, 8, 1), (4, 2, 3), (3, 1, 5), (5, 3, 21), (64, 5, 21), (65, 2, 64), (130, 8, 64), (1024, 5, 21)]
TABLE_SEED = 99


def make_corpus(G, R, T, seed):
    """test_84's generator with one hypothesis per group: hyp [G, T], ref [G, R, T], count [G]."""
    return BU.make_corpus(G, R, T, 1, seed)


def clamp(count, g, R):
    return R if count is None else min(max(int(count[g]), 1), R)


def word_lists(hyp, ref, count):
    """(refs, hyps) as CaptionMetrics.score takes them: the rows read as word strings, the valid references of every group."""
    G, R = ref.shape[:2]
    return [[CM.words_of_row(r) for r in ref[g, :clamp(count, g, R)]] for g in range(G)], [CM.words_of_row(h) for h in hyp]


_TABLES = {}


def table(T):
    """Document frequencies of a 200-image corpus of its own (five references per image, strings as long as the case's), so that a kernel
    case of one group does not score 0 everywhere."""
    if T not in _TABLES:
        _, ref, count = U.make_corpus(200, 5, T, 1, TABLE_SEED)
        _TABLES[T] = SC.DocFreq.from_token_lists(word_lists(np.zeros((200, T), dtype=np.int64), ref, count)[0])
    return _TABLES[T]


def brute_lcs(a, b):
    """LCS length by recursion on the two last elements (memoised): shares no code with caption_metrics.lcs_len."""
    memo = {}

    def f(i, j):
        if i == 0 or j == 0:
            return 0
        if (i, j) not in memo:
            memo[(i, j)] = f(i - 1, j - 1) + 1 if a[i - 1] == b[j - 1] else max(f(i - 1, j), f(i, j - 1))
        return memo[(i, j)]
    import sys
    old = sys.getrecursionlimit()
    sys.setrecursionlimit(max(old, 4 * (len(a) + len(b)) + 100))
    try:
        return f(len(a), len(b))
    finally:
        sys.setrecursionlimit(old)


_COUNTS = {}


def host_counts(hyp, ref, count, cache_key=None):
    """The host classes on the word strings of id rows: (bleu_stats int32 [G, 6], lcs int32 [G, R, 2] with (0, 0) for an invalid reference,
    rouge float64 [G]).  cache_key: computed once per key and left unchanged."""
    if cache_key is not None and cache_key in _COUNTS:
        return _COUNTS[cache_key]
    G, R = ref.shape[:2]
    refs, hyps = word_lists(hyp, ref, count)
    bleu, rouge = SC.Bleu(), CM.Rouge()
    stats = np.zeros((G, 6), dtype=np.int32)
    lcs = np.zeros((G, R, 2), dtype=np.int32)
    rl = np.zeros(G)
    for g in range(G):
        correct, len_h, reflen = bleu.sentence_stats(" ".join(map(str, hyps[g])), [" ".join(map(str, r)) for r in refs[g]])
        stats[g] = list(correct) + [len_h, reflen]
        pairs = rouge.sentence_lcs(hyps[g], refs[g])
        lcs[g, :len(pairs)] = pairs
        rl[g] = rouge.from_lcs(len(hyps[g]), pairs)
    if cache_key is not None:
        _COUNTS[cache_key] = (stats, lcs, rl)
    return stats, lcs, rl


def host_cider(hyp, ref, count, tab):
    """CiderD(df=tab) on the word strings of id rows, float64 [G]."""
    refs, hyps = word_lists(hyp, ref, count)
    gts, res = OrderedDict(), OrderedDict()
    for g in range(len(hyps)):
        res[g], gts[g] = [" ".join(map(str, hyps[g]))], [" ".join(map(str, r)) for r in refs[g]]
    return SC.CiderD(df=tab).compute_score(gts, res)[1]


def host_values(hyp, ref, count, tab, cache_key=None):
    """(bleu_stats, lcs, cider float64 [G], rouge) of host_counts and host_cider."""
    stats, lcs, rl = host_counts(hyp, ref, count, cache_key)
    return stats, lcs, host_cider(hyp, ref, count, tab), rl


def lcs_shares(stats, lcs, count):
    """(share of the valid pairs with 0 < lcs < min(len_h, len_r), number of groups in which no reference is both precision-best -- the
    largest lcs -- and recall-best -- the largest lcs / len_r)."""
    G, R = lcs.shape[:2]
    inner = total = split = 0
    for g in range(G):
        n = clamp(count, g, R)
        len_h = int(stats[g, 4])
        for r in range(n):
            l, lr = int(lcs[g, r, 0]), int(lcs[g, r, 1])
            total += 1
            inner += 0 < l < min(len_h, lr)
        best_p = max(int(lcs[g, r, 0]) for r in range(n))
        rec = [lcs[g, r, 0] / float(lcs[g, r, 1]) if lcs[g, r, 1] else 0.0 for r in range(n)]
        best_r = max(rec)
        if best_p > 0 and not any(int(lcs[g, r, 0]) == best_p and rec[r] == best_r for r in range(n)):
            split += 1
    return inner / float(max(total, 1)), split


def conditions(shape, stats, lcs, count):
    """What a corpus of the kernel comparison must offer, on the host values alone."""
    G, R, T = shape
    share, split = lcs_shares(stats, lcs, count)
    return (share >= 0.5 or not (G >= 5 and T >= 21)) and (split >= 1 or G < 64)


_SEEDS = {}


def seed_of(shape):
    """The first of 0, 1, 2, ... whose corpus meets conditions(), chosen on the host values alone."""
    if shape not in _SEEDS:
        for seed in range(64):
            hyp, ref, count = make_corpus(*shape, seed)
            stats, lcs, _ = host_counts(hyp, ref, count, cache_key=(shape, seed))
            if conditions(shape, stats, lcs, count):
                _SEEDS[shape] = seed
                break
        else:
            raise AssertionError("no seed below 64 meets the conditions for %r" % (shape,))
    return _SEEDS[shape]


def hard_case(garbage=True):
    """G = 8, R = 3, T = 64; ref_count = [2, 2, 1, 2, 1, 1, 2, 2].  Words are 1000..1011 and 2000.. (group 4).
      group 0   an empty hypothesis (the row starts with 0)
      group 1   a hypothesis equal to its first reference at length 64: no 0 in either row; the second reference has 63 words
      group 2   a reversed copy of the reference (64 distinct-enough words: the LCS is far below the length)
      group 3   one word ten times against 64 copies of it (lcs 10 = len_h) and against 3 copies (lcs 3 = len_r)
      group 4   disjoint vocabularies: lcs 0
      group 5   `a b a` against `b a a`: lcs 2
      group 6   an empty valid reference next to a normal one
      group 7   63 words against a reference of 64 (the hypothesis with one word inserted) and one of 63
    garbage=True puts words behind every row's first 0 and into the invalid reference rows; garbage=False zeroes both."""
    G, R, T = 8, 3, 64
    rng = np.random.RandomState(7)
    hyp = np.zeros((G, T), dtype=np.int64)
    ref = np.zeros((G, R, T), dtype=np.int64)
    count = np.array([2, 2, 1, 2, 1, 1, 2, 2], dtype=np.int32)
    words = lambda n: rng.randint(1000, 1012, size=n)
    ref[0, 0, :9] = words(9)
    ref[0, 1, :5] = words(5)
    ref[1, 0] = words(64)
    hyp[1] = ref[1, 0]
    ref[1, 1, :63] = ref[1, 0, 1:]
    ref[2, 0] = words(64)
    hyp[2] = ref[2, 0, ::-1]
    hyp[3, :10] = 1003
    ref[3, 0] = 1003
    ref[3, 1, :3] = 1003
    hyp[4, :12] = words(12)
    ref[4, 0, :15] = 2000 + np.arange(15)
    hyp[5, :3] = [1000, 1001, 1000]
    ref[5, 0, :3] = [1001, 1000, 1000]
    hyp[6, :7] = words(7)
    ref[6, 1, :7] = hyp[6, :7]
    ref[6, 1, 3] = 1011 if hyp[6, 3] != 1011 else 1010
    hyp[7, :63] = words(63)
    ref[7, 0] = np.insert(hyp[7, :63], 30, 1005)
    ref[7, 1, :63] = hyp[7, :63]
    ref[7, 1, 10:20] = words(10)
    if garbage:
        junk = np.array([1001, 1009, 1000, 1004, 102, 1002, 1005] * 10)
        for rows in (hyp, ref.reshape(G * R, T)):
            for row in rows:
                z = np.flatnonzero(row == 0)
                if len(z):
                    row[z[0] + 1:] = junk[:T - int(z[0]) - 1]
        for g in range(G):
            for r in range(int(count[g]), R):
                ref[g, r] = hyp[g] if hyp[g, 0] else junk[:T]
    return hyp, ref, count


# ---- the CLI case: 7 images, one with a 70-word reference, one with 9 references ---------------------------------------------------------
CLI_WORDS = ["a", "man", "woman", "dog", "cat", "sits", "stands", "on", "the", "bench", "grass", "with", "red", "ball", "and", "looks"]


def write_cli_case(tmp_path, seed=3):
    """Writes dataset json and predictions; returns (src_file, predictions file, image ids in prediction order).  Images 0..6 of split
    'val' (image 2 has a 70-word reference, image 4 nine references), two more images of split 'train' that nothing may read."""
    import os
    rng = np.random.RandomState(seed)
    sent = lambda n: [CLI_WORDS[i] for i in rng.randint(0, len(CLI_WORDS), size=n)]
    images, preds = [], []
    for i in range(9):
        n_refs = 9 if i == 4 else 5
        sents = [sent(rng.randint(5, 12)) for _ in range(n_refs)]
        if i == 2:
            sents[1] = sent(70)
        images.append({"filename": "COCO_val2014_%012d.jpg" % (100 + i), "split": "val" if i < 7 else "train", "imgid": i,
                       "sentences": [{"tokens": s, "raw": " ".join(s)} for s in sents]})
        if i < 7:
            cap = list(sents[rng.randint(n_refs)][:10])
            for j in range(len(cap)):
                if rng.rand() < 0.3:
                    cap[j] = CLI_WORDS[rng.randint(len(CLI_WORDS))]
            text = " ".join(cap).capitalize() + " ."                     # upper case and punctuation for the tokenisation rule to remove
            preds.append({"image_id": 100 + i, "caption": text})
    order = rng.permutation(7)
    preds = [preds[i] for i in order]
    src, prd = os.path.join(str(tmp_path), "dataset.json"), os.path.join(str(tmp_path), "preds.json")
    json.dump({"images": images, "dataset": "coco"}, open(src, "w"))
    json.dump(preds, open(prd, "w"))
    return src, prd, [p["image_id"] for p in preds]
