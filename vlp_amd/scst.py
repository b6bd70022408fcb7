"""Self-critical sequence training on the host side: the CIDEr-D reward and the REINFORCE criterion (vlp/scst_utils.py).

The reference imports its scorer from the coco-caption submodule (`pycocoevalcap.cider.cider.Cider(df='corpus')`, scst_utils.py:10-12).
CiderD below is written from the published definition of CIDEr-D with corpus document frequencies:

  * tokens are the whitespace split of each string; n-grams for n = 1..4 are counted;
  * df(g) = number of reference SETS of this call whose union contains g; ref_len = log(number of reference sets);
  * every n-gram gets tf(g) * (ref_len - log(max(1, df(g)))); one L2 norm per n;
  * a sentence's "length" is its number of bigram occurrences (coco-caption's `if n == 1: length += term_freq` on a 0-based n);
  * per reference and n: sum_g min(h_g, r_g) * r_g / (|h| |r|) (a zero norm leaves the sum undivided), times the Gaussian length penalty
    exp(-(len_h - len_r)^2 / (2 sigma^2));
  * score = mean over n, averaged over the references, x 10.

Its parity with coco-caption's own file is not pinned by a test (that source is not available here).

The reward is computed where the reference computes it, on the host: one device -> host copy of the cleaned ids, numpy / python scoring of
2B short id strings, and the [B, T] reward back.  Caption cleaning and the criterion are vectorised torch ops.

self_critical_reward_device computes the same reward with the vlp_cider_d kernels (no host round trip), and together with
self_critical_reward_refs accepts several references per sample (input_prep.CaptionRefs: all captions of the image, which is how CIDEr is
defined; the reference's recipe scores against the one caption the loader drew).  CiderD stays the specification of both.

Document frequencies of a whole training set (coco-caption's `df=<file>` mode, the line scst_utils.py:17 reaches for): DocFreq is a table
n-gram -> number of IMAGES whose captions hold it, built once from the example list (DocFreq.from_examples, `python -m vlp_amd.cider_df`)
with every caption in the exact string form the reward sees.  CiderD(df=<DocFreq>) takes df from it and ref_len = log(n_docs); an n-gram the
table does not hold has df 0.  The three self_critical_reward* functions pass a `df=` table through (None = the call's own references, the
reference's behaviour); on the device the table is two resident arrays searched by the vlp_cider_d_df kernels.  DocFreq.from_token_lists
builds the table of an evaluation instead (vlp_amd/caption_metrics.py): word strings as they are, nothing appended.

A second metric: Bleu is sentence BLEU-1..4 (coco-caption's per-sentence values, closest reference length).  Every self_critical_reward*
function takes cider_weight / bleu_weight and scores a hypothesis with cider_weight * CIDEr-D + bleu_weight * BLEU-4 (CIDEr-D is 0..10 here,
BLEU-4 0..1); the defaults (1, 0) are the CIDEr-D reward, computed exactly as before.  On the device one more kernel, vlp_bleu4, scores
BLEU-4, mixes and baselines.
"""
import itertools
from collections import Counter, OrderedDict

import numpy as np
import torch
import torch.nn as nn


def _ngrams(words, n):
    counts = Counter()
    for k in range(1, n + 1):
        for i in range(len(words) - k + 1):
            counts[tuple(words[i:i + k])] += 1
    return counts


MAX_TOKEN_ID = 65534            # ids 0..65534 have keys; +1 keeps an absent position (0) apart from id 0
MAX_DOCS = 1 << 24              # float32(n_docs) is exact on the device


def pack_ngram(ids):
    """The uint64 key of an n-gram of 1..4 ids, each in 0..65534: ((t0+1) << 48) | ((t1+1) << 32) | ((t2+1) << 16) | (t3+1), absent positions
    contributing 0.  Distinct n-grams have distinct keys, key 0 never occurs.  A python int."""
    if not 1 <= len(ids) <= 4:
        raise ValueError("pack_ngram: an n-gram has 1..4 ids")
    key = 0
    for j, t in enumerate(ids):
        if not 0 <= t <= MAX_TOKEN_ID:
            raise ValueError("pack_ngram: id %d is outside 0..%d" % (t, MAX_TOKEN_ID))
        key |= (int(t) + 1) << (48 - 16 * j)
    return key


class DocFreq(object):
    """Document frequencies of a training set: keys uint64 [N] strictly ascending (pack_ngram), vals int32 [N] (1 <= df <= n_docs), n_docs the
    number of documents (images).  max_len_b / sep_id record the caption format the table was built for (None when unknown)."""

    def __init__(self, keys, vals, n_docs, max_len_b=None, sep_id=None):
        keys, vals = np.ascontiguousarray(keys), np.ascontiguousarray(vals)
        if keys.dtype != np.uint64 or vals.dtype != np.int32 or keys.ndim != 1 or keys.shape != vals.shape:
            raise ValueError("DocFreq: keys must be uint64 [N] and vals int32 [N]")
        n_docs = int(n_docs)
        if not 1 <= n_docs <= MAX_DOCS:
            raise ValueError("DocFreq: n_docs %d is outside 1..2**24 (float32(n_docs) must be exact on the device)" % n_docs)
        if len(keys):
            if keys[0] == 0:
                raise ValueError("DocFreq: key 0 is no n-gram")
            if (keys[1:] == keys[:-1]).any():
                raise ValueError("DocFreq: duplicate keys")
            if (keys[1:] < keys[:-1]).any():
                raise ValueError("DocFreq: keys are not sorted (ascending as unsigned 64-bit integers)")
            if int(vals.min()) < 1:
                raise ValueError("DocFreq: a document frequency below 1")
            if int(vals.max()) > n_docs:
                raise ValueError("DocFreq: a document frequency above n_docs = %d" % n_docs)
        self.keys, self.vals, self.n_docs = keys, vals, n_docs
        self.max_len_b = None if max_len_b is None else int(max_len_b)
        self.sep_id = None if sep_id is None else int(sep_id)
        self._resident, self._scorer = {}, None

    def __len__(self):
        return len(self.keys)

    @classmethod
    def from_examples(cls, examples, max_len_b, sep_id, chunk=1 << 16):
        """examples: the loader's list of (image id, [caption token ids], ...).  A document is one image: ALL its captions in the list, each
        as the reference row BatchPrefetcher builds -- the first max_len_b tokens, [SEP], then 0 -- read like array_to_str reads it (up to and
        including the first 0, so [SEP] and the trailing 0 are tokens of n-grams; a caption of max_len_b or more tokens has no 0).
        df(g) = the number of images whose strings hold g.  Vectorised numpy per chunk of `chunk` images; no python loop per n-gram."""
        max_len_b, sep_id = int(max_len_b), int(sep_id)
        T = max_len_b + 1
        if max_len_b < 0 or not 0 <= sep_id <= MAX_TOKEN_ID:
            raise ValueError("DocFreq: needs max_len_b >= 0 and sep_id in 0..%d" % MAX_TOKEN_ID)
        index = {}
        img = np.fromiter((index.setdefault(ex[0], len(index)) for ex in examples), dtype=np.int64, count=len(examples))
        if not index:
            raise ValueError("DocFreq: no examples")
        order = np.argsort(img, kind="stable")
        img_sorted = img[order]
        cols = np.arange(T)
        parts_k, parts_v = [], []
        lo = 0
        while lo < len(order):
            hi = int(np.searchsorted(img_sorted, img_sorted[lo] + chunk, side="left"))
            caps = [examples[i][1][:max_len_b] for i in order[lo:hi]]
            lens = np.fromiter((len(c) for c in caps), dtype=np.int64, count=len(caps))
            flat = np.fromiter(itertools.chain.from_iterable(caps), dtype=np.int64, count=int(lens.sum()))
            if len(flat) and (flat.min() < 0 or flat.max() > MAX_TOKEN_ID):
                raise ValueError("DocFreq: a caption token id is outside 0..%d" % MAX_TOKEN_ID)
            rows = np.zeros((len(caps), T + 3), dtype=np.uint64)                      # id + 1 (so the row's padding 0 is 1); 0 = past the row
            text = rows[:, :T]
            text[:] = 1
            text[cols[None, :] < lens[:, None]] = (flat + 1).astype(np.uint64)
            text[np.arange(len(caps)), lens] = sep_id + 1
            is0 = text == 1
            slen = np.where(is0.any(1), is0.argmax(1) + 1, T)                        # up to and including the first 0
            docs = img_sorted[lo:hi]
            key = np.zeros((len(caps), T), dtype=np.uint64)
            pairs_k, pairs_d = [], []
            for k in range(4):
                key = key | (rows[:, k:k + T] << np.uint64(48 - 16 * k))
                ok = cols[None, :] + (k + 1) <= slen[:, None]
                pairs_k.append(key[ok])
                pairs_d.append(np.broadcast_to(docs[:, None], ok.shape)[ok])
            pk, pd = np.concatenate(pairs_k), np.concatenate(pairs_d)
            o = np.lexsort((pk, pd))
            pk, pd = pk[o], pd[o]
            new = np.ones(len(pk), dtype=bool)
            new[1:] = (pk[1:] != pk[:-1]) | (pd[1:] != pd[:-1])                       # an n-gram counts once per image
            k_u, k_c = np.unique(pk[new], return_counts=True)
            parts_k.append(k_u)
            parts_v.append(k_c)
            lo = hi
        keys, inv = np.unique(np.concatenate(parts_k), return_inverse=True)
        vals = np.bincount(inv, weights=np.concatenate(parts_v), minlength=len(keys)).astype(np.int32)
        return cls(keys.astype(np.uint64), vals, len(index), max_len_b, sep_id)

    @classmethod
    def from_token_lists(cls, docs, chunk=1 << 14):
        """The table of an evaluation (vlp_amd.caption_metrics): docs is one entry per image, each a list of WORD STRINGS -- lists of word ids
        in 1..65534, the empty list included; nothing is appended (from_examples adds [SEP] and the 0 of the reward's strings; a word string
        has neither, so no key is ever formed from 0).  df(g) = the number of images one of whose strings holds g; n_docs = len(docs).
        Vectorised numpy per chunk of `chunk` images."""
        n_docs = len(docs)
        if not n_docs:
            raise ValueError("DocFreq: no documents")
        parts_k, parts_v = [], []
        for lo in range(0, n_docs, chunk):
            caps, owner = [], []
            for d in range(lo, min(lo + chunk, n_docs)):
                for c in docs[d]:
                    caps.append(c)
                    owner.append(d)
            lens = np.fromiter((len(c) for c in caps), dtype=np.int64, count=len(caps))
            if not len(caps) or not int(lens.sum()):
                continue
            flat = np.fromiter(itertools.chain.from_iterable(caps), dtype=np.int64, count=int(lens.sum()))
            if flat.min() < 1 or flat.max() > MAX_TOKEN_ID:
                raise ValueError("DocFreq: a word id is outside 1..%d" % MAX_TOKEN_ID)
            T = int(lens.max())
            cols = np.arange(T)
            rows = np.zeros((len(caps), T + 3), dtype=np.uint64)                      # id + 1; 0 = past the string
            rows[:, :T][cols[None, :] < lens[:, None]] = (flat + 1).astype(np.uint64)
            owner = np.asarray(owner, dtype=np.int64)
            key = np.zeros((len(caps), T), dtype=np.uint64)
            pairs_k, pairs_d = [], []
            for k in range(4):
                key = key | (rows[:, k:k + T] << np.uint64(48 - 16 * k))
                ok = cols[None, :] + (k + 1) <= lens[:, None]
                pairs_k.append(key[ok])
                pairs_d.append(np.broadcast_to(owner[:, None], ok.shape)[ok])
            pk, pd = np.concatenate(pairs_k), np.concatenate(pairs_d)
            o = np.lexsort((pk, pd))
            pk, pd = pk[o], pd[o]
            new = np.ones(len(pk), dtype=bool)
            new[1:] = (pk[1:] != pk[:-1]) | (pd[1:] != pd[:-1])                       # an n-gram counts once per image
            k_u, k_c = np.unique(pk[new], return_counts=True)
            parts_k.append(k_u)
            parts_v.append(k_c)
        if not parts_k:
            return cls(np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.int32), n_docs)
        keys, inv = np.unique(np.concatenate(parts_k), return_inverse=True)
        vals = np.bincount(inv, weights=np.concatenate(parts_v), minlength=len(keys)).astype(np.int32)
        return cls(keys.astype(np.uint64), vals, n_docs)

    def save(self, path):
        """An .npz of keys, vals, n_docs, max_len_b and sep_id (-1 = unknown), nothing else."""
        with open(path, "wb") as f:
            np.savez(f, keys=self.keys, vals=self.vals, n_docs=np.int64(self.n_docs),
                     max_len_b=np.int64(-1 if self.max_len_b is None else self.max_len_b), sep_id=np.int64(-1 if self.sep_id is None else self.sep_id))

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as z:
            if sorted(z.files) != ["keys", "max_len_b", "n_docs", "sep_id", "vals"]:
                raise ValueError("DocFreq.load: %s is not a table written by DocFreq.save (fields %s)" % (path, sorted(z.files)))
            m, s = int(z["max_len_b"]), int(z["sep_id"])
            return cls(z["keys"], z["vals"], int(z["n_docs"]), None if m < 0 else m, None if s < 0 else s)

    def get(self, ngram, default=0.0):
        """df of an n-gram given as a tuple of ids or of id strings (CiderD's words); `default` when the table does not hold it -- an id
        outside 0..65534, or a word that is no id, has no key and is a miss."""
        try:
            key = pack_ngram([int(w) for w in ngram])
        except ValueError:
            return default
        i = int(np.searchsorted(self.keys, np.uint64(key)))
        return int(self.vals[i]) if i < len(self.keys) and int(self.keys[i]) == key else default

    def to(self, device):
        """(keys, vals) on `device`: keys as an int64 tensor holding the uint64 keys bit for bit, vals int32.  Uploaded once per device and
        kept (the device reward reads the same two arrays every step)."""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if device not in self._resident:
            self._resident[device] = (torch.from_numpy(self.keys.view(np.int64)).to(device), torch.from_numpy(self.vals).to(device))
        return self._resident[device]


class CiderD(object):
    """CIDEr-D; compute_score(gts, res) -> (mean score, per-key scores as np.ndarray).  df='corpus': document frequencies of the references of
    each call, ref_len = log(number of reference sets).  df=<DocFreq>: document frequencies of that table (0 for an n-gram it does not hold),
    ref_len = log(table.n_docs); everything else is the same."""

    def __init__(self, n=4, sigma=6.0, df="corpus"):
        if not isinstance(df, DocFreq) and not (isinstance(df, str) and df == "corpus"):
            raise NotImplementedError("CiderD: only df='corpus' (document frequencies of the references of each call) or a DocFreq table is "
                                      "implemented")
        self.n, self.sigma, self.df = n, float(sigma), df

    def _vec(self, counts, df, ref_len):
        vec = [dict() for _ in range(self.n)]
        norm = [0.0] * self.n
        length = 0
        for g, tf in counts.items():
            k = len(g) - 1
            val = float(tf) * (ref_len - np.log(max(1.0, df.get(g, 0.0))))
            vec[k][g] = val
            norm[k] += val * val
            if k == 1:
                length += tf
        return vec, [np.sqrt(x) for x in norm], length

    def _sim(self, vh, vr, nh, nr, lh, lr):
        delta = float(lh - lr)
        val = np.zeros(self.n)
        for k in range(self.n):
            for g, hv in vh[k].items():
                rv = vr[k].get(g, 0.0)
                val[k] += min(hv, rv) * rv
            if nh[k] != 0 and nr[k] != 0:
                val[k] /= nh[k] * nr[k]
            val[k] *= np.e ** (-(delta ** 2) / (2 * self.sigma ** 2))
        return val

    def compute_score(self, gts, res):
        assert gts.keys() == res.keys()
        keys = list(gts.keys())
        crefs, ctest = [], []
        for k in keys:
            hypo, ref = res[k], gts[k]
            assert type(hypo) is list and len(hypo) == 1
            assert type(ref) is list and len(ref) > 0
            ctest.append(_ngrams(hypo[0].split(), self.n))
            crefs.append([_ngrams(r.split(), self.n) for r in ref])
        if isinstance(self.df, DocFreq):
            df, ref_len = self.df, np.log(float(self.df.n_docs))
        else:
            df = Counter()
            for refs in crefs:
                for g in set(g for r in refs for g in r):
                    df[g] += 1
            ref_len = np.log(float(len(crefs)))
        scores = []
        for test, refs in zip(ctest, crefs):
            vh, nh, lh = self._vec(test, df, ref_len)
            acc = np.zeros(self.n)
            for r in refs:
                vr, nr, lr = self._vec(r, df, ref_len)
                acc += self._sim(vh, vr, nh, nr, lh, lr)
            scores.append(np.mean(acc) / len(refs) * 10.0)
        scores = np.array(scores)
        return np.mean(scores), scores


class Bleu(object):
    """Sentence BLEU-1..4 (coco-caption's BLEU scorer with option='closest', its per-sentence values); compute_score(gts, res) -> (mean BLEU-4,
    scores float64 [4, N]).  Same dictionaries of strings as CiderD.compute_score; tokens are the whitespace split (array_to_str's strings: the
    terminating 0 is a token).  Per hypothesis h with references r_1..r_m, in fp64:
      * reflen = the reference length closest to len_h, the shorter on a tie: the minimum over (|len_r - len_h|, len_r);
      * guess_k = max(0, len_h - k + 1); correct_k = sum over the distinct k-grams g of h of min(count_h(g), max_j count_{r_j}(g));
      * p_0 = 1, p_k = p_{k-1} * (correct_k + TINY) / (guess_k + SMALL), bleu_k = p_k ** (1 / k);
      * ratio = (len_h + TINY) / (reflen + SMALL); ratio < 1 multiplies every bleu_k by exp(1 - 1 / ratio).
    The specification of the vlp_bleu4 kernel (csrc/reward.hip); sentence_stats gives the integers a score is made of."""
    TINY, SMALL = 1e-15, 1e-9

    def __init__(self, n=4):
        self.n = n

    def sentence_stats(self, hypo, refs):
        """(correct_1..n, len_h, reflen) of one hypothesis string against its reference strings, as python ints."""
        h = hypo.split()
        rs = [r.split() for r in refs]
        best = Counter()
        for r in rs:
            for g, c in _ngrams(r, self.n).items():
                if c > best[g]:
                    best[g] = c
        correct = [0] * self.n
        for g, c in _ngrams(h, self.n).items():
            correct[len(g) - 1] += min(c, best.get(g, 0))
        reflen = min((abs(len(r) - len(h)), len(r)) for r in rs)[1]
        return correct, len(h), reflen

    def sentence_scores(self, correct, len_h, reflen):
        """bleu_1..n (float64 [n]) from sentence_stats' integers."""
        out = np.empty(self.n)
        p = 1.0
        for k in range(1, self.n + 1):
            p = p * (correct[k - 1] + self.TINY) / (max(0, len_h - k + 1) + self.SMALL)
            out[k - 1] = p ** (1.0 / k)
        ratio = (len_h + self.TINY) / (reflen + self.SMALL)
        if ratio < 1:
            out *= np.exp(1 - 1 / ratio)
        return out

    def compute_score(self, gts, res):
        assert gts.keys() == res.keys()
        keys = list(gts.keys())
        scores = np.empty((self.n, len(keys)))
        for i, k in enumerate(keys):
            hypo, ref = res[k], gts[k]
            assert type(hypo) is list and len(hypo) == 1
            assert type(ref) is list and len(ref) > 0
            scores[:, i] = self.sentence_scores(*self.sentence_stats(hypo[0], ref))
        return (float(np.mean(scores[-1])) if keys else 0.0), scores


def array_to_str(arr):
    """scst_utils.py:27-33: the ids up to and including the first 0, space separated."""
    out = []
    for x in arr:
        out.append(str(x))
        if x == 0:
            break
    return " ".join(out)


def clean_captions(raw, eos_id, pad_id=0):
    """run_img2txt_dist.py:491-499 / 509-515 without the per-sample loop: the tokens before the first [SEP] or [PAD] are kept, a [SEP] that
    ends the caption is kept, everything after becomes 0 (a [PAD] ends the caption without being kept -- it is 0 already)."""
    stop = (raw == eos_id) | (raw == pad_id)
    n_stop = stop.to(torch.int32).cumsum(dim=1)
    keep = (n_stop == 0) | (stop & (n_stop == 1))
    return torch.where(keep, raw, torch.zeros_like(raw))


_scorer = CiderD(df="corpus")


def _table_scorer(df):
    """The scorer of a `df=` argument: None -> the module's df='corpus' scorer, a DocFreq -> its CiderD (made once per table)."""
    if df is None:
        return _scorer
    if not isinstance(df, DocFreq):
        raise TypeError("df must be None or a vlp_amd.scst.DocFreq")
    if df._scorer is None:
        df._scorer = CiderD(df=df)
    return df._scorer


_bleu = Bleu()


def check_reward_weights(cider_weight, bleu_weight):
    """(cider_weight, bleu_weight) of the mixed reward cider_weight * CIDEr-D + bleu_weight * BLEU-4 as floats; negative or non-finite weights,
    and both zero, raise ValueError."""
    cw, bw = float(cider_weight), float(bleu_weight)
    if not (np.isfinite(cw) and np.isfinite(bw)) or cw < 0 or bw < 0:
        raise ValueError("the reward weights must be finite and not negative (cider_weight %r, bleu_weight %r)" % (cider_weight, bleu_weight))
    if cw == 0 and bw == 0:
        raise ValueError("the reward weights are both zero: there is no reward")
    return cw, bw


def _mixed_scores(gts, res, scorer, cider_weight, bleu_weight):
    """cider_weight * CIDEr-D + bleu_weight * BLEU-4 per key (CIDEr-D here is 0..10, BLEU-4 0..1).  (1, 0) is the scorer's own array; a scorer
    whose weight is 0 is not called."""
    cw, bw = check_reward_weights(cider_weight, bleu_weight)
    if cw == 1 and bw == 0:
        return scorer.compute_score(gts, res)[1]
    scores = None
    if cw > 0:
        scores = cw * np.asarray(scorer.compute_score(gts, res)[1], dtype=np.float64)
    if bw > 0:
        b = bw * _bleu.compute_score(gts, res)[1][3]
        scores = b if scores is None else scores + b
    return scores


def _host(x):
    return x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


def self_critical_reward(greedy_res, gt_ids, gen_result, batch_size, scorer=None, df=None, cider_weight=1.0, bleu_weight=0.0):
    """scst_utils.py:36-63: CIDEr-D of the B samples and the B greedy captions (2B hypotheses), each against its own ground truth (so the 2B
    reference sets are the ground truths twice); reward[b, :] = score(sample_b) - score(greedy_b) repeated over the T columns.  Arguments are
    id tensors or arrays [B, T]; returns (reward [B, T] float64 ndarray, scores [2B]).  df: a DocFreq whose document frequencies replace the
    call's own (ignored when a scorer is given).  cider_weight / bleu_weight: the score of a hypothesis is cider_weight * CIDEr-D +
    bleu_weight * sentence BLEU-4 (Bleu); (1, 0) is the CIDEr-D reward as it always was."""
    greedy_res, gt_ids, gen_result = _host(greedy_res), _host(gt_ids), _host(gen_result)
    B = batch_size
    res, gts = OrderedDict(), OrderedDict()
    gen_s = [array_to_str(r) for r in gen_result[:B].tolist()]
    gre_s = [array_to_str(r) for r in greedy_res[:B].tolist()]
    gt_s = [array_to_str(r) for r in gt_ids[:B].tolist()]
    for i in range(B):
        res[i], gts[i] = [gen_s[i]], [gt_s[i]]
    for i in range(B):
        res[B + i], gts[B + i] = [gre_s[i]], [gt_s[i]]
    scores = _mixed_scores(gts, res, scorer or _table_scorer(df), cider_weight, bleu_weight)
    d = scores[:B] - scores[B:]
    return np.repeat(d[:, np.newaxis], gen_result.shape[1], 1), scores


class RewardCriterion(nn.Module):
    """scst_utils.py:66-78: -sum(logp * reward * mask) / sum(mask) with mask = [1, (seq > 0)[:, :-1]] -- the position right after the first 0
    still counts."""

    def forward(self, input, seq, reward):
        input = input.contiguous().view(-1)
        reward = reward.contiguous().view(-1).to(input.dtype)
        mask = (seq > 0).to(input.dtype)
        mask = torch.cat([torch.ones_like(mask[:, :1]), mask[:, :-1]], 1).contiguous().view(-1)
        return torch.sum(-input * reward * mask) / torch.sum(mask)


def reward_mask(seq, dtype=torch.float32):
    """RewardCriterion's mask [B, T]: [1, (seq > 0)[:, :-1]] -- every position up to and including the one right after the first 0."""
    mask = (seq > 0).to(dtype)
    return torch.cat([torch.ones_like(mask[:, :1]), mask[:, :-1]], 1)


def policy_loss(logp, seq, reward, entropy=None, entropy_weight=0.0, crit=None):
    """The SCST loss with an entropy bonus (--scst_entropy_weight): RewardCriterion(logp, seq, reward) - entropy_weight * sum(H * mask) /
    sum(mask) over RewardCriterion's mask, H = `entropy` [B, T], the sampled policy's entropy at every position.  Returns (loss, masked mean
    entropy or None).  entropy_weight 0 returns the criterion's own value (the mean entropy, detached, only when `entropy` is given)."""
    w = float(entropy_weight)
    if not (np.isfinite(w) and w >= 0):
        raise ValueError("the entropy weight must be finite and not negative (got %r)" % (entropy_weight,))
    loss = (crit if crit is not None else RewardCriterion())(logp, seq, reward)
    if entropy is None:
        if w > 0:
            raise ValueError("an entropy weight of %r needs the policy's entropy" % w)
        return loss, None
    mask = reward_mask(seq, entropy.dtype)
    mean_h = torch.sum(entropy * mask) / torch.sum(mask)
    if w == 0:
        return loss, mean_h.detach()
    return loss - w * mean_h, mean_h.detach()


def _refs_parts(refs, B):
    """refs -> (ids [B, R, T], count [B] or None): a CaptionRefs as it is, the [B, T] ground-truth ids as one reference per sample."""
    from .input_prep import CaptionRefs
    if isinstance(refs, CaptionRefs):
        return refs.ids[:B], refs.count[:B]
    return refs[:B].unsqueeze(1), None


def _ref_strings(refs, B):
    """The reference strings of B samples, a list per sample: of a CaptionRefs the first count[b] rows (clamped to 1..R) of sample b, of [B, T]
    ground-truth ids the one row."""
    from .input_prep import CaptionRefs
    if not isinstance(refs, CaptionRefs):
        return [[array_to_str(r)] for r in _host(refs)[:B].tolist()]
    ids, count = _host(refs.ids), _host(refs.count)
    R = ids.shape[1]
    return [[array_to_str(r) for r in ids[b, :min(max(int(count[b]), 1), R)].tolist()] for b in range(B)]


def _device_reward(hyp, ids, count, mult, loo, weights, scores_out, workspace, df):
    """The launch sequence of the two device rewards on hyp [mult*B, T] against ids [B, R, T] / count: the CIDEr-D entry (its df form with a
    DocFreq; its multi form with loo; only with a CIDEr-D weight > 0), then for weights other than (1, 0) vlp_bleu4, which mixes the scores
    and writes the reward.  loo: the leave-one-out reward [mult*B], else scores[:B] - scores[B:] (mult == 2).  Returns (reward, scores)."""
    from . import _lib as K
    cw, bw = weights
    n = hyp.shape[0]
    nr = n if loo else n // mult
    scores = scores_out if scores_out is not None else torch.empty(n, dtype=torch.float32, device=hyp.device)
    mix = not (cw == 1 and bw == 0)
    out = torch.empty(nr + n if mix else nr, dtype=torch.float32, device=hyp.device)      # the reward, then the BLEU-4 of the hypotheses
    reward = out[:nr]
    if cw > 0:
        first = None if mix else reward                 # mixed: the reward is the vlp_bleu4 launch's
        if df is None:
            (K.cider_d_multi if loo else K.cider_d)(hyp, ids, count, mult, scores, reward=first, sigma=_scorer.sigma, workspace=workspace)
        else:
            keys, vals = df.to(hyp.device)
            (K.cider_d_multi_df if loo else K.cider_d_df)(hyp, ids, count, mult, scores, keys, vals, df.n_docs, reward=first,
                                                          sigma=_table_scorer(df).sigma, workspace=workspace)
    if mix:
        K.bleu4(hyp, ids, count, mult, out[nr:], base=scores if cw > 0 else None, w_base=cw, w_bleu=bw, mixed=scores, reward=reward, loo=loo)
    return reward, scores


def self_critical_reward_refs(greedy_res, refs, gen_result, df=None, cider_weight=1.0, bleu_weight=0.0):
    """self_critical_reward against one OR several references per sample, on the host with CiderD: `refs` is the [B, T] ground-truth ids
    (then this is self_critical_reward itself) or a CaptionRefs (ids [B, R, T], count [B]: sample b is scored against the first count[b]
    rows).  Returns (reward [B, T] float64 ndarray, scores [2B]).  The oracle of self_critical_reward_device, and the host path of
    multi-reference training.  df: a DocFreq whose document frequencies replace the call's own.  cider_weight / bleu_weight: as in
    self_critical_reward."""
    from .input_prep import CaptionRefs
    B = len(gen_result)
    if not isinstance(refs, CaptionRefs):
        return self_critical_reward(greedy_res, refs, gen_result, B, df=df, cider_weight=cider_weight, bleu_weight=bleu_weight)
    greedy_res, gen_result, gt_s = _host(greedy_res), _host(gen_result), _ref_strings(refs, B)
    res, gts = OrderedDict(), OrderedDict()
    for i in range(B):
        res[i], gts[i] = [array_to_str(gen_result[i].tolist())], gt_s[i]
    for i in range(B):
        res[B + i], gts[B + i] = [array_to_str(greedy_res[i].tolist())], gt_s[i]
    scores = _mixed_scores(gts, res, _table_scorer(df), cider_weight, bleu_weight)
    d = scores[:B] - scores[B:]
    return np.repeat(d[:, np.newaxis], gen_result.shape[1], 1), scores


def self_critical_reward_device(greedy_res, refs, gen_result, scores_out=None, workspace=None, df=None, cider_weight=1.0, bleu_weight=0.0):
    """self_critical_reward_refs on the device (vlp_cider_d, csrc/reward.hip): id tensors [B, T] on the GPU, `refs` the [B, T] ground-truth
    ids or a CaptionRefs with ids [B, R, T] of the same T.  Returns (reward f32 [B, T] -- the [B] differences expanded over the columns --,
    scores f32 [2B]) as device tensors; scores_out (f32 [2B]) receives the scores when given; workspace: the caller's kernel scratch
    (_lib.cider_d_workspace_bytes(B, R, T, 2) bytes, uint8), else allocated per call.  No device -> host transfer, no synchronisation: two
    kernel launches on the current stream, capturable into a graph.
    df: a DocFreq -- the vlp_cider_d_df kernels score with its document frequencies (workspace: _lib.cider_d_df_workspace_bytes).  The table
    is uploaded by the first call that uses it on a device (DocFreq.to) and stays resident; make that call before a graph capture.
    cider_weight / bleu_weight other than (1, 0): the CIDEr-D launches (only with cider_weight > 0) write their scores, then one vlp_bleu4
    launch scores sentence BLEU-4, replaces the scores by cider_weight * CIDEr-D + bleu_weight * BLEU-4 and writes the reward of those
    mixed scores: the returned scores are the mixed ones; df applies to the CIDEr-D part only.  Still no host work and capturable."""
    weights = check_reward_weights(cider_weight, bleu_weight)
    from .input_prep import CaptionRefs
    B, T = gen_result.shape
    if isinstance(refs, CaptionRefs):
        refs.check(B, T)
    ids, count = _refs_parts(refs, B)
    if tuple(greedy_res.shape) != (B, T) or ids.shape[0] != B or ids.shape[2] != T:
        raise RuntimeError("self_critical_reward_device: samples, greedy captions and references must share [B, T] = [%d, %d]" % (B, T))
    diff, scores = _device_reward(torch.cat([gen_result, greedy_res], 0), ids, count, 2, False, weights, scores_out, workspace, df)
    return diff.unsqueeze(1).expand(B, T), scores


# ------------------------------------------------------------------------------------------------------------------------------------------
# K samples per image with a leave-one-out baseline (--scst_samples K).  A deliberate departure from the reference's estimator (one sample
# against a greedy decode): every sample is baselined by the mean score of the image's other K - 1 samples, so no greedy decode is needed.
# Rows are sample-major: row k*B + b is sample k of image b (the reward kernels' `i % G`).
# ------------------------------------------------------------------------------------------------------------------------------------------
MAX_SAMPLES = 16


def _check_samples(n_rows, n_samples):
    n_samples = int(n_samples)
    if not 2 <= n_samples <= MAX_SAMPLES:
        raise ValueError("the leave-one-out reward needs 2..%d samples per image (got %d)" % (MAX_SAMPLES, n_samples))
    if n_rows % n_samples:
        raise ValueError("%d rows are not %d samples of every image" % (n_rows, n_samples))
    return n_samples, n_rows // n_samples


def self_critical_reward_group(gen_result, refs, n_samples, df=None, cider_weight=1.0, bleu_weight=0.0):
    """The leave-one-out reward of K = n_samples samples per image, on the host with CiderD in fp64: the specification of
    self_critical_reward_group_device and the `--scst_reward host` path.  gen_result [K*B, T] ids, row k*B + b = sample k of image b; refs
    the [B, T] ground-truth ids or a CaptionRefs (image b is scored against its first count[b] rows).  The K*B hypotheses each list their
    image's references, which is what coco-caption's Cider(df='corpus') sees: df counts every image K times and ref_len = log(K*B); a
    DocFreq `df` replaces both, without a K anywhere.  reward[k*B + b] = s[k*B + b] - (sum of s[j*B + b] over j != k, ascending j) / (K - 1).
    Returns (reward [K*B, T] float64 ndarray -- the [K*B] rewards repeated over the columns --, scores [K*B]).  cider_weight / bleu_weight:
    s is cider_weight * CIDEr-D + bleu_weight * sentence BLEU-4, as in self_critical_reward."""
    gen_result = _host(gen_result)
    K, B = _check_samples(len(gen_result), n_samples)
    gt_s = _ref_strings(refs, B)
    res, gts = OrderedDict(), OrderedDict()
    for i, row in enumerate(gen_result.tolist()):
        res[i], gts[i] = [array_to_str(row)], gt_s[i % B]
    scores = _mixed_scores(gts, res, _table_scorer(df), cider_weight, bleu_weight)
    s = np.asarray(scores, dtype=np.float64).reshape(K, B)
    reward = np.empty_like(s)
    for k in range(K):
        others = np.zeros(B)
        for j in range(K):
            if j != k:
                others = others + s[j]
        reward[k] = s[k] - others / (K - 1)
    return np.repeat(reward.reshape(-1)[:, np.newaxis], gen_result.shape[1], 1), scores


def self_critical_reward_group_device(gen_result, refs, n_samples, scores_out=None, workspace=None, df=None, cider_weight=1.0, bleu_weight=0.0):
    """self_critical_reward_group on the device (vlp_cider_d_multi / vlp_cider_d_multi_df, csrc/reward.hip): gen_result int64 [K*B, T] on the
    GPU, refs the [B, T] ground-truth ids or a CaptionRefs of the same T.  Returns (reward f32 [K*B, T] -- expanded over the columns --,
    scores f32 [K*B]) as device tensors; scores_out (f32 [K*B]) receives the scores when given; workspace: the caller's kernel scratch
    (_lib.cider_d_multi_workspace_bytes(B, R, T, K) or ..._multi_df_... bytes, uint8), else allocated per call.  No device -> host transfer,
    no synchronisation: two launches on the current stream, capturable.  df, cider_weight, bleu_weight: as in self_critical_reward_device
    (the vlp_bleu4 launch then writes the leave-one-out reward of the mixed scores)."""
    weights = check_reward_weights(cider_weight, bleu_weight)
    from .input_prep import CaptionRefs
    KB, T = gen_result.shape
    K, B = _check_samples(KB, n_samples)
    if isinstance(refs, CaptionRefs):
        refs.check(B, T)
    ids, count = _refs_parts(refs, B)
    if ids.shape[0] != B or ids.shape[2] != T:
        raise RuntimeError("self_critical_reward_group_device: %d samples of %d images need references [%d, R, %d]" % (K, B, B, T))
    reward, scores = _device_reward(gen_result, ids, count, K, True, weights, scores_out, workspace, df)
    return reward.unsqueeze(1).expand(KB, T), scores
