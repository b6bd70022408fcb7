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
"""
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


class CiderD(object):
    """CIDEr-D with corpus document frequencies (df='corpus'); compute_score(gts, res) -> (mean score, per-key scores as np.ndarray)."""

    def __init__(self, n=4, sigma=6.0, df="corpus"):
        if df != "corpus":
            raise NotImplementedError("CiderD: only df='corpus' (document frequencies of the references of each call) is implemented")
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


def self_critical_reward(greedy_res, gt_ids, gen_result, batch_size, scorer=None):
    """scst_utils.py:36-63: CIDEr-D of the B samples and the B greedy captions (2B hypotheses), each against its own ground truth (so the 2B
    reference sets are the ground truths twice); reward[b, :] = score(sample_b) - score(greedy_b) repeated over the T columns.  Arguments are
    id tensors or arrays [B, T]; returns (reward [B, T] float64 ndarray, scores [2B])."""
    def host(x):
        return x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    greedy_res, gt_ids, gen_result = host(greedy_res), host(gt_ids), host(gen_result)
    B = batch_size
    res, gts = OrderedDict(), OrderedDict()
    gen_s = [array_to_str(r) for r in gen_result[:B].tolist()]
    gre_s = [array_to_str(r) for r in greedy_res[:B].tolist()]
    gt_s = [array_to_str(r) for r in gt_ids[:B].tolist()]
    for i in range(B):
        res[i], gts[i] = [gen_s[i]], [gt_s[i]]
    for i in range(B):
        res[B + i], gts[B + i] = [gre_s[i]], [gt_s[i]]
    _, scores = (scorer or _scorer).compute_score(gts, res)
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


def _refs_parts(refs, B):
    """refs -> (ids [B, R, T], count [B] or None): a CaptionRefs as it is, the [B, T] ground-truth ids as one reference per sample."""
    from .input_prep import CaptionRefs
    if isinstance(refs, CaptionRefs):
        return refs.ids[:B], refs.count[:B]
    return refs[:B].unsqueeze(1), None


def self_critical_reward_refs(greedy_res, refs, gen_result):
    """self_critical_reward against one OR several references per sample, on the host with CiderD: `refs` is the [B, T] ground-truth ids
    (then this is self_critical_reward itself) or a CaptionRefs (ids [B, R, T], count [B]: sample b is scored against the first count[b]
    rows).  Returns (reward [B, T] float64 ndarray, scores [2B]).  The oracle of self_critical_reward_device, and the host path of
    multi-reference training."""
    def host(x):
        return x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    from .input_prep import CaptionRefs
    B = len(gen_result)
    if not isinstance(refs, CaptionRefs):
        return self_critical_reward(greedy_res, refs, gen_result, B)
    greedy_res, gen_result, ids, count = host(greedy_res), host(gen_result), host(refs.ids), host(refs.count)
    R = ids.shape[1]
    gt_s = [[array_to_str(r) for r in ids[b, :min(max(int(count[b]), 1), R)].tolist()] for b in range(B)]
    res, gts = OrderedDict(), OrderedDict()
    for i in range(B):
        res[i], gts[i] = [array_to_str(gen_result[i].tolist())], gt_s[i]
    for i in range(B):
        res[B + i], gts[B + i] = [array_to_str(greedy_res[i].tolist())], gt_s[i]
    _, scores = _scorer.compute_score(gts, res)
    d = scores[:B] - scores[B:]
    return np.repeat(d[:, np.newaxis], gen_result.shape[1], 1), scores


def self_critical_reward_device(greedy_res, refs, gen_result, scores_out=None, workspace=None):
    """self_critical_reward_refs on the device (vlp_cider_d, csrc/reward.hip): id tensors [B, T] on the GPU, `refs` the [B, T] ground-truth
    ids or a CaptionRefs with ids [B, R, T] of the same T.  Returns (reward f32 [B, T] -- the [B] differences expanded over the columns --,
    scores f32 [2B]) as device tensors; scores_out (f32 [2B]) receives the scores when given; workspace: the caller's kernel scratch
    (_lib.cider_d_workspace_bytes(B, R, T, 2) bytes, uint8), else allocated per call.  No device -> host transfer, no synchronisation: two
    kernel launches on the current stream, capturable into a graph."""
    from . import _lib as K
    from .input_prep import CaptionRefs
    B, T = gen_result.shape
    if isinstance(refs, CaptionRefs):
        refs.check(B, T)
    ids, count = _refs_parts(refs, B)
    if tuple(greedy_res.shape) != (B, T) or ids.shape[0] != B or ids.shape[2] != T:
        raise RuntimeError("self_critical_reward_device: samples, greedy captions and references must share [B, T] = [%d, %d]" % (B, T))
    hyp = torch.cat([gen_result, greedy_res], 0)
    scores = scores_out if scores_out is not None else torch.empty(2 * B, dtype=torch.float32, device=hyp.device)
    diff = torch.empty(B, dtype=torch.float32, device=hyp.device)
    K.cider_d(hyp, ids, count, 2, scores, reward=diff, sigma=_scorer.sigma, workspace=workspace)
    return diff.unsqueeze(1).expand(B, T), scores
