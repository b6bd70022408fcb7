"""Caption metrics without Java: corpus BLEU-1..4, ROUGE-L and CIDEr of a set of predicted captions, on the host or on the device.

The reference scores its predictions with the coco-caption package (lang_utils.language_eval -> COCOEvalCap), which runs Java for the PTB
tokenizer, METEOR and SPICE.  BLEU, ROUGE-L and the metric coco-caption prints as "CIDEr" are plain counting; they are written here from the
published definitions, because coco-caption itself is not available to this project -- parity with its files is not pinned by a test:

  * Bleu_1..4   coco-caption's corpus value with option='closest': corpus_bleu() over vlp_amd.scst.Bleu.sentence_stats' integers;
  * ROUGE_L     Rouge below: the LCS-based F-measure with beta = 1.2, precision and recall each maximised over the references, mean over
                the images;
  * CIDEr       CIDEr-D arithmetic (clipped products, Gaussian length penalty with sigma 6) with df over the reference sets of the
                evaluated images: vlp_amd.scst.CiderD(df=<DocFreq.from_token_lists of those sets>), mean over the images.

A WORD STRING is a list of word ids in 1..65534, the empty list included.  In a padded row it is the ids before the first 0, or all T ids
without one: the 0 is padding and never a token (words_of_row).  The SCST reward's strings (scst.array_to_str) include that 0.

CaptionMetrics.score(refs, hyps, on="host" | "device") takes words and returns the six corpus values with per-image arrays.  The device path
(vlp_caption_eval, csrc/caption_eval.hip) produces the BLEU integers, the LCS lengths and fp32 CIDEr scores; the corpus values are reduced on
the host in fp64 from the integers, so Bleu_1..4 and ROUGE_L equal the host path exactly and only CIDEr carries fp32 error.  An image with a
string of more than 64 words or more than 8 references does not fit the kernel and is scored by the host classes against the same table.

Departure from the Java pipeline: COCOEvalCap runs PTBTokenizer over the raw captions of both sides.  Given the same tokens the three metrics
are coco-caption's; the tokenisation here is tokenize_caption's rule (python -m vlp_amd.eval_captions), so figures can differ from the Java
pipeline's.  Nobody has measured by how much.  METEOR and SPICE are out of scope.
"""
import numpy as np

from .scst import Bleu, CiderD, DocFreq, MAX_TOKEN_ID

MAX_T, MAX_R, MAX_G = 64, 8, 1024          # what vlp_caption_eval accepts
# coco-caption's PTBTokenizer punctuation list
PUNCTUATIONS = frozenset(["''", "'", "``", "`", "-LRB-", "-RRB-", "-LCB-", "-RCB-", ".", "?", "!", ",", ":", "-", "--", "...", ";"])
_PUNCT_LOWER = frozenset(p.lower() for p in PUNCTUATIONS)
METRICS = ("Bleu_1", "Bleu_2", "Bleu_3", "Bleu_4", "ROUGE_L", "CIDEr")


def tokenize_caption(text):
    """A predicted caption -> words: lower-cased, split on whitespace, the tokens of coco-caption's punctuation list dropped (compared after
    lower-casing, so '-lrb-' is dropped as '-LRB-' is)."""
    return [w for w in text.lower().split() if w not in _PUNCT_LOWER]


def words_of_row(row):
    """The word string of a padded row: the ids before the first 0 (all of them without one)."""
    out = []
    for t in row:
        t = int(t)
        if t == 0:
            break
        out.append(t)
    return out


def lcs_len(a, b):
    """Length of the longest common subsequence of two sequences (the quadratic DP): the specification of the device kernel."""
    prev = [0] * (len(b) + 1)
    for x in a:
        cur = [0]
        for j, y in enumerate(b):
            cur.append(prev[j] + 1 if x == y else max(prev[j + 1], cur[j]))
        prev = cur
    return prev[-1]


class Rouge(object):
    """ROUGE-L.  Per hypothesis h with references r: lcs_r = lcs_len(h, r); prec = max_r lcs_r / len_h, rec = max_r lcs_r / len_r;
    score = (1 + beta^2) prec rec / (rec + beta^2 prec), 0 when prec or rec is 0.  An empty hypothesis scores 0; an empty reference
    contributes precision 0 and recall 0.  The corpus value is the mean of the sentence scores."""

    def __init__(self, beta=1.2):
        self.beta = float(beta)

    def from_lcs(self, len_h, pairs):
        """The sentence score from integers: len_h and [(lcs_r, len_r), ...] over the valid references (fp64)."""
        prec = rec = 0.0
        for lcs, len_r in pairs:
            if len_h > 0 and len_r > 0:
                prec = max(prec, lcs / float(len_h))
                rec = max(rec, lcs / float(len_r))
        if prec == 0.0 or rec == 0.0:
            return 0.0
        b2 = self.beta ** 2
        return (1.0 + b2) * prec * rec / (rec + b2 * prec)

    def sentence_lcs(self, hypo, refs):
        """[(lcs_r, len_r), ...] of one hypothesis (a sequence of words) against its references."""
        return [(lcs_len(hypo, r), len(r)) for r in refs]

    def sentence_score(self, hypo, refs):
        return self.from_lcs(len(hypo), self.sentence_lcs(hypo, refs))

    def compute_score(self, gts, res):
        """Dictionaries of whitespace-joined strings, as CiderD.compute_score takes -> (mean, per-key scores)."""
        assert gts.keys() == res.keys()
        scores = np.array([self.sentence_score(res[k][0].split(), [r.split() for r in gts[k]]) for k in gts.keys()], dtype=np.float64)
        return (float(scores.mean()) if len(scores) else 0.0), scores


def corpus_bleu(stats, n=4):
    """coco-caption's corpus BLEU-1..n with option='closest' from per-sentence integers: stats [N, n + 2] = (correct_1..n, len_h, reflen) as
    Bleu.sentence_stats gives them.  Sums of correct_k, guess_k = max(0, len_h - k + 1), len_h and reflen over the sentences;
    p_k = p_(k-1) (sum correct_k + 1e-15) / (sum guess_k + 1e-9), Bleu_k = p_k^(1/k); ratio = (sum len_h + 1e-15) / (sum reflen + 1e-9), and
    ratio < 1 multiplies every Bleu_k by exp(1 - 1 / ratio).  float64 [n]."""
    stats = np.asarray(stats, dtype=np.int64).reshape(-1, n + 2)
    len_h = stats[:, n]
    out = np.empty(n)
    p = 1.0
    for k in range(1, n + 1):
        correct = int(stats[:, k - 1].sum())
        guess = int(np.maximum(0, len_h - k + 1).sum())
        p = p * (correct + Bleu.TINY) / (guess + Bleu.SMALL)
        out[k - 1] = p ** (1.0 / k)
    ratio = (int(len_h.sum()) + Bleu.TINY) / (int(stats[:, n + 1].sum()) + Bleu.SMALL)
    if ratio < 1:
        out *= np.exp(1 - 1 / ratio)
    return out


def _join(ids):
    return " ".join(str(t) for t in ids)


class CaptionMetrics(object):
    """score(refs, hyps, on) -> {"Bleu_1".."Bleu_4", "ROUGE_L", "CIDEr": corpus values (float), "images": N, "scored_on_host": the number of
    images that do not fit the kernel -- the ones the host classes score whatever `on` says; on="host" scores all the others there too --, "per_image": {"bleu_stats"
    int64 [N, 6], "ROUGE_L" float64 [N], "CIDEr" float64 [N]}}.

    refs[i] is the list of references of image i (at least one), hyps[i] its hypothesis; a reference or hypothesis is a list of words
    (any hashable, sortable values of one type: strings, or ids).  Words are mapped to ids 1..N over the sorted union of all words; more than
    65 534 distinct words are refused.  df is counted over the reference sets of these images (one document per image).
    chunk: images per kernel call on the device (at most 1024)."""

    def __init__(self, sigma=6.0, beta=1.2, chunk=MAX_G, device=None):
        if not 1 <= int(chunk) <= MAX_G:
            raise ValueError("CaptionMetrics: chunk must be in 1..%d" % MAX_G)
        self.sigma, self.chunk, self.device = float(sigma), int(chunk), device
        self.bleu, self.rouge = Bleu(), Rouge(beta)

    @staticmethod
    def vocabulary(refs, hyps):
        words = set()
        for h in hyps:
            words.update(h)
        for rs in refs:
            for r in rs:
                words.update(r)
        if len(words) > MAX_TOKEN_ID:
            raise ValueError("CaptionMetrics: %d distinct words; the n-gram keys hold ids up to %d" % (len(words), MAX_TOKEN_ID))
        return {w: i + 1 for i, w in enumerate(sorted(words))}

    def score(self, refs, hyps, on="host"):
        if on not in ("host", "device"):
            raise ValueError("CaptionMetrics: on must be 'host' or 'device'")
        if len(refs) != len(hyps) or not len(hyps):
            raise ValueError("CaptionMetrics: needs one hypothesis and one reference list per image, and at least one image")
        if any(len(rs) < 1 for rs in refs):
            raise ValueError("CaptionMetrics: an image without a reference")
        vocab = self.vocabulary(refs, hyps)
        hyp_ids = [[vocab[w] for w in h] for h in hyps]
        ref_ids = [[[vocab[w] for w in r] for r in rs] for rs in refs]
        N = len(hyp_ids)
        table = DocFreq.from_token_lists(ref_ids)
        stats = np.zeros((N, 6), dtype=np.int64)
        rouge, cider = np.zeros(N), np.zeros(N)
        fits = [len(h) <= MAX_T and len(rs) <= MAX_R and all(len(r) <= MAX_T for r in rs) for h, rs in zip(hyp_ids, ref_ids)]
        unfit = [i for i in range(N) if not fits[i]]
        on_dev = [i for i in range(N) if fits[i]] if on == "device" else []
        self._score_host(unfit if on == "device" else list(range(N)), hyp_ids, ref_ids, table, stats, rouge, cider)
        for lo in range(0, len(on_dev), self.chunk):
            self._score_device(on_dev[lo:lo + self.chunk], hyp_ids, ref_ids, table, stats, rouge, cider)
        out = dict(zip(METRICS[:4], (float(v) for v in corpus_bleu(stats))))
        out["ROUGE_L"] = float(np.mean(rouge))
        out["CIDEr"] = float(np.mean(cider))
        out["images"] = N
        out["scored_on_host"] = len(unfit)
        out["per_image"] = {"bleu_stats": stats, "ROUGE_L": rouge, "CIDEr": cider}
        return out

    def score_rows(self, hyp, ref, count=None, on="host"):
        """score() of padded id rows read as word strings: hyp [G, T], ref [G, R, T], count [G] (the first count[g], clamped to 1..R, references
        of image g are valid; None = all R)."""
        hyp, ref = np.asarray(hyp), np.asarray(ref)
        G, R = ref.shape[:2]
        n = [R if count is None else min(max(int(count[g]), 1), R) for g in range(G)]
        return self.score([[words_of_row(r) for r in ref[g, :n[g]]] for g in range(G)], [words_of_row(h) for h in hyp], on=on)

    def _score_host(self, idx, hyp_ids, ref_ids, table, stats, rouge, cider):
        if not idx:
            return
        scorer = CiderD(sigma=self.sigma, df=table)
        gts, res = {}, {}
        for i in idx:
            h, rs = hyp_ids[i], ref_ids[i]
            res[i], gts[i] = [_join(h)], [_join(r) for r in rs]
            correct, len_h, reflen = self.bleu.sentence_stats(res[i][0], gts[i])
            stats[i] = list(correct) + [len_h, reflen]
            rouge[i] = self.rouge.sentence_score(h, rs)
        cider[idx] = scorer.compute_score(gts, res)[1]            # per image given the table: no other image enters a score

    def _score_device(self, idx, hyp_ids, ref_ids, table, stats, rouge, cider):
        import torch
        from . import _lib as K
        dev = torch.device(self.device if self.device is not None else "cuda")
        G, R = len(idx), max(len(ref_ids[i]) for i in idx)
        hyp = np.zeros((G, MAX_T), dtype=np.int64)
        ref = np.zeros((G, R, MAX_T), dtype=np.int64)
        count = np.zeros(G, dtype=np.int32)
        for g, i in enumerate(idx):
            hyp[g, :len(hyp_ids[i])] = hyp_ids[i]
            count[g] = len(ref_ids[i])
            for r, ids in enumerate(ref_ids[i]):
                ref[g, r, :len(ids)] = ids
        keys, vals = table.to(dev)
        c = torch.empty(G, dtype=torch.float32, device=dev)
        st = torch.empty((G, 6), dtype=torch.int32, device=dev)
        lc = torch.empty((G, R, 2), dtype=torch.int32, device=dev)
        K.caption_eval(torch.from_numpy(hyp).to(dev), torch.from_numpy(ref).to(dev), torch.from_numpy(count).to(dev), c, st, lc, keys, vals,
                       table.n_docs, sigma=self.sigma)
        st, lc = st.cpu().numpy(), lc.cpu().numpy()
        stats[idx] = st
        cider[idx] = c.cpu().numpy().astype(np.float64)
        for g, i in enumerate(idx):
            rouge[i] = self.rouge.from_lcs(int(st[g, 4]), [(int(l), int(n)) for l, n in lc[g, :count[g]]])
