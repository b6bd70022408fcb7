"""Host side of scoring given captions (BertForSeq2SeqDecoder.score, python -m vlp_amd.score_img2txt): which positions of a caption are
counted, and the arithmetic of the records, the summary and the selection.  No GPU is needed for anything here.

The counting rule, with T = the decoder's number of output positions and n = the caption's number of tokens:
  * n < T: the caption is scored over n + 1 positions -- its n tokens and the closing [SEP] the decoder would have to write behind them;
  * n >= T: the caption is cut to its first T tokens, no [SEP] is counted (the decoder never got to write one) and it is flagged truncated;
  * every position behind the counted ones holds -1: it is fed to the model as id 0, its logits row is never read and it adds to no sum.
Sums are reduced here in fp64 from the per-token fp32 values of the device, as vlp_amd.eval_captions reduces its integers."""
import math
from collections import OrderedDict

import numpy as np
import torch


def is_truncated(n_tokens, T):
    return n_tokens >= T


def counted_positions(caption_ids, T, sep_id, lengths=None, vocab_size=None):
    """caption_ids: a sequence of R token id lists, or a padded [R, W] tensor / array with lengths [R] (the number of tokens of every row;
    None: all W).  Returns (ids int64 [R, T] with -1 at the positions that are not counted, counted bool [R, T], truncated bool [R]), CPU
    tensors.  Token ids must lie in [0, vocab_size) (vocab_size None: >= 0)."""
    T = int(T)
    if T < 1:
        raise ValueError("the decoder has %d output positions: nothing can be scored" % T)
    if torch.is_tensor(caption_ids) or isinstance(caption_ids, np.ndarray):
        rows = torch.as_tensor(caption_ids).detach().cpu().tolist()
        if rows and not isinstance(rows[0], list):
            raise ValueError("caption_ids must be [R, W] (one caption per row)")
    else:
        rows = [list(r) for r in caption_ids]
    if lengths is not None:
        lengths = [int(n) for n in (lengths.tolist() if hasattr(lengths, "tolist") else lengths)]
        if len(lengths) != len(rows):
            raise ValueError("lengths holds %d entries for %d captions" % (len(lengths), len(rows)))
        for r, n in enumerate(lengths):
            if not 0 <= n <= len(rows[r]):
                raise ValueError("caption %d: length %d outside 0..%d" % (r, n, len(rows[r])))
        rows = [row[:n] for row, n in zip(rows, lengths)]
    R = len(rows)
    ids = torch.full((R, T), -1, dtype=torch.long)
    truncated = torch.zeros(R, dtype=torch.bool)
    for r, row in enumerate(rows):
        row = [int(t) for t in row]
        bad = [t for t in row[:T] if t < 0 or (vocab_size is not None and t >= vocab_size)]
        if bad:
            raise ValueError("caption %d: token id %d is outside the vocabulary [0, %s)" % (r, bad[0], "inf" if vocab_size is None else vocab_size))
        if is_truncated(len(row), T):
            ids[r] = torch.tensor(row[:T], dtype=torch.long)
            truncated[r] = True
        else:
            ids[r, :len(row) + 1] = torch.tensor(row + [int(sep_id)], dtype=torch.long)
    return ids, ids >= 0, truncated


def caption_record(logp, entropy, rank, counted):
    """One caption's figures from its [T] rows (any of tensor / array / list): {tokens, logprob, ppl, top1, top5, entropy}.  tokens, top1 and
    top5 are integers (counted positions; those with rank 0 / rank < 5), logprob the fp64 sum of the per-token values, entropy their fp64
    mean, ppl = exp(-logprob / tokens)."""
    c = np.asarray(counted, dtype=bool)
    lp = np.asarray(logp, dtype=np.float64)[c]
    h = np.asarray(entropy, dtype=np.float64)[c]
    rk = np.asarray(rank, dtype=np.int64)[c]
    n = int(c.sum())
    total = float(lp.sum())
    return {"tokens": n, "logprob": total, "ppl": perplexity(total, n), "top1": int((rk == 0).sum()), "top5": int((rk < 5).sum()),
            "entropy": float(h.sum()) / n if n else None}


def perplexity(logprob, tokens):
    """exp(-logprob / tokens); None for an empty set, inf where the exponent overflows."""
    if tokens <= 0:
        return None
    x = -float(logprob) / tokens
    return math.exp(x) if x < 709.0 else float("inf")


def summarize(records):
    """The corpus figures from the per-caption records: {captions, tokens, logprob, ppl, top1, top5, entropy}.  logprob is the sum,
    ppl = exp(-sum logprob / sum tokens), top1 / top5 the shares of all counted positions with rank 0 / rank < 5, entropy the mean over
    all counted positions (a record's mean weighted by its tokens).  An empty set has no ppl, shares or entropy (None)."""
    tokens = sum(int(r["tokens"]) for r in records)
    logprob = math.fsum(float(r["logprob"]) for r in records)
    out = {"captions": len(records), "tokens": tokens, "logprob": logprob, "ppl": perplexity(logprob, tokens), "top1": None, "top5": None,
           "entropy": None}
    if tokens:
        out["top1"] = sum(int(r["top1"]) for r in records) / float(tokens)
        out["top5"] = sum(int(r["top5"]) for r in records) / float(tokens)
        out["entropy"] = math.fsum(float(r["entropy"]) * int(r["tokens"]) for r in records if r["tokens"]) / tokens
    return out


def caption_indices(image_ids):
    """The number of every caption within its image, by order of occurrence (an image's captions need not be adjacent)."""
    seen, out = {}, []
    for i in image_ids:
        out.append(seen.get(i, 0))
        seen[i] = out[-1] + 1
    return out


def select_likelihood(records, length_norm="none"):
    """One record {image_id, caption, index, logprob} per image, in the order the images first occur: the caption with the largest total
    log-probability (length_norm 'none') or the largest log-probability per counted token ('mean'); ties go to the lowest index.  logprob
    stays the total."""
    if length_norm not in ("none", "mean"):
        raise ValueError("length_norm must be 'none' or 'mean' (got %r)" % (length_norm,))
    best = OrderedDict()
    for r in records:
        value = r["logprob"] / r["tokens"] if length_norm == "mean" else r["logprob"]
        held = best.get(r["image_id"])
        if held is None or value > held[0] or (value == held[0] and r["index"] < held[1]["index"]):
            best[r["image_id"]] = (value, r)
    return [{"image_id": r["image_id"], "caption": r["caption"], "index": r["index"], "logprob": r["logprob"]} for _, r in best.values()]


def filter_examples(examples, images=None):
    """examples: [(store key, [token ids])]; images: None, or select_images' [(image id, store key)] of a split.  Returns [(image id, store
    key, token ids)] in input order: with a split only the examples whose key belongs to it, under that image's integer id; without one
    every example, the key being the id."""
    if images is None:
        return [(key, key, list(toks)) for key, toks in examples]
    id_of = {str(key): imgid for imgid, key in images}
    return [(id_of[str(key)], key, list(toks)) for key, toks in examples if str(key) in id_of]
