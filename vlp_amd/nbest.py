"""The n-best list of a beam search: the finished hypotheses of every image, ranked by the rule the search's best hypothesis is picked with.

    last[b]          = the first frame whose K words are all eos, else F - 1
    candidate (f, k) = f <= last[b] and (wids[f, b, k] == eos or f == last[b])
    value            = float64(tot[f, b, k]) + length_penalty * (f + 1)
    order            = value descending, then f*K + k ascending

Rank 0 is BertForSeq2SeqDecoder._backtrack_batch's hypothesis (modeling.py:1446-1474 of the reference, quirks included); the further ranks are
the hypotheses the search has paid for and used to drop.  Rows are sample-major, as scst.clean_captions and consensus.consensus_select_device
take them: rank n of image b is row n*B + b.

beam_nbest_host is the specification (numpy, fp64); the device form is vlp_beam_nbest (csrc/elementwise.hip) behind Engine.beam_nbest, which
BertForSeq2SeqDecoder.beam_search uses for n_best > 1 or backtrack = "device".
"""
import numpy as np

MAX_BEAMS = 64       # vlp_beam_nbest: K <= 64,
MAX_FRAMES = 256     # F <= 256


def check_limits(F, B, K, n_best, out_len):
    if not (B > 0 and 1 <= n_best <= K <= MAX_BEAMS and 1 <= F <= MAX_FRAMES and out_len >= F):
        raise ValueError("an n-best list needs 1 <= n_best <= beams <= %d, 1 <= frames <= %d and an output length >= frames "
                         "(got n_best=%d, beams=%d, frames=%d, output length %d, batch %d)" % (MAX_BEAMS, MAX_FRAMES, n_best, K, F, out_len, B))


def beam_nbest_host(tot, wids, ptrs, n_best, eos_id, length_penalty, out_len):
    """tot f32 / wids / ptrs int64 [F, B, K] (arrays or tensors): the frames of Engine.decode_beam.  Returns, sample-major,
        seq int64 [n_best*B, out_len]   the hypothesis along its back pointers, zero padded (a pointer outside [0, K) counts as 0)
        score f32 [n_best*B]            its cumulative log-probability tot[f, b, k]
        value f64 [n_best*B]            the ranking value
        len int32 [n_best*B]            f + 1
        ok uint8 [n_best*B]             1: the value is finite and no word before the last one is eos (0: the continuation of a hypothesis
                                        that had ended; the search keeps those at -10000)
    A rank whose value is not finite is an all-zero row with len 0 and ok 0 (the reference's [0])."""
    def arr(t, dt):
        return np.ascontiguousarray((t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)).astype(dt, copy=False))
    tot, wids, ptrs = arr(tot, np.float32), arr(wids, np.int64), arr(ptrs, np.int64)
    if tot.ndim != 3 or wids.shape != tot.shape or ptrs.shape != tot.shape:
        raise ValueError("tot, wids and ptrs must be [frames, batch, beams] arrays of one shape")
    F, B, K = tot.shape
    N, T, eos, lp = int(n_best), int(out_len), int(eos_id), float(length_penalty)
    check_limits(F, B, K, N, T)
    all_eos = (wids == eos).all(axis=2)                                    # [F, B]
    last = np.where(all_eos.any(axis=0), all_eos.argmax(axis=0), F - 1)    # [B]
    f_idx = np.arange(F)[:, None, None]
    cand = (f_idx <= last[None, :, None]) & ((wids == eos) | (f_idx == last[None, :, None]))
    val = tot.astype(np.float64) + lp * (f_idx + 1)                        # [F, B, K]
    back = np.where((ptrs >= 0) & (ptrs < K), ptrs, 0)
    seq = np.zeros((N * B, T), dtype=np.int64)
    score = np.full(N * B, -np.inf, dtype=np.float32)
    value = np.full(N * B, -np.inf, dtype=np.float64)
    length = np.zeros(N * B, dtype=np.int32)
    ok = np.zeros(N * B, dtype=np.uint8)
    for b in range(B):
        idx = np.flatnonzero(cand[:, b, :].reshape(-1))                    # flat f*K + k, ascending
        v = val[:, b, :].reshape(-1)[idx]
        order = idx[np.lexsort((idx, -v))]                                 # value descending, index ascending
        for n, i in enumerate(order[:N].tolist()):
            f, k = divmod(i, K)
            row = n * B + b
            score[row], value[row] = tot[f, b, k], val[f, b, k]
            if not np.isfinite(val[f, b, k]):
                continue
            length[row], clean = f + 1, True
            for t in range(f, -1, -1):
                w = wids[t, b, k]
                seq[row, t] = w
                clean = clean and (t == f or w != eos)
                k = back[t, b, k]
            ok[row] = 1 if clean else 0
    return seq, score, value, length, ok


def by_image(x, n_best):
    """Sample-major [n_best*B, ...] (tensor or array) -> [B, n_best, ...]: the ranks of one image next to each other."""
    B = x.shape[0] // n_best
    x = x.reshape(n_best, B, *x.shape[1:])
    return x.transpose(0, 1) if hasattr(x, "detach") else np.swapaxes(x, 0, 1)
