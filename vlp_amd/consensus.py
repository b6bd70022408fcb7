"""Consensus selection among the K sampled captions of an image (minimum-Bayes-risk decoding): keep the sample that agrees most with the
image's other samples, measured by CIDEr-D with the document frequencies of a training set.  No references are needed.

    utility[k*B + b] = CIDEr-D of sample k of image b with the image's other K - 1 samples as its references (ascending j, j != k)
    pick[b]          = the lowest k with the largest utility of image b

Rows are sample-major, as Engine.decode_sample_group returns them: row k*B + b is sample k of image b.  The strings are the reward's
(vlp_amd.scst.array_to_str: the ids up to and including the first 0), which is what scst.clean_captions produces and what the tables of
`python -m vlp_amd.cider_df` are counted over.

consensus_utility is the specification (host, fp64, scst.CiderD); consensus_select_device is the vlp_cider_d_consensus kernels
(csrc/reward.hip).  select_by_logprob is the other selection rule of `python -m vlp_amd.sample_img2txt --select`: the most probable sample.
"""
from collections import OrderedDict

import numpy as np
import torch

from . import scst as SC

MAX_SAMPLES = SC.MAX_SAMPLES


def _check_samples(n_rows, n_samples):
    n_samples = int(n_samples)
    if not 2 <= n_samples <= MAX_SAMPLES:
        raise ValueError("a selection among the samples of an image needs 2..%d samples per image (got %d)" % (MAX_SAMPLES, n_samples))
    if n_rows % n_samples:
        raise ValueError("%d rows are not %d samples of every image" % (n_rows, n_samples))
    return n_samples, n_rows // n_samples


def _check_table(df):
    if not isinstance(df, SC.DocFreq):
        raise TypeError("df must be a vlp_amd.scst.DocFreq")
    return df


def first_max(values, n_samples):
    """values [K*B] sample-major -> the lowest k with the largest value of each image, int64 [B]."""
    return np.argmax(np.asarray(values).reshape(n_samples, -1), axis=0)


def consensus_utility(ids, n_samples, df):
    """The specification, on the host in fp64.  ids [K*B, T] (tensor or array), df a DocFreq.  Returns (utility float64 [K*B], pick int64
    [B]): every row scored by scst.CiderD(df=df) against the image's other samples, the pick the first maximum."""
    _check_table(df)
    ids = ids.detach().cpu().numpy() if torch.is_tensor(ids) else np.asarray(ids)
    K, B = _check_samples(len(ids), n_samples)
    strs = [SC.array_to_str(row) for row in ids.tolist()]
    gts, res = OrderedDict(), OrderedDict()
    for i in range(K * B):
        k, b = divmod(i, B)
        res[i] = [strs[i]]
        gts[i] = [strs[j * B + b] for j in range(K) if j != k]
    utility = np.asarray(SC._table_scorer(df).compute_score(gts, res)[1], dtype=np.float64)
    return utility, first_max(utility, K)


def consensus_select_device(ids, n_samples, df, utility_out=None, pair_out=None, workspace=None):
    """consensus_utility on the device (vlp_cider_d_consensus): ids int64 [K*B, T] on the GPU.  Returns (pick int32 [B], utility f32 [K*B])
    as device tensors; utility_out (f32 [K*B]) receives the utilities when given, pair_out (f32 [B, K, K]) the score of every sample against
    every other one alone; workspace: the caller's kernel scratch (_lib.cider_d_consensus_workspace_bytes(B, K, T) bytes, uint8), else
    allocated per call.  Two launches on the current stream, no synchronisation, capturable; the table is uploaded once per device."""
    from . import _lib as K_
    _check_table(df)
    if not torch.is_tensor(ids) or ids.dim() != 2:
        raise ValueError("consensus_select_device: ids must be an int64 [K*B, T] device tensor")
    K, B = _check_samples(ids.shape[0], n_samples)
    utility = utility_out if utility_out is not None else torch.empty(K * B, dtype=torch.float32, device=ids.device)
    pick = torch.empty(B, dtype=torch.int32, device=ids.device)
    keys, vals = df.to(ids.device)
    K_.cider_d_consensus(ids, K, keys, vals, df.n_docs, utility, pick, pair=pair_out, sigma=SC._table_scorer(df).sigma, workspace=workspace)
    return pick, utility


def select_by_logprob(logprobs, n_samples):
    """logprobs [K*B] sample-major (the sequence log-probabilities) -> the lowest k with the largest one of each image, int64 [B]."""
    logprobs = logprobs.detach().cpu().numpy() if torch.is_tensor(logprobs) else np.asarray(logprobs, dtype=np.float64)
    logprobs = logprobs.reshape(-1)
    K, _ = _check_samples(len(logprobs), n_samples)
    return first_max(logprobs, K)
