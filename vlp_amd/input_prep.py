"""On-device input preparation.

The reference prepares every sample on the CPU inside the DataLoader workers (vlp/seq2seq_loader.py:229-359): it converts the fp16
region features to fp32, normalises the boxes / layer-norms the 1601 class probabilities into the 1607-d `vis_pe`, and materialises an
int64 [L, L] attention mask -- 1.7 MB of fp32 + 223 KB of mask per sample that then cross PCIe and are cast back to fp16
(run_img2txt_dist.py:464-468).  Here the loader only has to deliver what is on disk plus a few integers:

    img       f16 [B, 100, 2048]                      (as stored; BertForPreTrainingLossMask already accepts fp16 features)
    RawRegions(bbox f32 [B, 100, 6], cls_prob f16 [B, 100, 1601])     in place of `vis_pe`
    MaskSpec(second_st, second_end, is_s2s)  int32 [B]                  in place of `attention_mask`
    SparseAnswers(idx int32 [B, 10], score f32 [B, 10])                 in place of the dense f32 [B, 3129] VQA `ans_labels`

and the HIP engine builds the packed masks (vlp_mask_build) and the K-padded box/class encoding (vlp_vis_pe_prep) directly in the
buffers its kernels read; the BCE loss kernels look a column's target up in the row's (index, score) pairs (vlp_bce_sparse_loss_fwd / _bwd).
The objects are accepted wherever the reference API takes `vis_pe` / `attention_mask` / `ans_labels`
(BertForPreTrainingLossMask.forward); the dense tensors keep working unchanged.
"""
import collections

import torch

N_CLS = 1601            # Visual Genome object classes + background, hard-coded in the reference (seq2seq_loader.py:351)


class RawRegions(collections.namedtuple("RawRegions", ["bbox", "cls_prob"])):
    """bbox: f32 [B, Nv, 6] = (x1, y1, x2, y2, <ignored>, confidence) as read from the bbox h5 file (seq2seq_loader.py:330);
    cls_prob: f16 or f32 [B, Nv, 1601] as read from the `_cls` h5 file (:329)."""
    __slots__ = ()

    def to(self, device, non_blocking=False):
        return RawRegions(self.bbox.to(device, non_blocking=non_blocking), self.cls_prob.to(device, non_blocking=non_blocking))

    @property
    def shape(self):      # what the dense vis_pe would be
        return (self.bbox.shape[0], self.bbox.shape[1], 6 + self.cls_prob.shape[2])

    def check(self, B, Nv):
        if tuple(self.bbox.shape) != (B, Nv, 6) or self.bbox.dtype != torch.float32:
            raise RuntimeError("RawRegions.bbox must be f32 [%d, %d, 6]" % (B, Nv))
        if tuple(self.cls_prob.shape) != (B, Nv, N_CLS) or self.cls_prob.dtype not in (torch.float16, torch.float32):
            raise RuntimeError("RawRegions.cls_prob must be f16/f32 [%d, %d, %d]" % (B, Nv, N_CLS))
        if not (self.bbox.is_cuda and self.cls_prob.is_cuda):
            raise RuntimeError("RawRegions must live on the GPU (there is no CPU path)")


_MaskSpecBase = collections.namedtuple("MaskSpec", ["second_st", "second_end", "is_s2s", "lens_host"])
_MaskSpecBase.__new__.__defaults__ = (None,)


class MaskSpec(_MaskSpecBase):
    """Per-sample description of the self-attention mask of seq2seq_loader.py:292-301; second_st / second_end / is_s2s: int32 [B].
    second_st = len(tokens_a) + 2, second_end = len(tokens_a) + len(tokens_b) + 3, is_s2s = 1 (seq2seq) / 0 (bidirectional).
    lens_host (optional): second_end as a HOST list of ints -- the number of leading positions of each sample that anything attends.
    The loader knows it for free; with it the engine's padding-free step (VLP_VARLEN=1) needs no device read-back."""
    __slots__ = ()

    @staticmethod
    def from_lengths(len_a, len_b, s2s, device=None):
        """len_a: region placeholders per sample (int or sequence), len_b: caption tokens without the final [SEP], s2s: bool(s)."""
        len_b = torch.as_tensor(len_b, dtype=torch.int32).reshape(-1)
        B = len_b.numel()
        len_a = torch.as_tensor(len_a, dtype=torch.int32).reshape(-1).expand(B)
        s2s = torch.as_tensor(s2s).to(torch.int32).reshape(-1).expand(B)
        end = (len_a + len_b + 3).contiguous()
        spec = MaskSpec((len_a + 2).contiguous(), end, s2s.contiguous(), [int(v) for v in end.tolist()])
        return spec if device is None else spec.to(device)

    def to(self, device, non_blocking=False):
        return MaskSpec(*(t.to(device, non_blocking=non_blocking) for t in self[:3]), self.lens_host)

    def check(self, B, L):
        for t in self[:3]:
            if t.dtype != torch.int32 or t.numel() != B or not t.is_cuda:
                raise RuntimeError("MaskSpec fields must be int32 [%d] tensors on the GPU" % B)

    def dense(self, L):
        """The int64 [B, L, L] mask this spec stands for (host/debug helper; the engine never builds it)."""
        st, en, s2s = (t.to(torch.long).view(-1, 1, 1) for t in self[:3])
        q = torch.arange(L, device=self.second_st.device).view(1, L, 1)
        k = torch.arange(L, device=self.second_st.device).view(1, 1, L)
        tri = (k < st) | ((q >= st) & (q < en) & (k >= st) & (k <= q))
        return torch.where(s2s.bool(), tri, (k < en).expand(-1, L, -1)).to(torch.long)


N_ANSWERS = 3129        # entries of the VQA 2.0 answer vocabulary, hard-coded in the reference (modeling.py:1029)
N_ANSWER_SLOTS = 10     # a VQA 2.0 question has 10 human answers, hence at most 10 distinct ones
MAX_ANSWER_SLOTS = 16   # what the kernels hold per row (vlp_bce_sparse_loss_fwd / _bwd, vlp_vqa_answer_rows)

_SparseAnswersBase = collections.namedtuple("SparseAnswers", ["idx", "score", "verified_for"])
_SparseAnswersBase.__new__.__defaults__ = (None,)


class SparseAnswers(_SparseAnswersBase):
    """The VQA soft target of one batch as (answer index, score) pairs in place of the dense f32 [B, num_answers] `ans_labels`
    (seq2seq_loader.py:355 `ans_proc(...)['answers_scores']`): idx int32 [B, S], score f32 [B, S], S <= 16 (the loader uses 10);
    idx == -1 marks an empty slot.  The dense target it stands for is y[b, idx[b, s]] = score[b, s], 0 elsewhere.
    Contract the loss kernels rely on: the indices of a row are distinct, and every index is -1 or in [0, num_answers).
    verified_for (optional, host int): the num_answers this instance is KNOWN to satisfy the contract for -- from_answer_ids sets it and
    .to() carries it along, so check() costs the training path no device read-back."""
    __slots__ = ()

    @staticmethod
    def answer_scores(answer_ids, unk_index=0):
        """[(answer index, score)] of one question's answer indices, distinct answers in order of first appearance, the unknown index left out.
        Pythia's VQAAnswerProcessor.compute_answers_scores, the soft VQA accuracy: for each distinct answer, the mean over the n leave-one-out
        subsets of the n given answers of min(1, matches in the subset / 3) -- for n = 10 an answer given c = 1, 2, 3, >= 4 times scores
        0.3, 0.6, 0.9, 1.0.  Pythia's source is not part of this project or of the reference checkout; the rule is written from its
        published definition (as vlp_amd.scst.CiderD is from coco-caption's)."""
        answer_ids = [int(a) for a in answer_ids]
        n = len(answer_ids)
        out = []
        for a in answer_ids:
            if a == unk_index or any(a == seen for seen, _ in out):
                continue
            c = answer_ids.count(a)
            # subset j leaves answer j out: it holds c - 1 matches when answer j is `a`, else c
            accs = [min(1.0, float(c - (1 if answer_ids[j] == a else 0)) / 3) for j in range(n)]
            out.append((a, sum(accs) / len(accs)))
        return out

    @staticmethod
    def from_answer_ids(answer_ids, unk_index=0, slots=N_ANSWER_SLOTS, num_answers=N_ANSWERS, out=None):
        """answer_ids: per question the list of its (<= 10) indices into the answer vocabulary -> SparseAnswers on the host, scored by
        answer_scores().  A row of unknown answers only has every slot empty.  out: optional (idx, score) numpy arrays [B, slots] to fill
        (the loader's pinned buffers); the result then wraps them."""
        import numpy as np
        B = len(answer_ids)
        if not 0 < slots <= MAX_ANSWER_SLOTS:
            raise ValueError("SparseAnswers: slots must be in 1..%d" % MAX_ANSWER_SLOTS)
        if out is None:
            out = (np.empty((B, slots), dtype=np.int32), np.empty((B, slots), dtype=np.float32))
        idx, score = out
        idx[...] = -1
        score[...] = 0.0
        for b, answers in enumerate(answer_ids):
            pairs = SparseAnswers.answer_scores(answers, unk_index)
            if len(pairs) > slots:
                raise ValueError("SparseAnswers: question %d has %d distinct answers, more than the %d slots" % (b, len(pairs), slots))
            for s, (a, sc) in enumerate(pairs):
                if not 0 <= a < num_answers:
                    raise ValueError("SparseAnswers: answer index %d of question %d is outside [0, %d)" % (a, b, num_answers))
                idx[b, s], score[b, s] = a, sc
        return SparseAnswers(torch.from_numpy(idx), torch.from_numpy(score), num_answers)

    def to(self, device, non_blocking=False):
        return SparseAnswers(self.idx.to(device, non_blocking=non_blocking), self.score.to(device, non_blocking=non_blocking), self.verified_for)

    @property
    def shape(self):
        return tuple(self.idx.shape)

    def check(self, B, NA):
        """Layout always; the kernels' contract (distinct indices per row, each -1 or in [0, NA)) from `verified_for` when the instance carries
        it (the loader's always do: no device read-back), else by looking at the values (a read-back when they live on the GPU: only
        instances assembled by hand from device tensors pay it)."""
        S = self.idx.shape[1] if self.idx.dim() == 2 else 0
        if self.idx.dtype != torch.int32 or self.score.dtype != torch.float32 or tuple(self.idx.shape) != (B, S) \
                or tuple(self.score.shape) != (B, S) or not 0 < S <= MAX_ANSWER_SLOTS:
            raise RuntimeError("SparseAnswers must be idx int32 / score f32 [%d, S] with 1 <= S <= %d" % (B, MAX_ANSWER_SLOTS))
        if self.verified_for is not None and self.verified_for <= NA:
            return
        idx = self.idx.cpu().to(torch.long)
        if bool(((idx < -1) | (idx >= NA)).any()):
            raise RuntimeError("SparseAnswers: every answer index must be -1 (empty slot) or in [0, %d)" % NA)
        srt = idx.sort(dim=1).values
        if bool(((srt[:, 1:] == srt[:, :-1]) & (srt[:, 1:] >= 0)).any()):
            raise RuntimeError("SparseAnswers: the answer indices of a row must be distinct")

    def dense(self, num_answers):
        """The f32 [B, num_answers] target this stands for (host/debug helper; the engine never builds it)."""
        y = torch.zeros(self.idx.shape[0], num_answers, dtype=torch.float32, device=self.idx.device)
        b, s = torch.nonzero(self.idx >= 0, as_tuple=True)
        y[b, self.idx[b, s].to(torch.long)] = self.score[b, s]
        return y


MAX_CAPTION_REFS = 8    # references per image vlp_cider_d accepts
MAX_CAPTION_LEN = 64    # ids per reference row vlp_cider_d accepts


class CaptionRefs(collections.namedtuple("CaptionRefs", ["ids", "count"])):
    """The captions of each image of one batch as references of the SCST reward (vlp_cider_d, vlp_amd.scst): ids int64 [B, R, T] in the
    format `gt_ids` has -- the caption's tokens, then [SEP], then 0 up to T (no 0 when [SEP] lands in the last column) -- and count
    int32 [B], 1..R: the first count[b] rows of image b are its references, the others are never read as text.  The loader
    (vlp_amd.data.BatchPrefetcher(caption_refs=R)) delivers one in place of the dummy `ans_labels` of a caption batch."""
    __slots__ = ()

    def to(self, device, non_blocking=False):
        return CaptionRefs(self.ids.to(device, non_blocking=non_blocking), self.count.to(device, non_blocking=non_blocking))

    @property
    def shape(self):
        return tuple(self.ids.shape)

    def check(self, B, T):
        """Layout only (no device read-back): the reward kernel clamps count to 1..R itself."""
        R = self.ids.shape[1] if self.ids.dim() == 3 else 0
        if self.ids.dtype != torch.int64 or tuple(self.ids.shape) != (B, R, T) or not 0 < R <= MAX_CAPTION_REFS or not 0 < T <= MAX_CAPTION_LEN:
            raise RuntimeError("CaptionRefs.ids must be int64 [%d, R, %d] with 1 <= R <= %d and T <= %d" % (B, T, MAX_CAPTION_REFS, MAX_CAPTION_LEN))
        if self.count.dtype != torch.int32 or tuple(self.count.shape) != (B,):
            raise RuntimeError("CaptionRefs.count must be int32 [%d]" % B)
        if self.ids.device != self.count.device:
            raise RuntimeError("CaptionRefs.ids and .count must live on one device")
