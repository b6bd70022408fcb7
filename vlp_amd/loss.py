"""Drop-in for `pytorch_pretrained_bert.loss` (the reference's loss.py): the label-smoothed masked-LM criterion.

As everywhere in vlp_amd the module is a container: it holds the reference's `one_hot` buffer (so state_dict keys, shapes and the
dtype the buffer takes under `model.half()` match a reference checkpoint trained with `--label_smoothing`), and the fused engine reads
the three numbers the HIP kernels need from it (`kernel_scalars`).  The arithmetic runs in vlp_mlm_loss_ls_fwd / _bwd (loss.hip).
"""
import torch
from torch import nn


class LabelSmoothingLoss(nn.Module):
    """KL divergence between the smoothed ground truth q and the model's distribution p (loss.py:12-48):
    q[w] = label_smoothing / (V - 2) for w != ignore_index, q[target] = 1 - label_smoothing, q == 0 on rows whose target is
    ignore_index."""

    def __init__(self, label_smoothing=0, tgt_vocab_size=0, ignore_index=0, size_average=None, reduce=None, reduction="mean"):
        super(LabelSmoothingLoss, self).__init__()
        assert 0.0 < label_smoothing <= 1.0
        assert tgt_vocab_size > 2, "label smoothing spreads over V - 2 words: needs a vocabulary of more than 2"
        assert 0 <= ignore_index < tgt_vocab_size
        self.ignore_index = ignore_index
        self.reduction = reduction
        self.label_smoothing = label_smoothing
        one_hot = torch.full((tgt_vocab_size,), label_smoothing / (tgt_vocab_size - 2), dtype=torch.float32)
        one_hot[ignore_index] = 0
        self.register_buffer("one_hot", one_hot.unsqueeze(0))
        self.confidence = 1.0 - label_smoothing
        self.tgt_vocab_size = tgt_vocab_size
        self._scalars = (None, None)

    def forward(self, *a, **k):
        raise NotImplementedError("LabelSmoothingLoss is a buffer container in vlp_amd: the fused HIP path evaluates it inside "
                                  "BertForPreTrainingLossMask.forward")

    def kernel_scalars(self):
        """(smooth, confidence, q_sum, q_log_q) exactly as the reference's forward sees them: `smooth` is the buffer's value in its
        CURRENT dtype (fp16 after model.half()), `confidence` is 1 - label_smoothing rounded to that dtype (the reference scatters it
        into the buffer's copy), q_sum = (V - 2) * smooth + confidence is the row sum of q, and q_log_q = sum_w q log q of a row with
        every term rounded to that dtype (F.kl_div evaluates xlogy on the target's dtype before promoting).  The buffer is read back
        once per storage / in-place change, not per step."""
        buf = self.one_hot
        key = (buf.data_ptr(), buf._version, buf.dtype, buf.device, self.confidence)
        if self._scalars[0] == key:
            return self._scalars[1]
        row = buf.detach().reshape(-1).double().cpu()
        V, ii = row.numel(), self.ignore_index
        if V != self.tgt_vocab_size:
            raise RuntimeError("crit_mask_lm_smoothed.one_hot has %d entries, expected %d" % (V, self.tgt_vocab_size))
        others = torch.cat((row[:ii], row[ii + 1:]))
        s = float(others[0])
        if float(row[ii]) != 0.0 or not bool((others == s).all()):
            raise NotImplementedError("the fused smoothed loss needs a uniform one_hot buffer with 0 at ignore_index (loss.py:28-31)")
        sc = torch.tensor([s, self.confidence], dtype=buf.dtype, device=buf.device)
        c = float(sc[1])
        xs, xc = (float(v) for v in torch.xlogy(sc, sc))           # on the buffer's device: the reference's xlogy is the one that runs there
        out = (s, c, (V - 2) * s + c, (V - 2) * xs + xc)
        self._scalars = (key, out)
        return out
