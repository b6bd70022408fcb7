"""CPU: the label-smoothed masked-LM loss (--label_smoothing; loss.py LabelSmoothingLoss, modeling.py:995-999, 1104-1106).

`smoothed_rows` restates the loss in fp64 from its definition; it is pinned here against the unmodified reference criterion (skipped
where the reference tree is absent) and is the yardstick of the GPU tests (tests/test_70_label_smoothing_gpu.py).  `closed_form_rows`
restates the algebra the HIP row kernel uses (two passes over the row: max, then sum exp and sum of z - max) and is checked against the
dense form.  The rest pins the model / checkpoint / entry-script surface and the C ABI of the new entry points."""
import ctypes
import math
import os
import subprocess

import pytest
import torch
import torch.nn.functional as F

from oracle import ref_loader
from oracle import vlp_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def smoothing_values(ls, V, dtype):
    """(s, c): the smoothed value and the confidence as the reference's buffer holds them in `dtype` (torch.full in fp32, then
    model.half() rounds; the confidence is scattered into the buffer's copy, i.e. rounded to its dtype)."""
    s = float(torch.tensor(ls / (V - 2), dtype=torch.float32).to(dtype))
    c = float(torch.tensor(1.0 - ls, dtype=dtype))
    return s, c


def smoothed_q(labels, V, s, c, ignore=0, dtype=torch.float64):
    R = labels.numel()
    q = torch.full((R, V), s, dtype=dtype)
    q[:, ignore] = 0
    lab = labels.reshape(-1)
    q[torch.arange(R), lab] = c
    q[lab == ignore] = 0
    return q


def smoothed_rows(logits, labels, s, c, ignore=0, qlogq_dtype=torch.float64):
    """[B, P] per-row KL(q || p) in fp64: sum_w q (log q - logp), 0 log 0 = 0, logp = log_softmax(logits).
    qlogq_dtype: every q log q term rounded to that dtype first.  The reference's F.kl_div evaluates xlogy(q, q) on its target's dtype
    before promoting, so with an fp16 buffer (model.half()) the label-independent term is (V-2) half(s log s) + half(c log c)."""
    B, P, V = logits.shape
    logp = F.log_softmax(logits.double().reshape(B * P, V), dim=-1)
    q = smoothed_q(labels.cpu(), V, s, c, ignore).to(logits.device)
    qt = q.to(qlogq_dtype)
    return (torch.xlogy(qt, qt).double() - q * logp).sum(-1).view(B, P)


def smoothed_loss(logits, labels, weights, s, c, drop_worst_ratio, ignore=0, qlogq_dtype=torch.float64):
    return O.loss_mask_and_normalize(smoothed_rows(logits, labels, s, c, ignore, qlogq_dtype), weights.double(), drop_worst_ratio)


def row_coef(rows, weights, drop_worst_ratio):
    """coef[r] = keep[b] * weight[r] / (sum of the kept samples' weights + 1e-5): d loss / d row_loss[r] of loss_mask_and_normalize."""
    B = rows.shape[0]
    w = weights.double()
    keep_n = int(B * (1 - drop_worst_ratio))
    _, kept = torch.topk((rows * w).sum(-1), keep_n, largest=False)
    keep = torch.zeros(B, dtype=torch.float64, device=rows.device)
    keep[kept] = 1.0
    den = float((w.sum(-1) * keep).sum()) + 1e-5
    return (keep[:, None] * w / den).reshape(-1)


def smoothed_grad(logits, labels, weights, s, c, drop_worst_ratio, ignore=0, qlogq_dtype=torch.float64):
    """[B*P, V] d loss / d logits = coef[r] * (p * sum(q) - q) (0 on rows whose label is `ignore`: q and sum(q) vanish)."""
    B, P, V = logits.shape
    coef = row_coef(smoothed_rows(logits, labels, s, c, ignore, qlogq_dtype), weights, drop_worst_ratio)
    q = smoothed_q(labels.cpu(), V, s, c, ignore).to(logits.device)
    p = F.softmax(logits.double().reshape(B * P, V), dim=-1)
    return coef[:, None] * (p * q.sum(-1, keepdim=True) - q)


def closed_form_rows(logits, labels, s, c, ignore=0, qlogq_dtype=torch.float64):
    """The HIP row kernel's algebra: m = max, S = sum exp(z - m), A = sum_{w != ignore} (z - m);
    row = q_log_q - s (A - (V-1) log S - logp_t) - c logp_t, 0 on rows whose label is `ignore`."""
    B, P, V = logits.shape
    z = logits.double().reshape(B * P, V)
    m = z.max(-1).values
    d = z - m[:, None]
    logS = torch.log(torch.exp(d).sum(-1))
    A = d.sum(-1) - d[:, ignore]
    lab = labels.reshape(-1).clamp(0, V - 1)
    lpt = d[torch.arange(B * P), lab] - logS
    sc = torch.tensor([s, c], dtype=qlogq_dtype)
    xs, xc = torch.xlogy(sc, sc).double()
    r = (V - 2) * xs + xc - s * (A - (V - 1) * logS - lpt) - c * lpt
    return torch.where(lab == ignore, torch.zeros_like(r), r).view(B, P)


def _case(V, B=6, P=5, seed=0):
    g = torch.Generator().manual_seed(seed)
    logits = (torch.randn(B, P, V, generator=g) * 3.0).half()
    labels = torch.randint(1, V, (B, P), generator=g)
    labels[0, 1] = 0
    labels[2, :2] = 0
    labels[3, 4] = V - 1
    labels[4, 0] = 1
    weights = (torch.rand(B, P, generator=g) < 0.8).long()
    weights[:, 0] = 1
    return logits, labels, weights


@pytest.mark.parametrize("V", [1001, 28996])
@pytest.mark.parametrize("ls", [0.1, 0.5, 1.0])
@pytest.mark.parametrize("half", [False, True])
def test_restatement_matches_reference_criterion(V, ls, half):
    if not ref_loader.reference_available():
        pytest.skip("reference tree not available")
    ref = ref_loader.load_reference()
    crit = ref.loss.LabelSmoothingLoss(ls, V, ignore_index=0, reduction="none")
    if half:
        crit = crit.half()
    dtype = torch.float16 if half else torch.float32
    assert crit.one_hot.dtype == dtype and tuple(crit.one_hot.shape) == (1, V)
    s, c = smoothing_values(ls, V, dtype)
    assert float(crit.one_hot[0, 1]) == s and float(crit.one_hot[0, 0]) == 0.0
    logits, labels, weights = _case(V)
    x = logits.float().requires_grad_(True)
    got = crit(F.log_softmax(x, dim=-1), labels)                    # modeling.py:1105-1106
    mine = smoothed_rows(logits, labels, s, c, qlogq_dtype=dtype)
    assert torch.allclose(got.double(), mine, rtol=2e-6, atol=2e-5), float((got.double() - mine).abs().max())
    assert bool((got[labels == 0] == 0).all())
    # without the per-term rounding the fp16 rows would sit a constant (V-2) * |half(s log s) - s log s| away (6e-5 at V = 1001, ls = 0.1)
    exact = smoothed_rows(logits, labels, s, c)
    assert float((exact - mine).abs().max()) <= (V - 2) * abs(s * math.log(s)) * (2.0 ** -10 if half else 2.0 ** -23) + 1e-5
    # the kernel's closed form equals the dense definition
    assert torch.allclose(closed_form_rows(logits, labels, s, c, qlogq_dtype=dtype), mine, rtol=1e-9, atol=1e-9)
    for ratio in (0.0, 0.3):
        ref_loss = O.loss_mask_and_normalize(got.float(), weights, ratio)
        want = float(smoothed_loss(logits, labels, weights, s, c, ratio, qlogq_dtype=dtype))
        assert abs(float(ref_loss.detach()) - want) <= 1e-5 * abs(want)
    # the backward the HIP kernel writes: coef * (p * sum(q) - q), rows with label 0 exactly zero
    ref_loss = O.loss_mask_and_normalize(got.float(), weights, 0.3)
    ref_loss.backward()
    g = smoothed_grad(logits, labels, weights, s, c, 0.3, qlogq_dtype=dtype)
    assert float((x.grad.reshape(-1, V).double() - g).abs().max()) <= 1e-4 * float(g.abs().max())      # fp32 autograd vs fp64
    assert bool((x.grad.reshape(-1, V)[labels.reshape(-1) == 0] == 0).all())


@pytest.mark.parametrize("ls", [0.1, 1.0])
def test_model_buffer_gives_the_reference_kernel_scalars(ls):
    from vlp_amd.loss import LabelSmoothingLoss
    V = 28996
    crit = LabelSmoothingLoss(ls, V, ignore_index=0, reduction="none")
    for dtype in (torch.float32, torch.float16):
        crit = crit.to(dtype)
        s, c = smoothing_values(ls, V, dtype)
        sc = torch.tensor([s, c], dtype=dtype)
        xs, xc = (float(v) for v in torch.xlogy(sc, sc))
        assert crit.kernel_scalars() == (s, c, (V - 2) * s + c, (V - 2) * xs + xc)
    if ls == 0.1:          # the fp16 numbers of the issue (s 3.4571e-6 instead of 3.4490e-6, c 0.89990234, sum(q) 1.0001)
        s, c, qs, _ = crit.kernel_scalars()
        assert abs(s - 3.4571e-6) < 1e-10 and c == 0.89990234375 and abs(qs - 1.0001) < 1e-4
    with pytest.raises(AssertionError):
        LabelSmoothingLoss(0.1, 2)


def _models(ls, vocab=512):
    from vlp_amd.modeling import BertConfig, BertForPreTrainingLossMask
    cfg = BertConfig(vocab, num_hidden_layers=2, type_vocab_size=6, label_smoothing=ls)
    return BertForPreTrainingLossMask(cfg, enable_butd=True, len_vis_input=100, tasks="img2txt", allow_random_fc7=True)


def test_smoothed_model_state_dict_and_layout():
    plain, sm = _models(None), _models(0.1)
    base = set(O.init_params(vocab_size=512, layers=2).keys()) | {"cls.predictions.decoder.weight"}
    assert set(plain.state_dict()) == base and plain.crit_mask_lm_smoothed is None
    sd = sm.state_dict()
    assert set(sd) == base | {"crit_mask_lm_smoothed.one_hot"}
    oh = sd["crit_mask_lm_smoothed.one_hot"]
    assert tuple(oh.shape) == (1, 512) and oh.dtype == torch.float32 and float(oh[0, 0]) == 0.0
    assert float(oh[0, 7]) == float(torch.tensor(0.1 / 510, dtype=torch.float32))
    # a buffer: not a parameter, so never in the engine's flat layout or an optimizer group
    assert [n for n, _ in sm.named_parameters()] == [n for n, _ in plain.named_parameters()]
    assert sm.engine.plan_layout(sm) == plain.engine.plan_layout(plain)
    assert sm.half().crit_mask_lm_smoothed.one_hot.dtype == torch.float16


def test_smoothed_checkpoint_keys_match_reference_and_load():
    from vlp_amd.modeling import load_checkpoint_state
    sm = _models(0.1)
    if ref_loader.reference_available():
        ref = ref_loader.build_reference_model(dict(vocab_size=512, num_hidden_layers=2, label_smoothing=0.1))
        rsd = ref.state_dict()
        assert set(rsd) == set(sm.state_dict())
        assert tuple(rsd["crit_mask_lm_smoothed.one_hot"].shape) == (1, 512)
    else:
        rsd = {k: v.clone() for k, v in _models(0.1).state_dict().items()}
    rsd = {k: v.clone() for k, v in rsd.items()}
    rsd["crit_mask_lm_smoothed.one_hot"] = rsd["crit_mask_lm_smoothed.one_hot"].half()          # saved after model.half()
    load_checkpoint_state(sm, rsd)
    assert sm.missing_keys == []
    assert torch.equal(sm.crit_mask_lm_smoothed.one_hot, rsd["crit_mask_lm_smoothed.one_hot"].float())
    # a checkpoint without the buffer (trained without smoothing) loads into a smoothed model: the buffer keeps its own values
    plain_sd = {k: v for k, v in rsd.items() if not k.startswith("crit_mask_lm_smoothed")}
    sm2 = _models(0.1)
    load_checkpoint_state(sm2, plain_sd)
    assert sm2.missing_keys == ["crit_mask_lm_smoothed.one_hot"]


def test_from_pretrained_label_smoothing_kwarg(tmp_path):
    from vlp_amd import modeling as M
    cfg = M.BertConfig(300, num_hidden_layers=1, type_vocab_size=6)
    open(os.path.join(tmp_path, "bert_config.json"), "w").write(cfg.to_json_string())
    m = M.BertForPreTrainingLossMask.from_pretrained(str(tmp_path), state_dict={}, label_smoothing=0.1, enable_butd=True, len_vis_input=100,
                                                     allow_random_fc7=True)
    assert m.config.label_smoothing == 0.1 and m.crit_mask_lm_smoothed is not None
    assert m.crit_mask_lm_smoothed.one_hot.shape == (1, 300)


def test_entry_script_copies_label_smoothing_into_the_config(tmp_path):
    from vlp_amd import run_img2txt_dist as R
    base = ["--output_dir", str(tmp_path), "--bert_model", "bert-base-cased", "--new_segment_ids", "--enable_butd", "--fp16"]
    args = R.derive_args(R.build_parser().parse_args(base + ["--label_smoothing", "0.1"]))
    assert R.model_config(args).label_smoothing == 0.1
    args = R.derive_args(R.build_parser().parse_args(base))
    assert not R.model_config(args).label_smoothing


def test_ls_structs_match_c_layout_and_are_exported(tmp_path):
    from vlp_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, "vlp_mlm_loss_ls_fwd") and hasattr(lib, "vlp_mlm_loss_ls_bwd")
    structs = {"vlp_mlm_loss_ls_fwd_args": _lib.MlmLossLsFwdArgs, "vlp_mlm_loss_ls_bwd_args": _lib.MlmLossLsBwdArgs}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "vlp_hip.h"', "int main(void) {"]
    for cname, st in structs.items():
        lines.append('printf("%s %%zu", sizeof(%s));' % (cname, cname))
        for fname, _ in st._fields_:
            lines.append('printf(" %%zu", offsetof(%s, %s));' % (cname, fname))
        lines.append('printf("\\n");')
    lines.append("return 0; }")
    src = os.path.join(tmp_path, "layout.c")
    open(src, "w").write("\n".join(lines))
    exe = os.path.join(tmp_path, "layout")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.strip().splitlines()
    assert len(out) == 2
    for line in out:
        parts = line.split()
        st = structs[parts[0]]
        assert int(parts[1]) == ctypes.sizeof(st), parts[0]
        assert [int(x) for x in parts[2:]] == [getattr(st, f).offset for f, _ in st._fields_], parts[0]
