"""GPU: the label-smoothed masked-LM loss (--label_smoothing) on the fused HIP path.

(1) vlp_mlm_loss_ls_fwd / _bwd through the C ABI against the fp64 restatement (tests/test_label_smoothing_cpu.py, pinned there against
    the unmodified reference criterion) on the same fp16 logits;
(2) the model with smoothing against the oracle's fp32 evaluation (encoder + gather_seq_out_by_pos + lm_head of oracle/vlp_oracle.py and
    the restated loss), every gradient tensor on the small model, padding-free vs dense, and the full BASELINE size;
(3) the entry script and the model API: --label_smoothing trains the KL (it used to train plain CE), checkpoints carry the reference's
    buffer and reload.
Every test prints what it measured (pytest -s); bounds are the measured values + 20 %."""
import json
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from oracle import vlp_oracle as O                                                 # noqa: E402  (checker only)
from tests.test_label_smoothing_cpu import smoothed_grad, smoothed_loss, smoothing_values   # noqa: E402
from vlp_amd import _lib as K                                                      # noqa: E402
from vlp_amd import synthetic as S                                                 # noqa: E402
from vlp_amd.modeling import BertConfig, BertForPreTrainingLossMask, load_checkpoint_state   # noqa: E402
from vlp_amd.optimization_fp16 import FP16_Optimizer_State, FusedAdam             # noqa: E402

DEV = torch.device("cuda:0")
REPORT = {}


def report(key, **kw):
    REPORT.setdefault(key, {}).update(kw)
    print("%s: %s" % (key, json.dumps(REPORT[key], sort_keys=True)))


def rel(a, b):
    """max(max-normalised error, relative L2 error) -- the metric of tests/test_00_kernels_gpu.py::test_mlm_loss."""
    a, b = a.detach().double(), b.detach().double()
    d = a - b
    return max(float(d.abs().max() / (b.abs().max() + 1e-30)), float(d.norm() / (b.norm() + 1e-30)))


def relL2(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).norm() / (b.norm() + 1e-30))


def scalars(ls, V, dtype):
    s, c = smoothing_values(ls, V, dtype)
    sc = torch.tensor([s, c], dtype=dtype, device=DEV)           # xlogy on the device, as the reference's model evaluates it
    xs, xc = (float(v) for v in torch.xlogy(sc, sc))
    return s, c, (V - 2) * s + c, (V - 2) * xs + xc


# =====================================================================================================================================
# (1) kernels
# =====================================================================================================================================
@pytest.mark.parametrize("ratio", [0.0, 0.3])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("ls", [0.1, 0.5, 1.0])
@pytest.mark.parametrize("V,ld", [(28996, 29056), (1001, 1008)])
def test_smoothed_loss_kernels(V, ld, ls, dtype, ratio):
    g = torch.Generator(device=DEV)
    g.manual_seed(4321)
    B, P = 16, 3
    logits = torch.full((B * P, ld), 30.0, device=DEV, dtype=torch.half)          # pad columns: large values the loss must not see
    logits[:, :V] = (torch.randn(B * P, V, device=DEV, generator=g) * 2.0).half()
    labels = torch.randint(1, V, (B, P), device=DEV, generator=g)
    labels[::5, 1] = 0                                                              # ignore_index rows
    labels[1, 2] = V - 1
    weights = (torch.rand(B, P, device=DEV, generator=g) < 0.7).long()
    weights[:, 0] = 1
    s, c, q_sum, q_log_q = scalars(ls, V, dtype)
    loss, lse, coef, row = (torch.zeros(n, device=DEV) for n in (1, B * P, B * P, B * P))
    K.mlm_loss_ls_fwd(logits, ld, labels, weights, loss, lse, coef, row, B, P, V, s, c, q_sum, q_log_q, ignore_index=0, drop_worst_ratio=ratio)
    x = logits[:, :V].view(B, P, V)
    want = float(smoothed_loss(x, labels, weights, s, c, ratio, qlogq_dtype=dtype))
    err = abs(float(loss) - want) / abs(want)
    assert bool((row.view(B, P)[labels == 0] == 0).all())
    gs = torch.full((1,), 128.0, device=DEV)
    dl = torch.full((B * P, ld), 3.0, device=DEV, dtype=torch.half)
    K.mlm_loss_ls_bwd(logits, ld, labels, lse, coef, gs, dl, ld, B * P, V, s, c, q_sum, ignore_index=0)
    torch.cuda.synchronize()
    ref = smoothed_grad(x, labels, weights, s, c, ratio, qlogq_dtype=dtype) * 128.0
    gerr = rel(dl[:, :V].float(), ref)
    report("kernel V%d ls%g %s ratio%g" % (V, ls, str(dtype)[6:], ratio), loss_rel_err=err, dlogits_rel_err=gerr)
    assert err < 1e-4, (float(loss), want)
    assert gerr < 2e-3
    assert float(dl[:, V:].abs().max()) == 0                                       # pad columns
    assert float(dl[labels.reshape(-1) == 0].abs().max()) == 0                     # label-0 rows, every column


def test_smoothed_kernels_refuse_bad_arguments():
    x = torch.zeros(4, 8, device=DEV, dtype=torch.half)
    lab = torch.ones(4, device=DEV, dtype=torch.long)
    f = torch.zeros(4, device=DEV)
    with pytest.raises(RuntimeError, match="V > 2"):
        K.mlm_loss_ls_fwd(x, 8, lab, lab, f, f, f, f, 2, 2, 2, 0.5, 0.5, 1.0, 0.0)
    with pytest.raises(RuntimeError, match="smoothing parameters"):
        K.mlm_loss_ls_bwd(x, 8, lab, f, f, f, x, 8, 4, 8, 0.1, 0.3, 1.0, ignore_index=8)


# =====================================================================================================================================
# (2) the model
# =====================================================================================================================================
def _build(p, V, layers, ls, drop=0.0):
    cfg = BertConfig(V, num_hidden_layers=layers, type_vocab_size=6, hidden_dropout_prob=drop, attention_probs_dropout_prob=drop, label_smoothing=ls)
    m = BertForPreTrainingLossMask(cfg, enable_butd=True, len_vis_input=100, tasks="img2txt", allow_random_fc7=True)
    sd = dict(p)
    sd["cls.predictions.decoder.weight"] = p["bert.embeddings.word_embeddings.weight"]
    if ls:
        sd["crit_mask_lm_smoothed.one_hot"] = m.crit_mask_lm_smoothed.one_hot
    m.load_state_dict(sd, strict=True)
    return m.half().to(DEV)


def _hip(m, b, scale=None):
    losses = m(b.img, b.vis_pe, b.input_ids, b.segment_ids, b.input_mask, b.lm_label_ids, b.ans_labels, b.is_next, masked_pos=b.masked_pos,
               masked_weights=b.masked_weights, task_idx=b.task_idx, vis_masked_pos=b.vis_masked_pos, mask_image_regions=False, drop_worst_ratio=0.0)
    if scale is not None:
        m.engine.zero_grad()
        (losses[0] * scale).sum().backward()
    torch.cuda.synchronize()
    return losses


def _oracle_smoothed(p, batch, ls, V, grads):
    """fp32 forward of the oracle up to the LM logits + the fp64 restated loss (dropout 0); gradients by autograd."""
    pd = {k: v.to(DEV).clone().requires_grad_(grads) for k, v in p.items()}
    b = S.batch_to(batch, DEV)
    with torch.set_grad_enabled(grads):
        vf, vp = O.vis_embed(pd, b.img.float()), O.vis_pe_embed(pd, b.vis_pe.float())
        emb, _ = O.embeddings(pd, vf, vp, b.input_ids, b.segment_ids, 100)
        seq = O.encoder(pd, emb, O.extended_attention_mask(b.input_mask, torch.float32), 12)[-1]
        logits = O.lm_head(pd, O.gather_seq_out_by_pos(seq, b.masked_pos))
        s, c = smoothing_values(ls, V, torch.float16)
        loss = smoothed_loss(logits, b.lm_label_ids, b.masked_weights, s, c, 0.0, qlogq_dtype=torch.float16)
        if grads:
            loss.backward()
    return float(loss.detach()), logits.detach(), ({k: t.grad for k, t in pd.items()} if grads else None)


def test_small_model_smoothed_loss_and_every_gradient_vs_oracle():
    V, ls = 1024, 0.1
    p = O.init_params(vocab_size=V, layers=2, seed=11)
    batch = S.make_batch(8, max_len_b=20, vocab_size=V, max_pred=3, s2s_prob=0.5, seed=12)
    m = _build(p, V, 2, ls).eval()
    GS = 1024.0
    losses = _hip(m, S.batch_to(batch, DEV, half=True), scale=GS)
    lh = float(losses[0])
    lo, logits_o, go = _oracle_smoothed(p, batch, ls, V, grads=True)
    # the kernel on the HIP logits against the restatement on the same logits
    s, c = smoothing_values(ls, V, torch.float16)
    b = S.batch_to(batch, DEV)
    own = float(smoothed_loss(m.last_mlm_logits, b.lm_label_ids, b.masked_weights, s, c, 0.0, qlogq_dtype=torch.float16))
    ce = float(O.loss_mask_and_normalize(F.cross_entropy(m.last_mlm_logits.float().transpose(1, 2), b.lm_label_ids, reduction="none"),
                                         b.masked_weights, 0.0))
    params = dict(m.named_parameters())
    per = {}
    for n, v in go.items():
        if v is None:
            assert float(params[n].grad.float().abs().max()) == 0.0, n
            continue
        nv = go[n.replace("key.bias", "query.bias")] if n.endswith("attention.self.key.bias") else v     # (true value 0, see test_20)
        per[n] = float((params[n].grad.float() / GS - v).double().norm() / (nv.double().norm() + 1e-30))
    worst = max(per, key=per.get)
    rep = dict(loss_hip=lh, loss_oracle_fp32=lo, loss_rel_err=abs(lh - lo) / lo, loss_vs_restated_own_logits=abs(lh - own) / own, ce_same_logits=ce,
               logits_relmax=float((m.last_mlm_logits.float() - logits_o).abs().max() / logits_o.abs().max()),
               grad_worst_relL2=per[worst], grad_worst_tensor=worst, grad_median_relL2=sorted(per.values())[len(per) // 2], grad_tensors=len(per))
    report("small_model", **rep)
    assert rep["loss_vs_restated_own_logits"] < 1e-4, rep
    assert abs(lh - ce) > 0.05 * ce, rep                                  # a KL, not the CE of the same logits
    assert len(per) == 48, rep
    # measured: loss 1.52e-5 from the fp32 truth, logits 1.03e-3 (max-rel), worst gradient tensor 1.47e-2 rel-L2 (vis_pe_embed.0.weight, also the
    # worst tensor of the plain-CE parity tests), median 1.0e-3
    assert rep["loss_rel_err"] <= 1.8e-5, rep
    assert rep["logits_relmax"] <= 1.24e-3, rep
    assert rep["grad_worst_relL2"] <= 1.76e-2, rep


def test_small_model_padding_free_equals_dense_with_smoothing():
    V, ls = 1024, 0.1
    p = O.init_params(vocab_size=V, layers=2, seed=13)
    b = S.batch_to(S.make_batch(8, max_len_b=20, vocab_size=V, max_pred=3, s2s_prob=0.5, seed=14), DEV, half=True)
    m = _build(p, V, 2, ls, drop=0.1).train()
    eng = m.engine
    res = []
    for packed in (False, True):
        eng.varlen = packed
        eng.step_seed = 7
        loss = _hip(m, b, scale=1024.0)[0].detach().clone()
        assert (eng.last_packed_rows is not None) == packed
        res.append((loss, m.last_mlm_logits.clone(), {n: q.grad.float().clone() for n, q in m.named_parameters()}))
    (l0, g0, gr0), (l1, g1, gr1) = res
    worst = max(relL2(gr1[n], gr0[n]) if float(gr0[n].norm()) > 0 else float(gr1[n].norm()) for n in gr0)
    report("padding_free_vs_dense", loss_dense=float(l0), loss_packed=float(l1), grad_worst_relL2=worst)
    assert torch.equal(l0, l1) and torch.equal(g0, g1)
    assert worst <= 1.3e-5                                                # measured 1.06e-5 (fp32 summation order of the row sums)


def test_full_size_smoothed_loss_vs_oracle():
    V, ls, B = 28996, 0.1, 64
    p = O.init_params(vocab_size=V, layers=12, seed=15)
    batch = S.make_batch(B, max_len_b=64, vocab_size=V, max_pred=3, s2s_prob=0.75, seed=16)
    assert batch.input_ids.shape == (B, 167)
    m = _build(p, V, 12, ls).eval()
    lh = float(_hip(m, S.batch_to(batch, DEV, half=True), scale=4096.0)[0])
    lo, logits_o, _ = _oracle_smoothed(p, batch, ls, V, grads=False)
    s, c = smoothing_values(ls, V, torch.float16)
    b = S.batch_to(batch, DEV)
    own = float(smoothed_loss(m.last_mlm_logits, b.lm_label_ids, b.masked_weights, s, c, 0.0, qlogq_dtype=torch.float16))
    rep = dict(loss_hip=lh, loss_oracle_fp32=lo, loss_rel_err=abs(lh - lo) / lo, loss_vs_restated_own_logits=abs(lh - own) / own,
               logits_relmax=float((m.last_mlm_logits.float() - logits_o).abs().max() / logits_o.abs().max()))
    report("full_size", **rep)
    assert rep["loss_vs_restated_own_logits"] < 1e-4, rep
    assert rep["loss_rel_err"] <= 2.3e-6, rep                             # measured 1.88e-6 from the fp32 truth
    assert rep["logits_relmax"] <= 2.0e-3, rep                            # measured 1.69e-3
    assert all(torch.isfinite(q.grad.float()).all() for q in m.parameters())


# =====================================================================================================================================
# (3) the model API and the entry script
# =====================================================================================================================================
def test_model_with_label_smoothing_trains_a_step_on_the_smoothed_kernels(monkeypatch):
    from vlp_amd.run_img2txt_dist import train_step
    calls = {k: 0 for k in ("mlm_loss_fwd", "mlm_loss_bwd", "mlm_loss_ls_fwd", "mlm_loss_ls_bwd")}
    for name in calls:
        fn = getattr(K, name)

        def counted(*a, _fn=fn, _name=name, **k):
            calls[_name] += 1
            return _fn(*a, **k)
        monkeypatch.setattr(K, name, counted)
    V = 1024
    p = O.init_params(vocab_size=V, layers=2, seed=17)
    named_groups = lambda m: [{"params": [q for n, q in m.named_parameters() if "bias" not in n and "LayerNorm" not in n], "weight_decay": 0.01},
                              {"params": [q for n, q in m.named_parameters() if "bias" in n or "LayerNorm" in n], "weight_decay": 0.0}]
    b = S.batch_to(S.make_batch(4, max_len_b=20, vocab_size=V, max_pred=3, seed=18), DEV, half=True)
    for ls in (None, 0.1):
        m = _build(p, V, 2, ls).train()
        before = {n: q.detach().clone() for n, q in m.named_parameters()}
        opt = FP16_Optimizer_State(FusedAdam(named_groups(m), lr=1e-4, bias_correction=False, max_grad_norm=1.0), dynamic_loss_scale=True)
        lt = train_step(m, opt, b, 1e-4)
        torch.cuda.synchronize()
        assert not opt.overflow and torch.isfinite(lt[0]).all()
        assert any(not torch.equal(before[n], q) for n, q in m.named_parameters())
        if ls is None:
            assert calls == {"mlm_loss_fwd": 1, "mlm_loss_bwd": 1, "mlm_loss_ls_fwd": 0, "mlm_loss_ls_bwd": 0}, calls   # today's launches
        else:
            assert calls == {"mlm_loss_fwd": 1, "mlm_loss_bwd": 1, "mlm_loss_ls_fwd": 1, "mlm_loss_ls_bwd": 1}, calls
    # backward follows the choice its forward recorded, whatever the module holds by then
    losses = m(b.img, b.vis_pe, b.input_ids, b.segment_ids, b.input_mask, b.lm_label_ids, b.ans_labels, b.is_next, masked_pos=b.masked_pos,
               masked_weights=b.masked_weights, drop_worst_ratio=0.0)
    crit, m.crit_mask_lm_smoothed = m.crit_mask_lm_smoothed, None
    (losses[0] * 1024.0).backward()
    m.crit_mask_lm_smoothed = crit
    torch.cuda.synchronize()
    assert calls["mlm_loss_ls_fwd"] == 2 and calls["mlm_loss_ls_bwd"] == 2 and calls["mlm_loss_bwd"] == 1, calls


def _main_first_step(R, monkeypatch, argv):
    seen = {}
    orig = R.train_step

    def spy(model, optimizer, batch, lr, **kw):
        lt = orig(model, optimizer, batch, lr, **kw)
        if "loss" not in seen:
            mm = model.module if hasattr(model, "module") else model
            seen.update(loss=float(lt[0].detach()), logits=mm.last_mlm_logits.detach().clone(), labels=batch[3].clone(), weights=batch[5].clone(),
                        ratio=kw.get("drop_worst_ratio", 0.0))
        return lt
    monkeypatch.setattr(R, "train_step", spy)
    R.main(argv)
    monkeypatch.setattr(R, "train_step", orig)
    return seen


def test_entry_script_label_smoothing_trains_the_kl_and_reloads(tmp_path, monkeypatch):
    from vlp_amd import run_img2txt_dist as R
    base = ["--do_train", "--fp16", "--enable_butd", "--new_segment_ids", "--from_scratch", "--max_len_b", "20", "--train_batch_size", "4",
            "--synthetic", "3", "--num_hidden_layers", "2", "--len_vis_input", "100", "--log_every", "1"]
    out = os.path.join(tmp_path, "ls")
    sm = _main_first_step(R, monkeypatch, base + ["--output_dir", out, "--num_train_epochs", "1", "--label_smoothing", "0.1"])
    ce = _main_first_step(R, monkeypatch, base + ["--output_dir", os.path.join(tmp_path, "ce"), "--num_train_epochs", "1"])
    V = 28996
    s, c = smoothing_values(0.1, V, torch.float16)
    want = float(smoothed_loss(sm["logits"], sm["labels"], sm["weights"], s, c, sm["ratio"], qlogq_dtype=torch.float16))
    want_ce = float(O.loss_mask_and_normalize(F.cross_entropy(ce["logits"].float().transpose(1, 2), ce["labels"], reduction="none"),
                                              ce["weights"], ce["ratio"]))
    report("entry_script", first_loss_smoothed=sm["loss"], restated_kl=want, first_loss_plain=ce["loss"], restated_ce=want_ce)
    assert torch.equal(sm["logits"], ce["logits"])                       # same seed, same initial model, same first batch
    assert abs(sm["loss"] - want) <= 1e-4 * want, (sm["loss"], want)
    assert abs(ce["loss"] - want_ce) <= 1e-4 * want_ce, (ce["loss"], want_ce)
    assert abs(sm["loss"] - ce["loss"]) > 0.05 * ce["loss"]
    # the checkpoint carries the reference's buffer (fp16 after model.half()) and reloads: into a model, and as the entry script's resume
    sd = torch.load(os.path.join(out, "model.1.bin"))
    oh = sd["crit_mask_lm_smoothed.one_hot"]
    assert tuple(oh.shape) == (1, V) and oh.dtype == torch.float16 and float(oh[0, 0]) == 0 and float(oh[0, 5]) == s
    assert "crit_mask_lm_smoothed.one_hot" not in torch.load(os.path.join(tmp_path, "ce", "model.1.bin"))
    cfg = BertConfig(V, num_hidden_layers=2, type_vocab_size=6, label_smoothing=0.1)
    fresh = BertForPreTrainingLossMask(cfg, enable_butd=True, len_vis_input=100, allow_random_fc7=True)
    load_checkpoint_state(fresh, sd)
    assert fresh.missing_keys == []
    R.main(base + ["--output_dir", out, "--num_train_epochs", "2", "--label_smoothing", "0.1"])          # resumes from model.1.bin / optim.1.bin
    sd2 = torch.load(os.path.join(out, "model.2.bin"))
    assert torch.equal(sd2["crit_mask_lm_smoothed.one_hot"], oh)
    assert all(torch.isfinite(v.float()).all() for v in sd2.values())
    assert not torch.equal(sd2["cls.predictions.bias"], sd["cls.predictions.bias"])
