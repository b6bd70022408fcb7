"""GPU: the dropout-ON training step (hidden / attention dropout 0.1, the configuration every real run and the benchmark use) against the
oracle with the SAME masks.

The kernels' dropout is a pure function of (seed, stream, row, col) (vlp_amd/csrc/common.h); tests/dropout_ref.py mirrors that hash and
holds the table of sites (stream ids, row / column meaning) the engine promises.  Each case runs one forward + backward of the model in
train() mode with a set step seed, rebuilds every mask of that step from the table, and runs the oracle's dropout hooks (pinned on the
CPU against the unmodified reference in train() mode, tests/test_oracle_vs_reference.py) on the device twice with those masks:

    fp32 + autograd            the truth
    fp16 (op by op) + autograd the reference's own arithmetic: its distance to the truth is the yardstick

Compared: logits, each of the three losses, the pooled output (pretext branch), the last layer's hidden states, every parameter gradient
(norm and whole-tensor L2 error) and exact zeros for the parameters the task never reaches.  What this sees and the p = 0 parity tests
plus the dropout self-consistency tests (same seed = same bits, dense = packed, side stream = main stream, resume) cannot: a stream id
that differs between forward and backward, the undropped LayerNorm gradient handed to a weight gradient, a missing 1/(1-p), a mask on the
wrong side of the residual add, an attention mask keyed (key, query) in one direction -- all deterministic, all identical dense and packed.
tests/test_dropout_oracle_cpu.py shows that each such slip moves some gradient by >= 5x the bounds used here.

Bounds: those of tests/test_10_model_gpu.py at p = 0 (dropout adds a multiplier in fp32, no rounding point):
    logits / pooled (max-rel) and hidden (rel-L2):  err(hip) <= err(fp16 oracle) + 1e-3
    each loss:                                     2e-3 relative
    gradient norm:                                 2e-2 ||ref|| + 2e-3 gscale              (dropout_ref.grad_norm_bound)
    gradient tensor (whole):                       max(3e-2 ||ref|| + 2e-3 gscale, 1.5 x the fp16 oracle's own error)   (grad_tensor_bound)
They hold as they stand (measured on one MI355X, all eight cases, profiles/dropout_parity_report.json): logits 0.9 - 1.15e-3 against a
yardstick of 1.0 - 1.5e-3; losses <= 3.3e-5 (the pretext loss 1.0e-3 of its 2e-3); hidden 0.73 - 0.95e-3 against 0.99 - 1.2e-3; gradient
norms <= 5.3 % of their bound; the worst gradient tensor of a case at 10 - 66 % of its bound -- a region-projection tensor in seven cases
(the first answer-classifier weight in vqa2), there its error equals the fp16 oracle's own within 3 % (the fp16 region features, which both read).
Every case writes what it measured (hip, yardstick, bound) to dropout_parity_report.json in the directory $VLP_REPORT_DIR names (default
test_reports/); profiles/dropout_parity_report.json is a copy of one run.

In a scratch copy of the engine each of these two edits makes test_img2txt_mixed_masks_three_layers fail: backward's `16 * i + 3` -> `16 * i + 2`
(among others the tied word-embedding gradient off by 1.93 against a bound of 0.40) and `dpre` in place of
`dy2` as the dY operand of the FFN-down wgrad (output.dense.weight: norm 4.24 for 4.40, bound 0.11; output.dense.bias 0.077 against 0.019)."""
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from oracle import vlp_oracle as O                                                  # noqa: E402  (checker)
from tests.dropout_ref import grad_norm_bound, grad_tensor_bound, step_masks        # noqa: E402
from tests.test_label_smoothing_cpu import smoothed_loss, smoothing_values          # noqa: E402
from tests.test_scst_cpu import layout_logp, layout_mirror, scst_inputs             # noqa: E402
from vlp_amd import _lib as K                                                       # noqa: E402
from vlp_amd import synthetic as S                                                  # noqa: E402
from vlp_amd.input_prep import MaskSpec                                             # noqa: E402
from vlp_amd.modeling import BertConfig, BertForPreTrainingLossMask, BertForSeq2SeqDecoder   # noqa: E402

DEV = torch.device("cuda:0")
V, H, HEADS, P_DROP = 1024, 768, 12, 0.1
LOSS_KEYS = ("mlm_loss", "vis_pretext_loss", "vqa_loss")
REPORT = {}
REPORT_DIR = os.environ.get("VLP_REPORT_DIR", "test_reports")


def relmax(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def relL2(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).norm() / (b.norm() + 1e-30))


def build(p, layers, Nv, tasks="img2txt", ls=0.0):
    cfg = BertConfig(V, num_hidden_layers=layers, type_vocab_size=6, hidden_dropout_prob=P_DROP, attention_probs_dropout_prob=P_DROP,
                     label_smoothing=ls)
    m = BertForPreTrainingLossMask(cfg, enable_butd=True, len_vis_input=Nv, tasks=tasks, allow_random_fc7=True)
    sd = dict(p)
    sd["cls.predictions.decoder.weight"] = p["bert.embeddings.word_embeddings.weight"]
    if ls:
        sd["crit_mask_lm_smoothed.one_hot"] = m.crit_mask_lm_smoothed.one_hot
    m.load_state_dict(sd, strict=True)
    return m.half().to(DEV).train()


def masks_of(eng, B, L, Nv, layers):
    return step_masks(eng.base_seed + eng.step_seed, P_DROP, P_DROP, B, L, Nv, H, HEADS, layers, device=DEV)


def hip_forward(m, b, step_seed, mir, input_mask=None):
    """One train() forward with the step seed set; asserts that the engine increments before use.  Returns the three losses."""
    eng = m.engine
    eng.step_seed = step_seed
    losses = m(b.img, b.vis_pe, b.input_ids, b.segment_ids, b.input_mask if input_mask is None else input_mask, b.lm_label_ids, b.ans_labels,
               b.is_next, masked_pos=b.masked_pos, masked_weights=b.masked_weights, task_idx=b.task_idx, vis_masked_pos=b.vis_masked_pos,
               mask_image_regions=mir, drop_worst_ratio=0.0)
    assert eng.step_seed == step_seed + 1                      # incremented once, BEFORE the kernels read it (backward reads the same value)
    return losses


def oracle_step(p, batch, masks, dtype, tasks, Nv, mir, gs, ls=0.0):
    """The hooked oracle on the device with autograd in `dtype`; the backward carries the same loss scale `gs` as the HIP step's."""
    pd = {k: v.to(DEV).to(dtype).clone().requires_grad_(True) for k, v in p.items()}
    b = S.batch_to(batch, DEV)
    out = O.forward_pretraining_loss_mask(pd, b, tasks=tasks, len_vis_input=Nv, capture=True, mask_image_regions=mir, dropout=masks)
    if ls:          # the label-smoothed KL on the same logits in place of the cross entropy (modeling.py:1104-1106; restated in fp64)
        s, c = smoothing_values(ls, V, torch.float16)
        out["mlm_loss"] = smoothed_loss(out["mlm_logits"], b.lm_label_ids, b.masked_weights, s, c, 0.0, qlogq_dtype=torch.float16)
        out["loss"] = out["mlm_loss"] + out["vis_pretext_loss"].double() + out["vqa_loss"].double()
    (out["loss"].sum() * gs).backward()
    res = dict(logits=out["vqa_logits" if tasks == "vqa2" else "mlm_logits"].detach().float(), hidden=out["hidden"][-1].detach().float(),
               losses=[float(out[k].detach().sum()) for k in LOSS_KEYS],
               grads={k: (None if t.grad is None else t.grad.detach().float() / gs) for k, t in pd.items()})
    if "pooled_output" in out:
        res["pooled"] = out["pooled_output"].detach().float()
    return res


class Checker(object):
    """Collects every figure of a case in the report, then fails on the first list of violated bounds (so one run shows them all)."""

    def __init__(self, case):
        self.case, self.bad, self.rep = case, [], REPORT.setdefault(case, {})

    def put(self, key, hip, yard, bound, ok):
        self.rep[key] = dict(hip=hip, yardstick=yard, bound=bound)
        if not ok:
            self.bad.append((key, self.rep[key]))

    def closer_than_fp16(self, key, hip, truth, yard, metric):
        e, y = metric(hip, truth), metric(yard, truth)
        self.put(key, e, y, y + 1e-3, e <= y + 1e-3)

    def losses(self, hip, truth, yard):
        for k, a, t, y in zip(LOSS_KEYS, hip, truth, yard):
            if t == 0.0:
                self.put(k, a, y, 0.0, a == 0.0)                # a loss the task does not have: the shared zero
            else:
                self.put(k, abs(a - t) / abs(t), abs(y - t) / abs(t), 2e-3, abs(a - t) <= 2e-3 * abs(t))

    def grads(self, hip, truth, yard, unused):
        gscale = max(float(v.double().norm()) for v in truth.values() if v is not None)
        worst_n, worst_t = ("", 0.0), ("", 0.0)
        for n, ref in truth.items():
            g = hip[n]
            if ref is None:
                assert n in unused, n
                if float(g.abs().max()) != 0.0:
                    self.bad.append((n, "unused parameter with a gradient"))
                continue
            assert n not in unused, n
            rn, gn = float(ref.double().norm()), float(g.double().norm())
            e = float((g.double() - ref.double()).norm())
            y = float((yard[n].double() - ref.double()).norm()) if yard.get(n) is not None else 0.0
            nb, tb = grad_norm_bound(rn, gscale), grad_tensor_bound(rn, ref.numel(), gscale, y)
            if abs(gn - rn) > nb:
                self.bad.append((n, "norm", gn, rn, nb))
            if e > tb:
                self.bad.append((n, "tensor", e, y, tb))
            if abs(gn - rn) / nb > worst_n[1]:
                worst_n = (n, abs(gn - rn) / nb)
            if e / tb > worst_t[1]:
                worst_t = (n, e / tb, e, y, tb, rn)
        self.rep["grads"] = dict(gscale=gscale, tensors=sum(v is not None for v in truth.values()),
                                 worst_norm=dict(name=worst_n[0], fraction_of_bound=worst_n[1]),
                                 worst_tensor=dict(name=worst_t[0], fraction_of_bound=worst_t[1], hip=worst_t[2], yardstick=worst_t[3],
                                                   bound=worst_t[4], ref_norm=worst_t[5]))

    def finish(self):
        os.makedirs(REPORT_DIR, exist_ok=True)
        with open(os.path.join(REPORT_DIR, "dropout_parity_report.json"), "w") as f:
            json.dump(REPORT, f, indent=1, sort_keys=True)
        print("%s: %s" % (self.case, json.dumps(self.rep, sort_keys=True)))
        assert not self.bad, self.bad


def hip_grads(m, gs):
    return {n: q.grad.detach().float() / gs for n, q in m.named_parameters()}


def run_case(case, layers, Nv, B, max_len_b, tasks="img2txt", seed=0, mir=False, ls=0.0, varlen=False, gs=128.0, min_len_b=1, vis_mask_prob=0.0,
             s2s_prob=0.5, step_seed=40):
    p = O.init_params(vocab_size=V, layers=layers, tasks=tasks, seed=100 + seed)
    batch = S.make_batch(B, max_len_b=max_len_b, len_vis_input=Nv, vocab_size=V, max_pred=3 if tasks != "vqa2" else 1, s2s_prob=s2s_prob,
                         tasks=tasks, seed=200 + seed, min_len_b=min_len_b, vis_mask_prob=vis_mask_prob)
    L = batch.input_ids.shape[1]
    m = build(p, layers, Nv, tasks, ls)
    eng = m.engine
    b = S.batch_to(batch, DEV, half=True)
    spec, lens = None, None
    eng.varlen = bool(varlen)
    if varlen:       # the loader's form: per-sample lengths (host lengths ride along), rows packed, keys stay logical
        nb = [int(batch.input_mask[i].any(dim=0).sum()) - (Nv + 3) for i in range(B)]
        spec = MaskSpec.from_lengths(Nv, nb, [int(t) == 3 for t in batch.task_idx], device=DEV)
        assert torch.equal(spec.dense(L).cpu(), batch.input_mask)
        lens = [max(n, Nv + 2) for n in spec.lens_host]
    losses = hip_forward(m, b, step_seed, mir, input_mask=spec)
    masks = masks_of(eng, B, L, Nv, layers)
    ((losses[0] + losses[1] + losses[2]).sum() * gs).backward()
    torch.cuda.synchronize()
    if varlen:
        assert eng.last_packed_rows == sum(lens) and sum(lens) < B * L
    else:
        assert eng.last_packed_rows is None
    truth = oracle_step(p, batch, masks, torch.float32, tasks, Nv, mir, gs, ls)
    yard = oracle_step(p, batch, masks, torch.float16, tasks, Nv, mir, gs, ls)
    c = Checker(case)
    logits = (m.last_vqa_logits if tasks == "vqa2" else m.last_mlm_logits).float()
    c.closer_than_fp16("logits", logits.reshape(truth["logits"].shape), truth["logits"], yard["logits"], relmax)
    c.losses([float(x.detach().sum()) for x in losses], truth["losses"], yard["losses"])
    if mir:
        c.closer_than_fp16("pooled", m.last_pooled_output.float(), truth["pooled"], yard["pooled"], relmax)
    Pk = batch.masked_pos.shape[1] if tasks != "vqa2" else 0
    hs = eng._ws[(B, L, Pk)]["layers"][layers - 1]["x2"].float()
    th, yh = truth["hidden"].reshape(B * L, H), yard["hidden"].reshape(B * L, H)
    if varlen:       # packed rows: sample b's first lens[b] positions
        idx = torch.cat([bb * L + torch.arange(n) for bb, n in enumerate(lens)]).to(DEV)
        hs, th, yh = hs[:idx.numel()], th[idx], yh[idx]
    c.closer_than_fp16("hidden_last", hs, th, yh, relL2)
    c.grads(hip_grads(m, gs), truth["grads"], yard["grads"], eng.unused_parameter_names())
    c.rep["shape"] = dict(layers=layers, Nv=Nv, B=B, L=L, rows=eng.last_packed_rows or B * L, seed=eng.base_seed + eng.step_seed)
    c.finish()
    return m, batch, p


def test_img2txt_mixed_masks_three_layers():
    """3 layers, Nv = 100, B = 4, L = 123 (M = 492 < 2048: split-M wgrads): streams of layers 0, 1, 2, both dY-set parities, a ragged
    last key tile (123 = 3 x 32 + 27); captions of 1..20 tokens, seq2seq and bidirectional samples mixed."""
    run_case("img2txt_L123_3l", 3, 100, 4, 20, seed=1)


def test_img2txt_packed_rows_with_maskspec():
    """The same batch as per-sample lengths (MaskSpec) on the padding-free step: packed rows, logical (b*L + l) dropout rows and keys."""
    run_case("img2txt_L123_3l_packed", 3, 100, 4, 20, seed=1, varlen=True)


def test_grouped_wgrad_at_the_row_threshold():
    """B * L = 16 x 128 = 2048 rows: the first size at which a layer's four weight gradients go through gemm_tn_grouped, whose operand
    list names the dropped / undropped LayerNorm gradients a second time."""
    run_case("img2txt_grouped_M2048", 2, 8, 16, 117, seed=2, min_len_b=60)


def test_vqa2_head_behind_dropped_hidden_states():
    run_case("vqa2_B5", 2, 8, 5, 20, tasks="vqa2", seed=3, gs=1.0)       # (the VQA loss is BCE x 3129, ~2000: no loss scale)


def test_mask_image_regions_pretext_on_dropped_projections():
    """Pm = 2 of Nv = 8 regions masked: pretext_fwd / pretext_bwd read the DROPPED projections (streams 1001 / 1002), embed_bwd skips the
    masked rows."""
    run_case("vismask_Pm2", 2, 8, 4, 20, seed=4, mir=True, vis_mask_prob=0.25)


def test_label_smoothing_loss_pair():
    run_case("label_smoothing", 2, 8, 4, 20, seed=5, ls=0.1)


def test_two_micro_steps_accumulate():
    """Two forward / backward passes without zero_grad: the second takes seed s + 2 and ADDS its gradient; the sum equals the sum of the
    oracle's gradients under the two steps' masks."""
    layers, Nv, B, gs = 2, 100, 4, 128.0
    p = O.init_params(vocab_size=V, layers=layers, seed=106)
    batch = S.make_batch(B, max_len_b=20, len_vis_input=Nv, vocab_size=V, max_pred=3, s2s_prob=0.5, seed=206, min_len_b=1)
    L = batch.input_ids.shape[1]
    m = build(p, layers, Nv)
    eng = m.engine
    eng.varlen = False
    b = S.batch_to(batch, DEV, half=True)
    c = Checker("two_micro_steps")
    truth, yard = [], []
    for k in range(2):
        losses = hip_forward(m, b, 70 + k, False)
        assert eng.base_seed + eng.step_seed == eng.base_seed + 71 + k
        masks = masks_of(eng, B, L, Nv, layers)
        ((losses[0] + losses[1] + losses[2]).sum() * gs).backward()
        truth.append(oracle_step(p, batch, masks, torch.float32, "img2txt", Nv, False, gs))
        yard.append(oracle_step(p, batch, masks, torch.float16, "img2txt", Nv, False, gs))
        lh, lt, ly = float(losses[0].detach()), truth[k]["losses"][0], yard[k]["losses"][0]
        c.put("mlm_loss_step%d" % k, abs(lh - lt) / lt, abs(ly - lt) / lt, 2e-3, abs(lh - lt) <= 2e-3 * lt)
    torch.cuda.synchronize()
    assert truth[0]["losses"][0] != truth[1]["losses"][0]          # two different masks

    def total(rs):
        return {n: (None if rs[0]["grads"][n] is None else rs[0]["grads"][n] + rs[1]["grads"][n]) for n in rs[0]["grads"]}
    c.grads(hip_grads(m, gs), total(truth), total(yard), eng.unused_parameter_names())
    c.finish()


def test_scoring_layout_with_explicit_position_ids():
    """The SCST scoring sequence (vlp_scst_layout's layout, explicit position ids, one [MASK] slot per sampled token) through
    Engine.forward with dropout ON and the log-probability backward: vlp_embed_bwd_pos with drop_p > 0, the region rows' masks behind
    explicit positions.  (Engine.score_samples itself scores without dropout, so the product reaches this combination only through
    Engine.forward(position_ids=..., dropout=True); the layout and the loss are those score_samples sets up.)"""
    layers, Nv, B, gs = 2, 8, 3, 128.0
    p = O.init_params(vocab_size=V, layers=layers, seed=107)
    cfg = BertConfig(V, num_hidden_layers=layers, type_vocab_size=6, hidden_dropout_prob=P_DROP, attention_probs_dropout_prob=P_DROP)
    m = BertForSeq2SeqDecoder(cfg, mask_word_id=S.MASK_ID, eos_id=S.SEP_ID, enable_butd=True, len_vis_input=Nv)
    sd = dict(p)
    sd["cls.predictions.decoder.weight"] = p["bert.embeddings.word_embeddings.weight"]
    m.load_state_dict(sd, strict=True)
    m = m.half().to(DEV).train()
    eng = m.engine
    img, vis_pe, prefix, seg, pos, am, sample, _ = scst_inputs(B, 8, 17, V, short=(1,), pos_offset=2, Nv=Nv)
    dv = [t.to(DEV) for t in (prefix, seg, pos, am, sample)]
    img16, vpe16 = img.to(DEV).half(), vis_pe.to(DEV).half()
    ids, seg2, pos2, mask2, mpos = layout_mirror(dv[0], dv[4], dv[1], dv[2], dv[3], S.MASK_ID)
    T, Lo = sample.shape[1], ids.shape[1]
    w = (torch.randn(B, T, generator=torch.Generator().manual_seed(3)) * 0.5).to(DEV)        # signed upstream gradient of every log-prob
    eng.step_seed = 90
    st = eng.forward(img16, vpe16, ids, seg2, mask2, mpos, True, True, False, position_ids=pos2, dropout=True, dense=True)
    assert eng.step_seed == 91 and st.seed == eng.base_seed + 91 and st.p_drop == (P_DROP, P_DROP)
    st.task_labels = dv[4].reshape(-1).contiguous()
    logp = torch.empty(B, T, device=DEV, dtype=torch.float32)
    K.token_logprob_fwd(st.ws["logits"], st.ws["Vp"], st.task_labels, logp, st.ws["lse_ce"], B * T, V)
    eng.zero_grad()
    eng.backward(st, None, "logprob", g_rows=(w * gs).reshape(-1).contiguous())
    torch.cuda.synchronize()
    masks = masks_of(eng, B, Lo, Nv, layers)

    def oracle(dtype):
        pd = {k: v.to(DEV).to(dtype).clone().requires_grad_(True) for k, v in p.items()}
        vf = O.vis_embed(pd, img16.to(dtype), drop=masks["vis"])
        vp = O.vis_pe_embed(pd, vpe16.to(dtype), drop=masks["vispe"])
        lp = layout_logp(pd, vf, vp, dv[0], dv[1], dv[2], dv[3], dv[4], S.MASK_ID, Nv=Nv, dropout=masks)
        ((lp.float() * w).sum() * gs).backward()
        return lp.detach().float(), {k: (None if t.grad is None else t.grad.detach().float() / gs) for k, t in pd.items()}
    lp32, g32 = oracle(torch.float32)
    lp16, g16 = oracle(torch.float16)
    c = Checker("scoring_position_ids")
    c.closer_than_fp16("logp", logp, lp32, lp16, relmax)
    c.grads(hip_grads(m, gs), g32, g16, eng.unused_parameter_names())
    c.rep["shape"] = dict(layers=layers, Nv=Nv, B=B, L=Lo, T=T)
    c.finish()
