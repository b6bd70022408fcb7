"""TEST INFRASTRUCTURE ONLY -- CPU restatement (the *oracle*) of the reference's hot path.

Only ``tests/``, ``__graft_entry__.smoke()`` and ``bench.py``'s ``cpu_baseline`` leg may import
this file; the product (``vlp_amd/``) never does and fails loudly without its HIP library.

What it restates: the unified encoder-decoder forward of LuoweiZhou/VLP
(``pytorch_pretrained_bert/modeling.py``), its losses, and the optimizer arithmetic
(``pytorch_pretrained_bert/optimization.py`` + apex FusedAdam/FP16_Optimizer as called from
``vlp/run_img2txt_dist.py:411-420,571-585``).  Every function cites the reference lines it follows.
It is a *functional* restatement over a plain ``{state_dict key: tensor}`` dict (the reference's
checkpoint key names), written with elementary torch CPU ops in the dtype of the parameters
(fp32 for ground truth, fp64 for tight kernel checks).  Backward is obtained by torch autograd
over these elementary ops (the path is floating point, so a torch reference is the yardstick).

PINNING (see tests/test_oracle_vs_reference.py and oracle/make_golden.py):
  * forward / losses / gradients / BertAdam: pinned against the reference's own modeling.py and
    optimization.py executed unmodified in the build container (oracle/ref_loader.py), and against
    the committed fixtures in tests/golden/ generated from that reference.
  * apex arithmetic (FusedLayerNorm, FusedAdam, FP16_Optimizer @1603407): apex is not under
    /root/reference and is not installable offline -> **parity unpinned** for `fused_adam_step`
    and `LossScaler`; they restate apex's published algorithm from the call sites
    (run_img2txt_dist.py:411-420, optimization_fp16.py:7-80).  LayerNorm follows the in-repo
    python fallback (modeling.py:179-192), which is what runs when apex is absent.
  * Unlike the reference (modeling.py:231 asserts len_vis_input == 100) the restatement accepts any
    region count so BASELINE.json's 8-region plumbing config can be checked.
"""
import contextlib
import math

import torch
import torch.nn.functional as F

# ----------------------------------------------------------------------------------------------
# rounding-point policy of an fp16 evaluation (parity decomposition, tests/test_20_fullsize_gpu.py)
# ----------------------------------------------------------------------------------------------
# Run in fp16, the functions below round where the REFERENCE rounds: after every elementary torch op (modeling.py executes
# op by op on half tensors).  The HIP path evaluates the same algorithm but fuses ops, i.e. it rounds at fewer points (DESIGN.md
# section 4).  Each flag moves ONE group of rounding points from the reference's place to the HIP path's place, so that the distance
# between the two fp16 evaluations can be attributed deviation by deviation -- and so that the HIP path can be compared with an
# evaluation that rounds exactly where it does.  With no flag set (the default) nothing here changes: reference arithmetic.
ROUNDING_FLAGS = (
    "fused_sum",           # dense + bias + residual rounded once (reference: Linear output rounded, then the add; modeling.py:314-316, 354-356)
    "gelu_fp32",           # gelu evaluated in fp32 on the fp16 pre-activation, rounded once (reference: five fp16 ops, modeling.py:62-67)
    "ln_fp32",             # LayerNorm statistics and affine in fp32, rounded once (reference fallback: every op in fp16, modeling.py:188-192)
    "scores_fp32",         # q.k^T, the 1/sqrt(d) scale, the additive mask and the softmax in fp32 (reference rounds scores three times, modeling.py:284-292)
    "probs_unnormalized",  # P~ = exp(s - max) rounded to fp16, context = (P~ . V) / sum rounded once (reference: normalised P rounded, modeling.py:292-298)
    "embed_fused",         # word + position + type summed in fp32, rounded once (reference: two fp16 adds, modeling.py:236-239)
    "decoder_bias_fused",  # tied decoder: h . E^T + bias rounded once (reference: matmul rounded, then + bias, modeling.py:481)
)
# not a rounding point: the same arithmetic with every Linear's contraction index visited in another (fixed, seeded) order.  The
# distance between an evaluation and its "sum_order" twin is the noise floor of ANY two fp16 evaluations that round at the same points
# (it is what a different GEMM tiling does) -- the yardstick for "as close as the arithmetic allows".
PERTURBATION_FLAGS = ("sum_order",)
# "what if" evaluations (round 6, VERDICT r5 #6b) -- NOT how the reference or the HIP path computes: can an fp16-operand design reach 1e-3 against the
# fp32 truth at 12 layers if the RESIDUAL STREAM stays in fp32?
#   residual_fp32       every LayerNorm also keeps its unrounded fp32 output and the next residual add takes that one (GEMM operands stay fp16; the
#                       dense + bias + residual sum is still rounded to fp16 before its LayerNorm): one extra fp32 stream per LayerNorm
#   residual_fp32_full  additionally the pre-LayerNorm sum reaches the LayerNorm unrounded (fp32 GEMM outputs on the two residual GEMMs of a layer)
# Both imply fp32 LayerNorm arithmetic and the fused sum (flags ln_fp32 / fused_sum) where they act.
EXPERIMENT_FLAGS = ("residual_fp32", "residual_fp32_full")
_policy = frozenset()
_res32 = [None, None]      # latest LayerNorm output under a residual_fp32* flag: (fp16 tensor handed on, its unrounded fp32 twin)
_pre32 = [None, None]      # latest pre-LayerNorm sum under residual_fp32_full: (fp16 tensor handed on, its unrounded fp32 twin)


@contextlib.contextmanager
def rounding(*flags):
    """with rounding("gelu_fp32", ...): evaluate fp16 with those rounding points moved to where the HIP path rounds."""
    global _policy
    bad = [f for f in flags if f not in ROUNDING_FLAGS + PERTURBATION_FLAGS + EXPERIMENT_FLAGS]
    if bad:
        raise ValueError("unknown rounding flag(s) %r" % (bad,))
    old, _policy = _policy, frozenset(flags)
    try:
        yield
    finally:
        _policy = old
        _res32[:] = [None, None]
        _pre32[:] = [None, None]


def _res_exp(t):
    return t.dtype == torch.float16 and ("residual_fp32" in _policy or "residual_fp32_full" in _policy)


def _moved(flag, t):
    return flag in _policy and t.dtype == torch.float16


# ----------------------------------------------------------------------------------------------
# elementary ops
# ----------------------------------------------------------------------------------------------
def gelu(x):
    """modeling.py:62-67 (exact erf form)."""
    if _moved("gelu_fp32", x):
        xf = x.float()
        return (xf * 0.5 * (1.0 + torch.erf(xf / math.sqrt(2.0)))).half()
    return x * 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0)))


def layer_norm(x, weight, bias, eps=1e-5):
    """modeling.py:188-192 (TF style: eps inside the sqrt; biased variance)."""
    if _res_exp(x):
        xf = _pre32[1] if (x is _pre32[0]) else x.float()
        u = xf.mean(-1, keepdim=True)
        s = (xf - u).pow(2).mean(-1, keepdim=True)
        out32 = weight.float() * ((xf - u) / torch.sqrt(s + eps)) + bias.float()
        out16 = out32.half()
        _res32[:] = [out16, out32]
        return out16
    if _moved("ln_fp32", x):
        xf = x.float()
        u = xf.mean(-1, keepdim=True)
        s = (xf - u).pow(2).mean(-1, keepdim=True)
        return (weight.float() * ((xf - u) / torch.sqrt(s + eps)) + bias.float()).half()
    u = x.mean(-1, keepdim=True)
    s = (x - u).pow(2).mean(-1, keepdim=True)
    x = (x - u) / torch.sqrt(s + eps)
    return weight * x + bias


def _kperm(x, w):
    if "sum_order" not in _policy:
        return x, w
    g = torch.Generator().manual_seed(w.shape[1])
    perm = torch.randperm(w.shape[1], generator=g).to(w.device)
    return x[..., perm], w[:, perm]


def linear(x, w, b=None):
    """nn.Linear, as everywhere in modeling.py: F.linear (in fp16: fp32 accumulation, bias added before the ONE rounding)."""
    x, w = _kperm(x, w)
    return F.linear(x, w, b)


def _drop(t, mult):
    """nn.Dropout as a given multiplier tensor (0 or 1/(1-p) per element, any shape with t's element count); None: not there at all."""
    if mult is None:
        return t
    return t * mult.to(t.dtype).view(t.shape)


def _no_site(site):
    return None


def linear_add(x, w, b, res, drop=None):
    """Linear, dropout, residual add (BertSelfOutput / BertOutput, modeling.py:314-316, 354-356).  drop: the multiplier tensor of the
    nn.Dropout between the Linear and the add (None: dropout p = 0); the fused branches apply it in fp32 in front of their one rounding."""
    if _res_exp(x):
        r32 = _res32[1] if (res is _res32[0]) else res.float()
        x, w = _kperm(x, w)
        s32 = _drop(F.linear(x.float(), w.float(), b.float()), drop) + r32
        s16 = s32.half()
        if "residual_fp32_full" in _policy:
            _pre32[:] = [s16, s32]
        return s16
    if _moved("fused_sum", x):
        x, w = _kperm(x, w)
        return (_drop(F.linear(x.float(), w.float(), b.float()), drop) + res.float()).half()
    return _drop(linear(x, w, b), drop) + res


def extended_attention_mask(attention_mask, dtype):
    """modeling.py:807-833: [B,L,L] (or [B,L]) 0/1 -> additive [B,1,L,L] with 0 / -10000."""
    if attention_mask.dim() == 2:
        ext = attention_mask.unsqueeze(1).unsqueeze(2)
    elif attention_mask.dim() == 3:
        ext = attention_mask.unsqueeze(1)
    else:
        raise NotImplementedError
    ext = ext.to(dtype=dtype)
    return (1.0 - ext) * -10000.0


# ----------------------------------------------------------------------------------------------
# model
# ----------------------------------------------------------------------------------------------
def vis_embed(p, vis_feats, drop=None):
    """modeling.py:1003-1007,1035: Dropout(ReLU(Linear(2048,768)(ReLU(Linear(2048,2048)(x))))); drop: the Dropout's multiplier (None: p = 0)."""
    h = torch.relu(linear(vis_feats, p["vis_embed.0.weight"], p["vis_embed.0.bias"]))
    return _drop(torch.relu(linear(h, p["vis_embed.2.weight"], p["vis_embed.2.bias"])), drop)


def vis_pe_embed(p, vis_pe, drop=None):
    """modeling.py:1016-1018,1036."""
    return _drop(torch.relu(linear(vis_pe, p["vis_pe_embed.0.weight"], p["vis_pe_embed.0.bias"])), drop)


def embeddings(p, vis_feats_h, vis_pe_h, input_ids, token_type_ids, len_vis_input, position_ids=None,
               vis_input=True, drop=None):
    """modeling.py:217-241: rows 1..Nv of the word stream are the projected region features and rows
    1..Nv of the position stream are the projected box/class encodings.  drop: multiplier of the Dropout behind the LayerNorm (:240)."""
    B, L = input_ids.shape
    if position_ids is None:
        position_ids = torch.arange(L, dtype=torch.long, device=input_ids.device).unsqueeze(0).expand_as(input_ids)
    words = p["bert.embeddings.word_embeddings.weight"][input_ids]
    pos = p["bert.embeddings.position_embeddings.weight"][position_ids]
    if vis_input:
        Nv = len_vis_input
        words = torch.cat((words[:, :1], vis_feats_h, words[:, Nv + 1:]), dim=1)
        pos = torch.cat((pos[:, :1], vis_pe_h, pos[:, Nv + 1:]), dim=1)
    typ = p["bert.embeddings.token_type_embeddings.weight"][token_type_ids]
    if _moved("embed_fused", words):
        pre = (words.float() + pos.float() + typ.float()).half()
    else:
        pre = words + pos + typ
    out = layer_norm(pre, p["bert.embeddings.LayerNorm.weight"], p["bert.embeddings.LayerNorm.bias"])
    return _drop(out, drop), pre


def self_attention(p, pre, x, ext_mask, num_heads, history=None, cap=None, drop=None):
    """modeling.py:268-303.  `pre` = 'bert.encoder.layer.{i}.attention.self.'; drop: multiplier [B, heads, Lq, Lk] of the Dropout on the
    attention probabilities (:296), None: p = 0."""
    B, Lq, H = x.shape
    d = H // num_heads
    kv_in = x if history is None else torch.cat((history, x), dim=1)
    q = linear(x, p[pre + "query.weight"], p[pre + "query.bias"])
    k = linear(kv_in, p[pre + "key.weight"], p[pre + "key.bias"])
    v = linear(kv_in, p[pre + "value.weight"], p[pre + "value.bias"])

    def heads(t):  # transpose_for_scores :262-266
        return t.view(t.shape[0], t.shape[1], num_heads, d).permute(0, 2, 1, 3)

    q, k, v = heads(q), heads(k), heads(v)
    half = q.dtype == torch.float16
    if _moved("scores_fp32", q):
        scores = q.float().matmul(k.float().transpose(-1, -2)) / math.sqrt(d) + ext_mask.float()
    else:
        scores = q.matmul(k.transpose(-1, -2)) / math.sqrt(d)
        scores = scores + ext_mask
    if _moved("probs_unnormalized", q):
        sf = scores.float()
        e = torch.exp(sf - sf.max(dim=-1, keepdim=True)[0])
        probs = e / e.sum(dim=-1, keepdim=True)                    # (captured only)
        if drop is None:
            ctx = (e.half().float().matmul(v.float()) / e.sum(dim=-1, keepdim=True)).half()
        else:                                                      # the multiplier in fp32 in front of P~'s one rounding; the sum stays undropped
            ctx = ((e * drop.float().view(e.shape)).half().float().matmul(v.float()) / e.sum(dim=-1, keepdim=True)).half()
    else:
        probs = torch.softmax(scores, dim=-1)
        if half:
            probs = probs.half()
        ctx = _drop(probs, drop).matmul(v)
    ctx = ctx.permute(0, 2, 1, 3).contiguous().view(B, Lq, H)
    if cap is not None:
        cap["probs"] = probs
    return ctx


def bert_layer(p, i, x, ext_mask, num_heads, history=None, cap=None, dropout=None):
    """modeling.py:306-372 (BertSelfOutput, BertIntermediate, BertOutput, BertLayer).  dropout: {site: multiplier} holding this layer's
    ("attn", i), ("attn_out", i) and ("ffn_out", i), or None."""
    L = "bert.encoder.layer.%d." % i
    site = _no_site if dropout is None else dropout.get
    ctx = self_attention(p, L + "attention.self.", x, ext_mask, num_heads, history, cap, drop=site(("attn", i)))
    a = linear_add(ctx, p[L + "attention.output.dense.weight"], p[L + "attention.output.dense.bias"], x, drop=site(("attn_out", i)))
    a = layer_norm(a, p[L + "attention.output.LayerNorm.weight"], p[L + "attention.output.LayerNorm.bias"])
    g = gelu(linear(a, p[L + "intermediate.dense.weight"], p[L + "intermediate.dense.bias"]))
    o = linear_add(g, p[L + "output.dense.weight"], p[L + "output.dense.bias"], a, drop=site(("ffn_out", i)))
    o = layer_norm(o, p[L + "output.LayerNorm.weight"], p[L + "output.LayerNorm.bias"])
    if cap is not None:
        cap.update(ctx=ctx, attn_out=a, inter=g)
    return o


def num_layers_of(p):
    n = 0
    while ("bert.encoder.layer.%d.output.dense.weight" % n) in p:
        n += 1
    return n


def encoder(p, x, ext_mask, num_heads, num_layers=None, dropout=None):
    """modeling.py:382-402 (no-history path).  Returns the list of all layer outputs."""
    outs = []
    for i in range(num_layers if num_layers is not None else num_layers_of(p)):
        x = bert_layer(p, i, x, ext_mask, num_heads, dropout=dropout)
        outs.append(x)
    return outs


def pooler(p, h):
    """modeling.py:411-417."""
    return torch.tanh(linear(h[:, 0], p["bert.pooler.dense.weight"], p["bert.pooler.dense.bias"]))


def lm_head(p, h):
    """modeling.py:431-435, 465-482 (relax_projection off): LN(gelu(dense(x))) . E^T + bias (tied)."""
    t = gelu(linear(h, p["cls.predictions.transform.dense.weight"], p["cls.predictions.transform.dense.bias"]))
    t = layer_norm(t, p["cls.predictions.transform.LayerNorm.weight"], p["cls.predictions.transform.LayerNorm.bias"])
    if _moved("decoder_bias_fused", t):
        tt, ww = _kperm(t, p["bert.embeddings.word_embeddings.weight"])
        return F.linear(tt.float(), ww.float(), p["cls.predictions.bias"].float()).half()
    return linear(t, p["bert.embeddings.word_embeddings.weight"]) + p["cls.predictions.bias"]


def gather_seq_out_by_pos(seq, pos):
    """modeling.py:1068-1069."""
    return torch.gather(seq, 1, pos.unsqueeze(2).expand(-1, -1, seq.size(-1)))


def loss_mask_and_normalize(loss, mask, drop_worst_ratio):
    """modeling.py:1083-1093."""
    mask = mask.type_as(loss)
    loss = loss * mask
    keep_loss, keep_ind = torch.topk(loss.sum(-1), int(loss.size(0) * (1 - drop_worst_ratio)), largest=False)
    denominator = torch.sum(mask.sum(-1)[keep_ind]) + 1e-5
    return (keep_loss / denominator).sum()


def vqa_head(p, h, len_vis_input):
    """modeling.py:1027-1030,1044-1045,1138-1139."""
    e = h[:, 0] * h[:, len_vis_input + 1]
    z = torch.relu(linear(e, p["ans_classifier.0.weight"], p["ans_classifier.0.bias"]))
    return linear(z, p["ans_classifier.2.weight"], p["ans_classifier.2.bias"])


def vis_pretext_loss(vf, vp, pooled, vis_masked_pos):
    """modeling.py:1113-1131 (the Selfie-style pretext task of mask_image_regions, enable_butd=True): for every sample the masked
    regions' projected box/class encodings (+ the pooled [CLS] output) are matched against the masked regions' projected features;
    the loss is the mean over samples of the mean negative log-softmax on the diagonal of the [P, P] similarity matrix.
    vf / vp are the UNMASKED projections (:1035-1036; masked_fill at :1054-1055 is out of place)."""
    idx = (vis_masked_pos - 1).unsqueeze(-1)
    masked_vis_feats = torch.gather(vf, 1, idx.expand(-1, -1, vf.size(-1)))                 # :1115-1116
    masked_pos_enc = torch.gather(vp, 1, idx.expand(-1, -1, vp.size(-1)))                   # :1119-1120
    masked_pos_enc = masked_pos_enc + pooled.unsqueeze(1).expand_as(masked_pos_enc)          # :1124
    sim = torch.matmul(masked_pos_enc, masked_vis_feats.permute(0, 2, 1).contiguous())       # :1126
    sim = F.log_softmax(sim, dim=-1)                                                          # :1127
    per = [sim[i].diag().mean().view(1) * -1.0 for i in range(sim.size(0))]                   # :1128-1130
    return torch.cat(per).mean()                                                               # :1131


def forward_pretraining_loss_mask(p, batch, num_heads=12, len_vis_input=100, tasks="img2txt",
                                  drop_worst_ratio=0.0, vqa_inference=False, capture=False, mask_image_regions=False, dropout=None):
    """modeling.py:1033-1143 (BertForPreTrainingLossMask.forward).  dropout: None = dropout 0 (not one operation differs), or a mapping
    {site: multiplier tensor} that stands for the reference's nn.Dropout modules of a train() forward: "vis" (:1007), "vispe" (:1018),
    "emb" (:240), ("attn", i) (:296), ("attn_out", i) (:315), ("ffn_out", i) (:355); a missing site is not dropped.  The pretext loss
    reads the dropped projections, as the reference's does; the VQA head, the pooler and the LM head have no dropout.
    mask_image_regions=True: the rows of the projected
    region features / encodings named by batch.vis_masked_pos enter the encoder as zeros (:1049-1056) and the pretext loss
    (:1113-1131) is returned in `vis_pretext_loss` (a 0-dim tensor then, as in the reference).

    Returns a dict: losses (`mlm_loss`, `vis_pretext_loss`, `vqa_loss` shaped like the reference's
    3-tuple) plus the parity capture points `mlm_logits` / `vqa_logits` / `hidden` (list)."""
    dt = p["bert.embeddings.word_embeddings.weight"].dtype
    out = {}
    site = _no_site if dropout is None else dropout.get
    vf = vis_embed(p, batch.img.to(dt), drop=site("vis"))
    vp = vis_pe_embed(p, batch.vis_pe.to(dt), drop=site("vispe"))
    emb_drop = site("emb")
    ext = extended_attention_mask(batch.input_mask, dt)
    if mask_image_regions and not vqa_inference:                   # :1049-1056 (the inference branch returns before it, :1039-1047)
        keep = torch.ones(vf.shape[0], vf.shape[1], 1, dtype=torch.bool, device=vf.device)
        keep.scatter_(1, (batch.vis_masked_pos - 1).unsqueeze(-1), False)
        emb, emb_pre = embeddings(p, vf * keep, vp * keep, batch.input_ids, batch.segment_ids, len_vis_input, drop=emb_drop)
    else:
        emb, emb_pre = embeddings(p, vf, vp, batch.input_ids, batch.segment_ids, len_vis_input, drop=emb_drop)
    hs = encoder(p, emb, ext, num_heads, dropout=dropout)
    seq = hs[-1]
    if capture:
        out.update(vis_feats=vf, vis_pe=vp, emb=emb, emb_pre=emb_pre, hidden=hs)
    out["sequence_output"] = seq

    if vqa_inference:
        logits = vqa_head(p, seq, len_vis_input)
        out["vqa_logits"] = logits
        out["ans_idx"] = torch.max(logits[:, 1:], -1)[1] + 1     # :1046
        return out

    zero1 = seq.new_zeros(1)
    if batch.masked_pos.numel() == 0:
        mlm_loss = zero1.clone()                                   # :1096-1098
    else:
        sel = gather_seq_out_by_pos(seq, batch.masked_pos)
        logits = lm_head(p, sel)
        out["mlm_logits"] = logits
        ce = F.cross_entropy(logits.transpose(1, 2).float(), batch.lm_label_ids, reduction="none")   # :1108
        mlm_loss = loss_mask_and_normalize(ce.float(), batch.masked_weights, drop_worst_ratio)
    if mask_image_regions:
        out["pooled_output"] = pooler(p, seq)
        pretext = vis_pretext_loss(vf, vp, out["pooled_output"], batch.vis_masked_pos)      # :1113-1131 (0-dim)
    else:
        pretext = zero1.clone()                                    # :1133
    if tasks == "vqa2":
        logits = vqa_head(p, seq, len_vis_input)
        out["vqa_logits"] = logits
        vqa_loss = F.binary_cross_entropy_with_logits(logits, batch.ans_labels.to(dt)) * batch.ans_labels.size(1)
        out.update(mlm_loss=zero1.clone(), vis_pretext_loss=pretext, vqa_loss=vqa_loss)   # :1141
    else:
        out.update(mlm_loss=mlm_loss, vis_pretext_loss=pretext, vqa_loss=zero1.clone())  # :1143
    out["loss"] = out["mlm_loss"] + out["vis_pretext_loss"] + out["vqa_loss"]   # run_img2txt_dist.py:531
    return out


# ----------------------------------------------------------------------------------------------
# incremental decoding (reference "next" row N1; restated for later rounds)
# ----------------------------------------------------------------------------------------------
def greedy_decode(p, batch_img, batch_vis_pe, input_ids, token_type_ids, position_ids, attention_mask,
                  mask_word_id, num_heads=12, len_vis_input=100):
    """modeling.py:1189-1253 (sample_mode='greedy', beam size 1) with the hidden-state history
    caches of BertModelIncr/BertEncoder (:856-875, :386-394)."""
    dt = p["bert.embeddings.word_embeddings.weight"].dtype
    vf, vp = vis_embed(p, batch_img.to(dt)), vis_pe_embed(p, batch_vis_pe.to(dt))
    nl = num_layers_of(p)
    in_len, out_len = input_ids.shape[1], token_type_ids.shape[1]
    out_ids, out_probs = [], []
    prev_emb, prev_layers = None, None
    curr_ids = input_ids
    mask_ids = input_ids[:, :1] * 0 + mask_word_id
    next_pos = in_len
    while next_pos < out_len:
        cl = curr_ids.shape[1]
        st = next_pos - cl
        x_ids = torch.cat((curr_ids, mask_ids), dim=1)
        tt = token_type_ids[:, st:next_pos + 1]
        am = attention_mask[:, st:next_pos + 1, :next_pos + 1]
        pid = position_ids[:, st:next_pos + 1]
        ext = extended_attention_mask(am, dt)
        emb, _ = embeddings(p, vf, vp, x_ids, tt, len_vis_input, position_ids=pid, vis_input=(prev_layers is None))
        x, hist, new_layers = emb, prev_emb, []
        for i in range(nl):
            x = bert_layer(p, i, x, ext, num_heads, history=hist)
            new_layers.append(x)
            if prev_layers is not None:
                hist = prev_layers[i]
        logits = lm_head(p, new_layers[-1][:, -1:, :])
        mp, mi = torch.max(logits, dim=-1)
        out_ids.append(mi)
        out_probs.append(mp)
        prev_emb = emb[:, :-1] if prev_emb is None else torch.cat((prev_emb, emb[:, :-1]), dim=1)
        if prev_layers is None:
            prev_layers = [t[:, :-1] for t in new_layers]
        else:
            prev_layers = [torch.cat((a, b[:, :-1]), dim=1) for a, b in zip(prev_layers, new_layers)]
        curr_ids = mi
        next_pos += 1
    return torch.cat(out_ids, dim=1), torch.cat(out_probs, dim=1)


def _incr_step(p, vf, vp, x_ids, tt, pid, am, prev_emb, prev_layers, num_heads, len_vis_input):
    """One incremental forward (BertModelIncr.forward :856-875 + BertEncoder history path :386-394): returns the new
    embedding rows, the new hidden rows of every layer and the LM logits of the last ([MASK]) position."""
    dt = p["bert.embeddings.word_embeddings.weight"].dtype
    ext = extended_attention_mask(am, dt)
    emb, _ = embeddings(p, vf, vp, x_ids, tt, len_vis_input, position_ids=pid, vis_input=(prev_layers is None))
    x, hist, new_layers = emb, prev_emb, []
    for i in range(num_layers_of(p)):
        x = bert_layer(p, i, x, ext, num_heads, history=hist)
        new_layers.append(x)
        if prev_layers is not None:
            hist = prev_layers[i]
    return emb, new_layers, lm_head(p, new_layers[-1][:, -1:, :])


def dup_ngram_candidates(seq, n, ignore=None):
    """modeling.py:1388-1406: words that would complete an n-gram already present in `seq` (sorted)."""
    if len(seq) < n:
        return []
    tail = seq[len(seq) - (n - 1):]
    if ignore and any(t in ignore for t in tail):
        return []
    out = set()
    for i in range(len(seq) - (n - 1)):
        if seq[i:i + n - 1] == tail and not (ignore and seq[i + n - 1] in ignore):
            out.add(seq[i + n - 1])
    return sorted(out)


def beam_backtrack(total_scores, step_ids, step_ptrs, eos_id, length_penalty):
    """modeling.py:1437-1474 for ONE sample: lists over frames of K-lists.  Picks the best finished hypothesis
    (ended by eos, or alive in the last valid frame) by score + length_penalty * length and follows the back pointers."""
    last = len(total_scores) - 1
    for i, w in enumerate(step_ids):
        if all(x == eos_id for x in w):
            last = i
            break
    best, fid_b, pos_b = -math.inf, -1, -1
    for fid in range(last + 1):
        for i, w in enumerate(step_ids[fid]):
            if w == eos_id or fid == last:
                sc = total_scores[fid][i] + length_penalty * (fid + 1)
                if sc > best:
                    best, fid_b, pos_b = sc, fid, i
    if fid_b < 0:
        return [0]
    seq = [step_ids[fid_b][pos_b]]
    for fid in range(fid_b, 0, -1):
        pos_b = step_ptrs[fid][pos_b]
        seq.append(step_ids[fid - 1][pos_b])
    return seq[::-1]


def beam_search(p, batch_img, batch_vis_pe, input_ids, token_type_ids, position_ids, attention_mask, mask_word_id,
                beam_size, eos_id, length_penalty=1.0, min_len=0, forbid_duplicate_ngrams=False, forbid_ignore_set=None,
                ngram_size=3, num_heads=12, len_vis_input=100, want_margins=False):
    """modeling.py:1255-1494 (BertForSeq2SeqDecoder.beam_search).  Returns the traces dict with python lists
    (pred_seq [B][*], scores / wids / ptrs [B][frames][K]); `margins` (optional) holds, per frame and sample, the gap
    between the K-th kept and the best rejected candidate score -- the test uses it to tell a numerical tie from an error."""
    dt = p["bert.embeddings.word_embeddings.weight"].dtype
    vf, vp = vis_embed(p, batch_img.to(dt)), vis_pe_embed(p, batch_vis_pe.to(dt))
    B, in_len = input_ids.shape
    out_len = token_type_ids.shape[1]
    K = beam_size
    V = p["bert.embeddings.word_embeddings.weight"].shape[0]
    curr_ids = input_ids
    mask_ids = torch.full_like(input_ids[:, :1], mask_word_id)
    prev_emb, prev_layers = None, None
    tot, wids, ptrs, eos_flags, margins = [], [], [], [], []
    partial = None
    forbid = None
    logit_scale = 0.0
    next_pos = in_len
    while next_pos < out_len:
        st = next_pos - curr_ids.shape[1]
        x_ids = torch.cat((curr_ids, mask_ids), dim=1)
        emb, new_layers, logits = _incr_step(p, vf, vp, x_ids, token_type_ids[:, st:next_pos + 1], position_ids[:, st:next_pos + 1],
                                             attention_mask[:, st:next_pos + 1, :next_pos + 1], prev_emb, prev_layers, num_heads,
                                             len_vis_input)
        logp = F.log_softmax(logits, dim=-1)                       # [rows, 1, V]
        logit_scale = max(logit_scale, float(logits.abs().max()))
        if forbid is not None:
            logp = logp + forbid * -10000.0
        if min_len and (next_pos - in_len + 1 <= min_len):
            logp[:, :, eos_id] = -10000.0
        kk_s, kk_i = torch.topk(logp, k=K)                         # [rows, 1, K]
        first = not tot
        if first:
            k_s, k_i = kk_s.reshape(B, K), kk_i.reshape(B, K)
            bp = torch.zeros(B, K, dtype=torch.long, device=k_i.device)
            if want_margins:
                kk1 = torch.topk(logp, k=K + 1)[0].reshape(B, K + 1)
                margins.append((kk1[:, K - 1] - kk1[:, K]).tolist())
        else:
            cand = kk_s + eos_flags[-1].reshape(B * K, 1, 1) * -10000.0 + tot[-1].reshape(B * K, 1, 1)
            cand = cand.reshape(B, K * K)
            k_s, sel = torch.topk(cand, k=K)
            bp = sel // K
            k_i = torch.gather(kk_i.reshape(B, K * K), 1, sel)
            if want_margins:
                # candidates beyond each beam's own top-K can never outrank that beam's K-th, so K*K (+1 per beam) suffices
                kk1_s = torch.topk(logp, k=K + 1)[0] + eos_flags[-1].reshape(B * K, 1, 1) * -10000.0 + tot[-1].reshape(B * K, 1, 1)
                allc = torch.sort(kk1_s.reshape(B, K * (K + 1)), dim=1, descending=True)[0]
                margins.append((allc[:, K - 1] - allc[:, K]).tolist())
        tot.append(k_s)
        wids.append(k_i)
        ptrs.append(bp)
        eos_flags.append((k_i == eos_id).to(k_s.dtype))

        def expand(x):                                             # first_expand :1325-1332
            return x.unsqueeze(1).expand(x.shape[0], K, *x.shape[1:]).reshape(x.shape[0] * K, *x.shape[1:])

        def pick(x):                                               # select_beam_items :1334-1349
            xs = x.reshape(B, K, *x.shape[1:])
            idx = bp.reshape(B, K, *([1] * (x.dim() - 1))).expand(B, K, *x.shape[1:])
            return torch.gather(xs, 1, idx).reshape(x.shape)

        if first:
            prev_emb = expand(emb[:, :-1])
            prev_layers = [expand(t[:, :-1]) for t in new_layers]
            token_type_ids, position_ids, attention_mask, mask_ids = (expand(t) for t in (token_type_ids, position_ids, attention_mask,
                                                                                          mask_ids))
        else:
            prev_emb = pick(torch.cat((prev_emb, emb[:, :-1]), dim=1))
            prev_layers = [pick(torch.cat((a, b[:, :-1]), dim=1)) for a, b in zip(prev_layers, new_layers)]
        curr_ids = k_i.reshape(B * K, 1)

        if forbid_duplicate_ngrams:                                # :1367-1430
            w, q = k_i.tolist(), bp.tolist()
            if first:
                partial = [[w[b][k]] for b in range(B) for k in range(K)]
            else:
                partial = [partial[q[b][k] + b * K] + [w[b][k]] for b in range(B) for k in range(K)]
            forbid = None
            if len(partial[0]) >= ngram_size:
                cands = [dup_ngram_candidates(sq, ngram_size, forbid_ignore_set) for sq in partial]
                if max(len(c) for c in cands) > 0:
                    fm = torch.zeros(B * K, 1, V, dtype=logp.dtype, device=logp.device)
                    for r, c in enumerate(cands):
                        for wid in c:
                            fm[r, 0, wid] = 1.0
                    forbid = fm
        next_pos += 1

    tot_l = [t.tolist() for t in tot]
    wid_l = [t.tolist() for t in wids]
    ptr_l = [t.tolist() for t in ptrs]
    traces = {"pred_seq": [], "scores": [], "wids": [], "ptrs": []}
    for b in range(B):
        sc, ww, pp = [x[b] for x in tot_l], [x[b] for x in wid_l], [x[b] for x in ptr_l]
        traces["scores"].append(sc)
        traces["wids"].append(ww)
        traces["ptrs"].append(pp)
        traces["pred_seq"].append(beam_backtrack(sc, ww, pp, eos_id, length_penalty))
    if want_margins:
        traces["margins"] = [[m[b] for m in margins] for b in range(B)]
        traces["logit_scale"] = logit_scale
    return traces


def pad_traces(traces, out_len, device=None):
    """modeling.py:1476-1494: lists -> zero-padded tensors [B, out_len, ...] (what the reference's forward returns)."""
    out = {}
    for k in ("pred_seq", "scores", "wids", "ptrs"):
        ts = [torch.tensor(t, dtype=torch.float if k == "scores" else torch.long) for t in traces[k]]
        buf = ts[0].new_zeros((len(ts), out_len) + tuple(ts[0].shape[1:]))
        for i, t in enumerate(ts):
            buf[i, :t.shape[0]] = t
        out[k] = buf if device is None else buf.to(device)
    return out


# ----------------------------------------------------------------------------------------------
# optimizers
# ----------------------------------------------------------------------------------------------
def warmup_linear(x, warmup=0.002):
    """optimization.py:45-48."""
    if x < warmup:
        return x / warmup
    return max((x - 1.) / (warmup - 1.), 0)


def warmup_constant(x, warmup=0.002):
    """optimization.py:39-42."""
    return x / warmup if x < warmup else 1.0


def warmup_cosine(x, warmup=0.002):
    """optimization.py:33-36."""
    if x < warmup:
        return x / warmup
    return 0.5 * (1.0 + math.cos(math.pi * x))


SCHEDULES = {"warmup_cosine": warmup_cosine, "warmup_constant": warmup_constant, "warmup_linear": warmup_linear}


def bert_adam_step(p, g, m, v, step, lr, warmup=-1, t_total=-1, schedule="warmup_linear", b1=0.9, b2=0.999,
                   e=1e-6, weight_decay=0.01, max_grad_norm=1.0):
    """optimization.py:112-182 for ONE parameter tensor; updates p, m, v in place, returns step+1.
    Note the clip is per parameter tensor (:146-147, clip_grad_norm_ on the single tensor: coefficient
    max_norm / (norm + 1e-6), applied only when < 1) and there is no bias correction (:177-180)."""
    g = g.clone()
    if max_grad_norm > 0:
        norm = g.norm(2)
        coef = max_grad_norm / (norm + 1e-6)
        if coef < 1:
            g.mul_(coef)
    m.mul_(b1).add_(g, alpha=1 - b1)
    v.mul_(b2).addcmul_(g, g, value=1 - b2)
    update = m / (v.sqrt() + e)
    if weight_decay > 0.0:
        update = update + weight_decay * p
    lr_s = lr * SCHEDULES[schedule](step / t_total, warmup) if t_total != -1 else lr
    p.add_(-lr_s * update)
    return step + 1


def fused_adam_step(p32, g16_scaled, m, v, lr, grad_norm_scaled, scale, b1=0.9, b2=0.999, eps=1e-8,
                    weight_decay=0.0, max_grad_norm=1.0, step=1, bias_correction=False,
                    eps_inside_sqrt=False):
    """apex FusedAdam.step + fused_adam_cuda kernel as configured at run_img2txt_dist.py:411-414
    (bias_correction=False, max_grad_norm=1.0, eps 1e-8) for ONE param group whose gradient is the
    flat fp16 tensor `g16_scaled` (still multiplied by the loss scale) with L2 norm
    `grad_norm_scaled`.  **parity unpinned** (apex @1603407 is not in /root/reference):
        clip = (norm/scale + 1e-6) / max_grad_norm ; combined_scale = scale * max(clip, 1)
        g = g16/combined_scale ; m = b1 m + (1-b1) g ; v = b2 v + (1-b2) g^2
        denom = sqrt(v + eps) if eps_inside_sqrt else sqrt(v) + eps
        p -= step_size * (m/denom + decay*p) ; p16 = half(p)
    Returns the fp16 copy of the updated master weights."""
    combined = scale
    if max_grad_norm > 0:
        clip = ((grad_norm_scaled / scale) + 1e-6) / max_grad_norm
        if clip > 1:
            combined = clip * scale
    if bias_correction:
        step_size = lr * math.sqrt(1 - b2 ** step) / (1 - b1 ** step)
    else:
        step_size = lr
    g = g16_scaled.float() / combined
    m.mul_(b1).add_(g, alpha=1 - b1)
    v.mul_(b2).add_(g * g, alpha=1 - b2)
    denom = torch.sqrt(v + eps) if eps_inside_sqrt else torch.sqrt(v) + eps
    p32.sub_(step_size * (m / denom + weight_decay * p32))
    return p32.half()


class LossScaler(object):
    """apex FP16_Optimizer (the FusedAdam-only variant) dynamic loss-scale bookkeeping, as wrapped
    by optimization_fp16.py:7-80 (state_dict fields :28-37).  **parity unpinned** (apex absent):
    init scale 2**16, x2 every `scale_window`=1000 clean iterations, /2 (floor 1) on overflow."""

    def __init__(self, dynamic=True, static_loss_scale=1.0, init_scale=2 ** 16, scale_factor=2, scale_window=1000):
        self.dynamic = dynamic
        self.cur_scale = init_scale if dynamic else static_loss_scale
        self.cur_iter = 0
        self.last_overflow_iter = -1
        self.scale_factor = scale_factor
        self.scale_window = scale_window

    def update(self, overflow):
        if self.dynamic:
            if overflow:
                self.cur_scale = max(self.cur_scale / self.scale_factor, 1)
                self.last_overflow_iter = self.cur_iter
            elif (self.cur_iter - self.last_overflow_iter) % self.scale_window == 0:
                self.cur_scale *= self.scale_factor
        self.cur_iter += 1


# ----------------------------------------------------------------------------------------------
# helpers for tests / bench
# ----------------------------------------------------------------------------------------------
def params_from_state_dict(sd, dtype=torch.float32, requires_grad=False):
    """Clone a reference-keyed state_dict into oracle parameters.  The tied decoder weight
    (cls.predictions.decoder.weight, modeling.py:445-448) is dropped: lm_head() reads the word
    embedding table directly so autograd accumulates both uses into one gradient."""
    p = {}
    for k, t in sd.items():
        if k == "cls.predictions.decoder.weight":
            continue
        t = t.detach().to(dtype).clone()
        if requires_grad:
            t.requires_grad_(True)
        p[k] = t
    return p


def init_params(vocab_size=28996, hidden=768, layers=12, inter=3072, max_pos=512, type_vocab=6,
                tasks="img2txt", feat_dim=2048, pe_dim=1607, num_answers=3129, seed=0, std=0.02,
                dtype=torch.float32):
    """Random parameters with the reference's shapes and init law (modeling.py:539-551:
    N(0, initializer_range) weights, zero biases, unit LayerNorm), keyed like its state_dict."""
    g = torch.Generator().manual_seed(seed)

    def w(*shape):
        return (torch.randn(*shape, generator=g) * std).to(dtype)

    def z(*shape):
        return torch.zeros(*shape, dtype=dtype)

    def o(*shape):
        return torch.ones(*shape, dtype=dtype)

    p = {}
    p["bert.embeddings.word_embeddings.weight"] = w(vocab_size, hidden)
    p["bert.embeddings.position_embeddings.weight"] = w(max_pos, hidden)
    p["bert.embeddings.token_type_embeddings.weight"] = w(type_vocab, hidden)
    p["bert.embeddings.LayerNorm.weight"], p["bert.embeddings.LayerNorm.bias"] = o(hidden), z(hidden)
    for i in range(layers):
        L = "bert.encoder.layer.%d." % i
        for n in ("query", "key", "value"):
            p[L + "attention.self.%s.weight" % n], p[L + "attention.self.%s.bias" % n] = w(hidden, hidden), z(hidden)
        p[L + "attention.output.dense.weight"], p[L + "attention.output.dense.bias"] = w(hidden, hidden), z(hidden)
        p[L + "attention.output.LayerNorm.weight"], p[L + "attention.output.LayerNorm.bias"] = o(hidden), z(hidden)
        p[L + "intermediate.dense.weight"], p[L + "intermediate.dense.bias"] = w(inter, hidden), z(inter)
        p[L + "output.dense.weight"], p[L + "output.dense.bias"] = w(hidden, inter), z(hidden)
        p[L + "output.LayerNorm.weight"], p[L + "output.LayerNorm.bias"] = o(hidden), z(hidden)
    p["bert.pooler.dense.weight"], p["bert.pooler.dense.bias"] = w(hidden, hidden), z(hidden)
    p["cls.predictions.bias"] = z(vocab_size)
    p["cls.predictions.transform.dense.weight"], p["cls.predictions.transform.dense.bias"] = w(hidden, hidden), z(hidden)
    p["cls.predictions.transform.LayerNorm.weight"], p["cls.predictions.transform.LayerNorm.bias"] = o(hidden), z(hidden)
    p["vis_embed.0.weight"], p["vis_embed.0.bias"] = w(feat_dim, feat_dim), w(feat_dim)
    p["vis_embed.2.weight"], p["vis_embed.2.bias"] = w(hidden, feat_dim), z(hidden)
    p["vis_pe_embed.0.weight"], p["vis_pe_embed.0.bias"] = w(hidden, pe_dim), z(hidden)
    if tasks == "vqa2":
        p["ans_classifier.0.weight"], p["ans_classifier.0.bias"] = w(hidden * 2, hidden), z(hidden * 2)
        p["ans_classifier.2.weight"], p["ans_classifier.2.bias"] = w(num_answers, hidden * 2), z(num_answers)
    return p


def loss_and_grads(p, batch, **kw):
    """Forward + autograd backward of the summed loss (run_img2txt_dist.py:531,575).  `p` must hold
    leaf tensors with requires_grad; dropout={site: multiplier} goes to the forward.  Returns (out dict, {key: grad or None})."""
    out = forward_pretraining_loss_mask(p, batch, **kw)
    out["loss"].sum().backward()
    return out, {k: t.grad for k, t in p.items()}
