"""GPU: self-critical sequence training (--scst) on the fused HIP path.

(1) vlp_scst_layout bit-exact against the Python mirror of tests/test_scst_cpu.py (pinned there against the incremental decoder in fp64);
(2) vlp_token_logprob_fwd / _bwd against fp64 torch on the same fp16 logits;
(3) vlp_embed_bwd_pos against an fp64 index_add, run-to-run bitwise, and bit-equal to vlp_embed_bwd for position ids 0..L-1;
(4) BertForSeq2SeqDecoder(sample_mode='sample') in train() mode: its log-probs against the decoder's own sampled log-probs and the oracle's
    forced decode (fp32 on the fp16-rounded weights), every parameter gradient of RewardCriterion against the oracle's autograd; eval() /
    no_grad keep the plain decoder; the scoring pass runs dense and silent under every varlen setting;
(5) the entry script: a CE epoch, then --scst epochs from its checkpoint (single process, RCCL world 1, --packed_features), resume.
Every test prints what it measured (pytest -s)."""
import json
import os
import re

import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from oracle import vlp_oracle as O                                                 # noqa: E402  (checker only)
from tests.test_scst_cpu import forced_decode_logp, layout_mirror, scst_inputs     # noqa: E402
from vlp_amd import _lib as K                                                      # noqa: E402
from vlp_amd import scst as SC                                                     # noqa: E402
from vlp_amd import synthetic as S                                                 # noqa: E402
from vlp_amd.modeling import BertConfig, BertForSeq2SeqDecoder                     # noqa: E402

DEV = torch.device("cuda:0")
REPORT = {}


def report(key, **kw):
    REPORT.setdefault(key, {}).update(kw)
    print("%s: %s" % (key, json.dumps(REPORT[key], sort_keys=True)))


def rel(a, b):
    """max(max-normalised error, relative L2 error) -- the metric of tests/test_70_label_smoothing_gpu.py."""
    a, b = a.detach().double(), b.detach().double()
    d = a - b
    return max(float(d.abs().max() / (b.abs().max() + 1e-30)), float(d.norm() / (b.norm() + 1e-30)))


# =====================================================================================================================================
# (1) - (3) kernels
# =====================================================================================================================================
@pytest.mark.parametrize("B,max_len_b,seed", [(1, 1, 1), (3, 6, 2), (5, 20, 3), (16, 20, 4)])
def test_scst_layout_bit_exact(B, max_len_b, seed):
    img, vis_pe, prefix, seg, pos, am, sample, _ = scst_inputs(B, max_len_b, seed, 28996, short=(0,) if B > 2 else (),
                                                               ragged=((B - 1, 17),), pos_offset=seed)
    am[:, 3, 7] = 2                                   # an arbitrary value is copied, not normalised
    dv = [t.to(DEV).contiguous() for t in (prefix, sample, seg, pos, am)]
    want = layout_mirror(*dv, S.MASK_ID)
    got = [torch.full_like(w, -5) for w in want]
    K.scst_layout(*dv, *got, S.MASK_ID)
    torch.cuda.synchronize()
    for g, w in zip(got, want):
        assert torch.equal(g, w)


def test_scst_layout_refuses_too_long():
    B, in_len, T = 1, 102, 78
    L = in_len + T
    Lo = in_len + 2 * T - 1

    def z(*s):
        return torch.zeros(*s, dtype=torch.long, device=DEV)
    with pytest.raises(RuntimeError, match="256"):
        K.scst_layout(z(B, in_len), z(B, T), z(B, L), z(B, L), z(B, L, L), z(B, Lo), z(B, Lo), z(B, Lo), z(B, Lo, Lo), z(B, T), S.MASK_ID)


def test_token_logprob_kernels():
    g = torch.Generator(device=DEV)
    g.manual_seed(11)
    V, ld, R = 28996, 29056, 48
    logits = torch.full((R, ld), 30.0, device=DEV, dtype=torch.half)            # pad columns: large values the kernels must not see
    logits[:, :V] = (torch.randn(R, V, device=DEV, generator=g) * 3.0).half()
    ids = torch.randint(0, V, (R,), device=DEV, generator=g)
    ids[0], ids[1] = 0, V - 1
    logp, lse = torch.zeros(R, device=DEV), torch.zeros(R, device=DEV)
    K.token_logprob_fwd(logits, ld, ids, logp, lse, R, V)
    x = logits[:, :V].double()
    want = torch.log_softmax(x, -1).gather(1, ids.view(-1, 1)).view(-1)
    e_f = float((logp.double() - want).abs().max())
    grow = torch.randn(R, device=DEV, generator=g) * 512.0                        # signed, loss-scaled
    dl = torch.full((R, ld), 7.0, device=DEV, dtype=torch.half)
    K.token_logprob_bwd(logits, ld, ids, lse, grow, dl, ld, R, V)
    onehot = torch.zeros_like(x).scatter_(1, ids.view(-1, 1), 1.0)
    want_d = grow.double().view(-1, 1) * (onehot - torch.softmax(x, -1))
    e_b = rel(dl[:, :V], want_d)
    report("token_logprob", fwd_abs=e_f, bwd_rel=e_b)
    assert e_f < 1e-4
    assert e_b < 2e-3
    assert bool((dl[:, V:] == 0).all())


def _embed_case(B, L, Nv, H, seed, pid):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    V, TV, MP = 300, 6, 512
    dpre = (torch.randn(B * L, H, device=DEV, generator=g)).half()
    ids = torch.randint(0, V, (B, L), device=DEV, generator=g)
    seg = torch.randint(0, TV, (B, L), device=DEV, generator=g)
    vis = torch.randn(B * Nv, H, device=DEV, generator=g).half()
    vpe = torch.randn(B * Nv, H, device=DEV, generator=g).half()
    init_pos = (torch.randn(MP, H, device=DEV, generator=g) * 0.1).half()
    outs = []
    for fn in ("pos", "plain"):
        dw, dp, dt = torch.zeros(V, H, device=DEV, dtype=torch.half), init_pos.clone(), torch.zeros(TV, H, device=DEV, dtype=torch.half)
        dvh, dvp = torch.zeros(B * Nv, H, device=DEV, dtype=torch.half), torch.zeros(B * Nv, H, device=DEV, dtype=torch.half)
        acc = torch.zeros(K.embed_bwd_workspace_floats(B, L, Nv, H), device=DEV)
        if fn == "pos":
            K.embed_bwd_pos(dpre, ids, seg, pid, vis, vpe, dw, dp, dt, dvh, dvp, acc, B, L, Nv, H, V, TV)
        else:
            K.embed_bwd(dpre, ids, seg, vis, vpe, dw, dp, dt, dvh, dvp, acc, B, L, Nv, H, V, TV)
        outs.append((dw, dp, dt, dvh, dvp))
    torch.cuda.synchronize()
    return dpre, init_pos, outs


def test_embed_bwd_pos():
    B, L, Nv, H = 6, 143, 100, 768
    g = torch.Generator(device=DEV)
    g.manual_seed(3)
    pid = torch.randint(0, 200, (B, L), device=DEV, generator=g)
    pid[:, 0] = 511
    pid[0, 101:106] = torch.tensor([-3, -1, 512, 515, 1 << 40], device=DEV)      # clamped to [0, max_pos) like vlp_embed_fwd
    dpre, init_pos, outs = _embed_case(B, L, Nv, H, 5, pid)
    tok = torch.tensor([l == 0 or l > Nv for l in range(L)], device=DEV).repeat(B)
    want = init_pos.double().index_add(0, pid.clamp(0, 511).view(-1)[tok], dpre.double()[tok])
    e = rel(outs[0][1], want)
    _, _, outs2 = _embed_case(B, L, Nv, H, 5, pid)
    report("embed_bwd_pos", rel=e)
    assert e < 2e-3
    for a, b in zip(outs[0], outs2[0]):
        assert torch.equal(a, b)                                        # bitwise reproducible
    for i in (0, 2, 3, 4):
        assert torch.equal(outs[0][i], outs[1][i])                      # word / type tables and region rows: vlp_embed_bwd's
    ar = torch.arange(L, device=DEV).unsqueeze(0).expand(B, L).contiguous()
    _, _, outs3 = _embed_case(B, L, Nv, H, 9, ar)
    for a, b in zip(outs3[0], outs3[1]):
        assert torch.equal(a, b)                                        # arange positions: vlp_embed_bwd's bits


# =====================================================================================================================================
# (4) the model
# =====================================================================================================================================
def _decoder(p, V, layers):
    cfg = BertConfig(V, num_hidden_layers=layers, type_vocab_size=6, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    m = BertForSeq2SeqDecoder(cfg, mask_word_id=S.MASK_ID, eos_id=S.SEP_ID, enable_butd=True, len_vis_input=100)
    sd = dict(p)
    sd["cls.predictions.decoder.weight"] = p["bert.embeddings.word_embeddings.weight"]
    m.load_state_dict(sd, strict=True)
    return m.half().to(DEV)


def _model_case(V, layers, B, max_len_b, seed, std, bounds):
    p = O.init_params(vocab_size=V, layers=layers, seed=seed, std=std)
    m = _decoder(p, V, layers)
    img, vis_pe, prefix, seg, pos, am, _, _ = scst_inputs(B, max_len_b, seed, V, short=(1,), ragged=((0, 41),), pos_offset=2)
    dv = [t.to(DEV) for t in (img, vis_pe, prefix, seg, pos, am)]
    img16, vpe16 = dv[0].half(), dv[1].half()
    eng = m.engine
    m.train()
    s0 = eng.step_seed
    with torch.no_grad():                                   # the decoder's own draw and log-probs (same seeds as the call below)
        ids_d, lp_d = eng.decode_greedy(img16, vpe16, dv[2], dv[3], dv[4], dv[5], S.MASK_ID, sample=True)
    eng.step_seed = s0
    ids, logp = m(img16, vpe16, *dv[2:], sample_mode="sample")
    assert logp.requires_grad and logp.grad_fn is not None
    assert torch.equal(ids, ids_d)
    T = ids.shape[1]
    gen = SC.clean_captions(ids, S.SEP_ID)
    g = torch.Generator().manual_seed(seed)
    reward = (torch.randn(B, 1, generator=g) * 2.0).expand(B, T).to(DEV)
    eng.zero_grad()
    loss = SC.RewardCriterion()(logp, gen, reward)
    (loss * 1024.0).backward()
    torch.cuda.synchronize()
    grads = {n: (q.grad.float() / 1024.0) for n, q in m.named_parameters()}
    # oracle: fp32 forced incremental decode on the fp16-rounded weights, autograd
    pd = {k: v.to(DEV).half().float().requires_grad_(True) for k, v in p.items()}
    vf, vp = O.vis_embed(pd, img16.float()), O.vis_pe_embed(pd, vpe16.float())
    lp_o = forced_decode_logp(pd, vf, vp, *dv[2:], ids, S.MASK_ID)
    SC.RewardCriterion()(lp_o, gen, reward).backward()
    e_self = float((logp.detach() - lp_d).abs().max())
    e_lp = float((logp.detach() - lp_o.detach()).abs().max())
    errs = {}
    for k, t in pd.items():
        if t.grad is None:
            continue
        if k.endswith("attention.self.key.bias"):     # true value 0: bounded against the sibling query-bias gradient (as test_70 does)
            d, qb = (grads[k] - t.grad).double(), pd[k.replace("key.bias", "query.bias")].grad.double()
            errs[k] = max(float(d.abs().max() / qb.abs().max()), float(d.norm() / qb.norm()))
        else:
            errs[k] = rel(grads[k], t.grad)
    assert {k for k, t in pd.items() if t.grad is None} <= eng.unused_parameter_names()
    worst = max(errs, key=errs.get)
    report("model_%d_%d" % (V, layers), logp_vs_decoder=e_self, logp_vs_oracle=e_lp, worst_grad=worst, worst_grad_rel=errs[worst], T=T, B=B,
           loss=float(loss.detach()))
    assert e_self < bounds[0], e_self
    assert e_lp < bounds[1], e_lp
    assert errs[worst] < bounds[2], (worst, errs[worst])
    return m, dv


def test_small_model_sample_logprobs_and_every_gradient_vs_oracle():
    m, dv = _model_case(1024, 3, 5, 12, 21, 0.05, (0.0048, 0.0036, 0.07))    # measured on MI355X: 0.0040, 0.0029, 0.058
    # eval() or no_grad: no scoring pass, the plain decoder bit for bit
    eng = m.engine
    gen0 = eng.gen
    m.eval()
    a = m(dv[0].half(), dv[1].half(), *dv[2:], sample_mode="greedy")
    b = eng.decode_greedy(dv[0].half(), dv[1].half(), *dv[2:], S.MASK_ID)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    s0 = eng.step_seed
    c = m(dv[0].half(), dv[1].half(), *dv[2:], sample_mode="sample")
    assert not c[1].requires_grad
    m.train()
    eng.step_seed = s0
    with torch.no_grad():
        d = m(dv[0].half(), dv[1].half(), *dv[2:], sample_mode="sample")
    assert torch.equal(c[0], d[0]) and torch.equal(c[1], d[1]) and not d[1].requires_grad
    assert eng.gen == gen0                                 # no training forward ran


def test_full_size_sample_logprobs_and_gradients_vs_oracle():
    _model_case(28996, 12, 16, 20, 5, 0.02, (0.003, 0.003, 0.0088))            # measured on MI355X: 0.0024, 0.0024, 0.0073


@pytest.mark.parametrize("varlen", [True, "auto"])
def test_scoring_pass_runs_dense_and_silent(varlen):
    """score_samples never takes the padding-free step (its fresh dense mask would need a read-back) and emits no VlpPerformanceWarning,
    whatever the engine's varlen setting; the same batch's scoring mask has unattended key columns (a short ground truth), so a packed
    forward would have been possible."""
    import warnings
    from vlp_amd.engine import VlpPerformanceWarning
    p = O.init_params(vocab_size=1024, layers=2, seed=4, std=0.05)
    m = _decoder(p, 1024, 2).train()
    eng = m.engine
    eng.varlen = varlen
    eng.varlen_readback_budget = 0
    img, vis_pe, prefix, seg, pos, am, _, _ = scst_inputs(4, 8, 6, 1024, short=(1, 2))
    dv = [t.to(DEV) for t in (img, vis_pe, prefix, seg, pos, am)]
    eng.last_packed_rows = -1
    with warnings.catch_warnings():
        warnings.simplefilter("error", VlpPerformanceWarning)
        ids, logp = m(dv[0].half(), dv[1].half(), *dv[2:], sample_mode="sample")
        logp.sum().backward()
    torch.cuda.synchronize()
    assert eng.last_packed_rows is None
    assert bool(torch.isfinite(logp).all())


def test_decoder_trains_with_fp16_optimizer():
    from vlp_amd.optimization_fp16 import FP16_Optimizer_State, FusedAdam
    p = O.init_params(vocab_size=1024, layers=2, seed=4, std=0.05)
    m = _decoder(p, 1024, 2).train()
    named = list(m.named_parameters())
    nd = ["bias", "LayerNorm.bias", "LayerNorm.weight"]
    groups = [{"params": [q for n, q in named if not any(x in n for x in nd)], "weight_decay": 0.01},
              {"params": [q for n, q in named if any(x in n for x in nd)], "weight_decay": 0.0}]
    opt = FP16_Optimizer_State(FusedAdam(groups, lr=1e-3, bias_correction=False, max_grad_norm=1.0), dynamic_loss_scale=True)
    img, vis_pe, prefix, seg, pos, am, _, _ = scst_inputs(4, 8, 6, 1024)
    dv = [t.to(DEV) for t in (img, vis_pe, prefix, seg, pos, am)]
    before = {n: q.detach().clone() for n, q in named}
    ids, logp = m(dv[0].half(), dv[1].half(), *dv[2:], sample_mode="sample")
    loss = SC.RewardCriterion()(logp, SC.clean_captions(ids, S.SEP_ID), torch.ones_like(logp))
    opt.backward(loss)
    opt.step()
    opt.zero_grad()
    torch.cuda.synchronize()
    changed = [n for n, q in named if not torch.equal(q.detach(), before[n])]
    assert "bert.embeddings.word_embeddings.weight" in changed and "bert.encoder.layer.0.attention.self.query.weight" in changed
    assert "bert.embeddings.position_embeddings.weight" in changed and "vis_embed.0.weight" in changed


# =====================================================================================================================================
# (5) the entry script
# =====================================================================================================================================
BASE = ["--do_train", "--fp16", "--enable_butd", "--new_segment_ids", "--max_len_b", "20", "--train_batch_size", "4", "--num_hidden_layers", "2",
        "--len_vis_input", "100", "--log_every", "1", "--max_pred", "0", "--mask_prob", "0"]


def _signed_reward(monkeypatch):
    """The real CIDEr-D reward + a fixed signed offset per sample.  A 2-layer model after one synthetic CE epoch rarely shares an
    informative n-gram with its ground truth, so the true reward (hence the gradient) is often exactly 0; the offset makes every step move
    the parameters, which is what the DDP / optimizer checks below look for."""
    import numpy as np
    real = SC.self_critical_reward

    def reward(greedy, gt, gen, B, scorer=None):
        r, scores = real(greedy, gt, gen, B, scorer)
        return r + np.where(np.arange(B) % 2 == 0, 0.5, -0.75)[:, None], scores
    monkeypatch.setattr(SC, "self_critical_reward", reward)


def _ce_checkpoint(R, tmp_path):
    out = os.path.join(tmp_path, "ce")
    R.main(BASE[:-4] + ["--from_scratch", "--synthetic", "2", "--output_dir", out, "--num_train_epochs", "1"])
    return os.path.join(out, "model.1.bin")


def test_entry_script_scst_trains_and_resumes(tmp_path):
    from vlp_amd import run_img2txt_dist as R
    ckpt = _ce_checkpoint(R, tmp_path)
    out = os.path.join(tmp_path, "scst")
    argv = BASE + ["--scst", "--synthetic", "3", "--learning_rate", "1e-4", "--model_recover_path", ckpt, "--output_dir", out,
                   "--num_train_epochs", "2", "--stop_after_epoch", "1"]
    R.main(argv)
    log = open(os.path.join(out, "training.log")).read()
    losses = [float(x) for x in re.findall(r"Loss (\S+), Mean R", log)]
    assert len(losses) == 3 and all(abs(v) < 1e4 for v in losses), log
    ce = torch.load(ckpt)
    sd = torch.load(os.path.join(out, "model.1.bin"))
    cfg = BertConfig(28996, num_hidden_layers=2, type_vocab_size=6)
    keys = set(BertForSeq2SeqDecoder(cfg, mask_word_id=S.MASK_ID, eos_id=S.SEP_ID, enable_butd=True, len_vis_input=100).state_dict())
    assert set(sd) == keys
    assert not torch.equal(sd["bert.encoder.layer.0.attention.self.query.weight"], ce["bert.encoder.layer.0.attention.self.query.weight"])
    report("entry_scst", losses=losses, mean_r=re.findall(r"Mean R (\S+)", log))
    R.main(argv[:-2])                                     # resume: epoch 2 from model.1.bin / optim.1.bin
    assert os.path.exists(os.path.join(out, "model.2.bin"))
    assert "Recover optimizer: 1" in open(os.path.join(out, "training.log")).read()


def test_entry_script_scst_rccl_world_1(tmp_path, monkeypatch):
    from vlp_amd import run_img2txt_dist as R
    ckpt = _ce_checkpoint(R, tmp_path)
    _signed_reward(monkeypatch)
    out = os.path.join(tmp_path, "dist")
    R.main(BASE + ["--scst", "--synthetic", "2", "--learning_rate", "1e-4", "--model_recover_path", ckpt, "--output_dir", out,
                   "--num_train_epochs", "1", "--local_rank", "0", "--global_rank", "0", "--world_size", "1"])
    log = open(os.path.join(out, "training.log")).read()
    losses = [float(x) for x in re.findall(r"Loss (\S+), Mean R", log)]
    assert len(losses) == 2 and all(abs(v) < 1e4 for v in losses), log
    ce, sd = torch.load(ckpt), torch.load(os.path.join(out, "model.1.bin"))
    for k in ("bert.encoder.layer.0.attention.self.query.weight", "bert.embeddings.word_embeddings.weight", "vis_embed.0.weight"):
        assert not torch.equal(sd[k], ce[k]), k                   # gradients went through the DDP reducer's buckets into the optimizer
    report("entry_scst_rccl", losses=losses)


def test_entry_script_scst_from_packed_features(tmp_path, monkeypatch):
    """--scst --packed_features: the packed loader's batches (MaskSpec masks, raw region boxes) through both decodes and the scoring pass."""
    from tests.test_60_data_gpu import make_store
    from vlp_amd import run_img2txt_dist as R
    monkeypatch.setenv("VLP_ALLOW_RANDOM_FC7", "1")
    ckpt = _ce_checkpoint(R, tmp_path)
    _signed_reward(monkeypatch)
    store_dir = os.path.join(tmp_path, "store")
    os.makedirs(store_dir)
    _, examples, *_ = make_store(store_dir, n=12, seed=2)
    tok = os.path.join(tmp_path, "tokens.json")
    json.dump([[i, t] for i, t in examples[:12]], open(tok, "w"))
    out = os.path.join(tmp_path, "packed")
    R.main(BASE + ["--scst", "--learning_rate", "1e-4", "--model_recover_path", ckpt, "--output_dir", out, "--num_train_epochs", "1",
                   "--packed_features", store_dir,
                   "--token_file", tok, "--always_truncate_tail", "--num_workers", "1"])
    log = open(os.path.join(out, "training.log")).read()
    losses = [float(x) for x in re.findall(r"Loss (\S+), Mean R", log)]
    assert len(losses) == 3 and all(abs(v) < 1e4 for v in losses), log
    sd = torch.load(os.path.join(out, "model.1.bin"))
    assert not torch.equal(sd["vis_pe_embed.0.weight"], torch.load(ckpt)["vis_pe_embed.0.weight"])
    report("entry_scst_packed", losses=losses)
