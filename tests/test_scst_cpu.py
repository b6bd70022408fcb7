"""CPU: self-critical sequence training (--scst) -- the CIDEr-D reward, the criterion, the scoring layout's math and the entry script's checks.

(1) vlp_amd.scst.CiderD from its published definition: a fixed check value, exact / disjoint / corpus-wide n-grams, the Gaussian length
    factor, the bigram length rule and the scorer's argument checks;
(2) where the reference tree is present: its UNMODIFIED vlp/scst_utils.py (after vlp_amd.compat.install(), which stands in for the
    coco-caption scorer) equals vlp_amd.scst on random id tensors;
(3) the scoring layout (a Python mirror of include/vlp_hip.h vlp_scst_layout, also the GPU tests' reference): the oracle's training forward
    on it equals the oracle's forced incremental decode in fp64 -- log-probs and every parameter gradient of RewardCriterion; where the
    reference tree is present, that forced decode in turn equals the UNMODIFIED reference decoder's train-mode sample_mode='sample' call
    (ids, log-probs and every gradient);
(4) the entry script's argument checks (run_img2txt_dist.py:200-204, :322)."""
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

from oracle import ref_loader
from oracle import vlp_oracle as O                       # checker only
from vlp_amd import scst as SC
from vlp_amd import synthetic as S

REF = ref_loader.REFERENCE_ROOT                          # VLP_REFERENCE_ROOT


# =====================================================================================================================================
# helpers shared with tests/test_80_scst_gpu.py
# =====================================================================================================================================
def layout_mirror(prefix, sample, seg, pos, am, mask_id):
    """The scoring sequence of vlp_scst_layout: (ids, segment ids, position ids [B, L'], mask [B, L', L'], masked_pos [B, T])."""
    B, in_len = prefix.shape
    T = sample.shape[1]
    nr = in_len + T - 1
    Lo = nr + T
    dev = prefix.device
    lg = torch.cat((torch.arange(nr, device=dev), torch.arange(in_len, in_len + T, device=dev)))
    is_m = torch.arange(Lo, device=dev) >= nr
    ids = torch.cat((prefix, sample[:, :T - 1], torch.full((B, T), int(mask_id), dtype=torch.long, device=dev)), dim=1)
    pi, pk = lg.view(Lo, 1), lg.view(1, Lo)
    mi, mk = is_m.view(Lo, 1), is_m.view(1, Lo)
    eye = torch.eye(Lo, dtype=torch.bool, device=dev)
    cond = torch.where(~mi & ~mk, pk <= torch.clamp(pi, min=in_len - 1),
                       torch.where(~mi & mk, pk == torch.clamp(pi + 1, min=in_len), torch.where(mi & ~mk, pk <= pi - 1, eye)))
    m = am[:, lg][:, :, lg]
    mask = torch.where(cond.unsqueeze(0), m, torch.zeros_like(m))
    mpos = torch.arange(nr, Lo, device=dev).unsqueeze(0).expand(B, T).contiguous()
    return ids, seg[:, lg].contiguous(), pos[:, lg].contiguous(), mask.contiguous(), mpos


def forced_decode_logp(p, vf, vp, input_ids, token_type_ids, position_ids, am, sample_ids, mask_id, num_heads=12, Nv=100):
    """The reference decoder's incremental forward (modeling.py:1210-1251, oracle _incr_step) fed the given sampled ids: log_softmax of
    every step's [MASK] logits at the sampled id [B, T]."""
    in_len, out_len = input_ids.shape[1], token_type_ids.shape[1]
    prev_emb = prev_layers = None
    curr = input_ids
    mask_ids = input_ids[:, :1] * 0 + mask_id
    out, t, next_pos = [], 0, in_len
    while next_pos < out_len:
        st = next_pos - curr.shape[1]
        x_ids = torch.cat((curr, mask_ids), dim=1)
        emb, new_layers, logits = O._incr_step(p, vf, vp, x_ids, token_type_ids[:, st:next_pos + 1], position_ids[:, st:next_pos + 1],
                                               am[:, st:next_pos + 1, :next_pos + 1], prev_emb, prev_layers, num_heads, Nv)
        lp = torch.log_softmax(logits[:, -1, :], dim=-1).gather(1, sample_ids[:, t:t + 1])
        out.append(lp)
        prev_emb = emb[:, :-1] if prev_emb is None else torch.cat((prev_emb, emb[:, :-1]), dim=1)
        prev_layers = [x[:, :-1] for x in new_layers] if prev_layers is None else [torch.cat((a, b[:, :-1]), dim=1)
                                                                                      for a, b in zip(prev_layers, new_layers)]
        curr = sample_ids[:, t:t + 1]
        next_pos += 1
        t += 1
    return torch.cat(out, dim=1)


def layout_logp(p, vf, vp, input_ids, token_type_ids, position_ids, am, sample_ids, mask_id, num_heads=12, Nv=100, dropout=None):
    """One training forward of the oracle (embeddings / encoder / lm_head) on the scoring layout: log-probs [B, T].  dropout: {site:
    multiplier} for the "emb" and per-layer sites of that forward (vf / vp arrive projected: the caller drops them), None: dropout 0."""
    out_len = token_type_ids.shape[1]
    ids, seg, pos, mask, mpos = layout_mirror(input_ids, sample_ids, token_type_ids[:, :out_len], position_ids[:, :out_len],
                                              am[:, :out_len, :out_len], mask_id)
    dt = p["bert.embeddings.word_embeddings.weight"].dtype
    emb, _ = O.embeddings(p, vf, vp, ids, seg, Nv, position_ids=pos, drop=None if dropout is None else dropout.get("emb"))
    seq = O.encoder(p, emb, O.extended_attention_mask(mask, dt), num_heads, dropout=dropout)[-1]
    logits = O.lm_head(p, O.gather_seq_out_by_pos(seq, mpos))
    return torch.log_softmax(logits, dim=-1).gather(2, sample_ids.unsqueeze(2)).squeeze(2)


def scst_inputs(B, max_len_b, seed, vocab, short=(), ragged=(), pos_offset=0, Nv=100):
    """Decoder inputs of an SCST step from a synthetic s2s batch (max_pred 0): img, vis_pe, prefix ids, segment ids, position ids, mask and
    random sampled ids [B, T].  short: samples whose ground truth is cut to 2 tokens (positions past second_end see only the prefix);
    ragged: (sample, valid regions) -- the mask hides the other region keys."""
    b = S.make_batch(B, max_len_b=max_len_b, len_vis_input=Nv, vocab_size=vocab, max_pred=0, mask_prob=0.0, seed=seed, min_len_b=4)
    L = b.input_ids.shape[1]
    am = b.input_mask.clone()
    for s in short:
        am[s] = S.build_attention_mask(L, Nv, 2, "s2s")
    for s, n in ragged:
        am[s, :, 1 + n:1 + Nv] = 0
    pos = torch.arange(L).unsqueeze(0).expand(B, L).contiguous() + pos_offset
    g = torch.Generator().manual_seed(seed + 7)
    T = L - (Nv + 2)
    sample = torch.randint(1, vocab, (B, T), generator=g)
    return b.img, b.vis_pe, b.input_ids[:, :Nv + 2].contiguous(), b.segment_ids, pos, am, sample, b.input_ids


# =====================================================================================================================================
# (1) CiderD
# =====================================================================================================================================
GT = [[11, 12, 13, 14, 102, 0, 0], [11, 15, 16, 17, 18, 102, 0], [19, 12, 13, 20, 102, 0, 0]]
GEN = [[11, 12, 13, 14, 102, 0, 0], [11, 15, 16, 102, 0, 0, 0], [19, 12, 21, 21, 21, 21, 21]]
GREEDY = [[11, 12, 13, 102, 0, 0, 0], [11, 15, 16, 17, 18, 102, 0], [12, 13, 102, 0, 0, 0, 0]]


def test_cider_check_value():
    reward, scores = SC.self_critical_reward(np.array(GREEDY), np.array(GT), np.array(GEN), 3)
    want_s = [10.0, 3.1001172239, 0.4307476915, 2.6301925787, 10.0, 0.9276059301]
    want_r = [7.3698074213, -6.8998827761, -0.4968582386]
    assert np.abs(scores - want_s).max() <= 1e-9, scores
    assert reward.shape == (3, 7)
    assert np.abs(reward - np.array(want_r)[:, None]).max() <= 1e-9, reward


def _score(gts, res):
    return SC.CiderD(df="corpus").compute_score(gts, res)


def test_cider_exact_match_disjoint_and_corpus_wide_ngrams():
    gts = {0: ["1 2 3 4 5 0"], 1: ["6 7 8 9 0"], 2: ["10 11 12 0"]}
    m, s = _score(gts, {0: ["1 2 3 4 5 0"], 1: ["6 7 8 9 0"], 2: ["10 11 12 0"]})
    assert np.allclose(s, 10.0, rtol=0, atol=1e-12) and abs(m - 10.0) < 1e-12
    _, s = _score(gts, {0: ["20 21 22 0"], 1: ["23 24 0"], 2: ["25 0"]})
    assert np.all(s[:2] == 0.0) and s[2] == 0.0
    # "0" ends every reference: df = #sets, so its idf weight log(3) - log(3) is 0 -- a hypothesis made of it scores nothing
    _, s = _score(gts, {0: ["0"], 1: ["0"], 2: ["0"]})
    assert np.all(s == 0.0)


def test_cider_gaussian_length_factor_and_bigram_length():
    gts = {0: ["1 2 3 4 0"], 1: ["5 6 7 8 0"]}
    # a hypothesis that repeats the reference's n-gram counts times 1 but is longer: only the Gaussian factor differs from a perfect match
    _, s_eq = _score(gts, {0: ["1 2 3 4 0"], 1: ["5 6 7 8 0"]})
    ref = SC.CiderD()
    # same clipped overlap (min(h, r) * r over the same n-grams), hypothesis two bigrams longer -> exp(-4 / 72) on every n
    _, s_long = _score(gts, {0: ["1 2 3 4 0 9 9"], 1: ["5 6 7 8 0"]})
    c = SC._ngrams("1 2 3 4 0 9 9".split(), 4)
    r = SC._ngrams("1 2 3 4 0".split(), 4)
    df = {}
    for refs in (r, SC._ngrams("5 6 7 8 0".split(), 4)):
        for g in refs:
            df[g] = df.get(g, 0) + 1
    vh, nh, lh = ref._vec(c, df, np.log(2.0))
    vr, nr, lr = ref._vec(r, df, np.log(2.0))
    assert (lh, lr) == (6, 4)
    assert abs(s_long[0] - np.mean(ref._sim(vh, vr, nh, nr, lh, lr)) * 10.0) < 1e-12
    nog = ref._sim(vh, vr, nh, nr, 0, 0)
    assert abs(s_long[0] - np.mean(nog) * 10.0 * np.exp(-4.0 / 72.0)) < 1e-12
    assert s_long[0] < s_eq[0]
    # length = number of bigram occurrences: a one-token sentence has length 0
    assert ref._vec(SC._ngrams(["7"], 4), {}, 0.0)[2] == 0
    assert ref._vec(SC._ngrams("7 8 9".split(), 4), {}, 0.0)[2] == 2


def test_cider_argument_checks():
    with pytest.raises(AssertionError):
        _score({0: ["1 0"]}, {1: ["1 0"]})
    with pytest.raises(AssertionError):
        _score({0: ["1 0"]}, {0: ["1 0", "2 0"]})
    with pytest.raises(AssertionError):
        _score({0: []}, {0: ["1 0"]})


def test_clean_captions_and_criterion_semantics():
    raw = torch.tensor([[5, 6, 102, 7, 0], [5, 0, 6, 102, 8], [5, 6, 7, 8, 9], [102, 5, 6, 0, 0]])
    got = SC.clean_captions(raw, 102, 0)
    assert got.tolist() == [[5, 6, 102, 0, 0], [5, 0, 0, 0, 0], [5, 6, 7, 8, 9], [102, 0, 0, 0, 0]]
    assert SC.array_to_str([5, 6, 0, 7, 0]) == "5 6 0" and SC.array_to_str([5, 6]) == "5 6"
    logp = torch.randn(4, 5, dtype=torch.float64, requires_grad=True)
    rew = torch.randn(4, 1, dtype=torch.float64).expand(4, 5)
    loss = SC.RewardCriterion()(logp, got, rew)
    mask = torch.cat([torch.ones(4, 1, dtype=torch.float64), (got > 0).double()[:, :-1]], 1)
    assert abs(float(loss) - float(-(logp * rew * mask).sum() / mask.sum())) < 1e-12


# =====================================================================================================================================
# (2) the reference's own scst_utils.py, unmodified
# =====================================================================================================================================
def _reference_scst_utils():
    path = os.path.join(REF, "vlp", "scst_utils.py")
    if not os.path.exists(path):
        pytest.skip("reference tree not present")
    from vlp_amd import compat
    compat.install()
    spec = importlib.util.spec_from_file_location("_ref_scst_utils", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_reference_scst_utils_equal_vlp_amd_scst():
    ref = _reference_scst_utils()
    g = torch.Generator().manual_seed(5)
    B, T, eos = 8, 9, 102
    for trial in range(6):
        gt = torch.randint(1, 40, (B, T), generator=g)
        gen_raw = torch.randint(0, 40, (B, T), generator=g)
        greedy_raw = torch.randint(1, 40, (B, T), generator=g)
        gt[:, -1] = 0
        gt[torch.arange(B), torch.randint(1, T - 1, (B,), generator=g)] = eos
        gen_raw[0, 0] = eos                    # eos at position 0
        gen_raw[1, -1] = eos                   # eos at the last column
        gen_raw[2] = torch.randint(1, 40, (T,), generator=g)     # no eos
        gen_raw[3, 2], gen_raw[3, 5] = 0, eos  # a sampled 0 before eos
        greedy_raw[4, 3] = eos
        if trial % 2:
            gen_raw[5:] = gt[5:]               # exact samples: negative / zero rewards against a worse greedy baseline
        gen, greedy = SC.clean_captions(gen_raw, eos), SC.clean_captions(greedy_raw, eos)
        want = ref.get_self_critical_reward(greedy, gt, gen, B)
        got, _ = SC.self_critical_reward(greedy, gt, gen, B)
        assert np.array_equal(got, want)
        logp = -torch.rand(B, T, generator=g, dtype=torch.float64)
        r = torch.from_numpy(want)
        l_ref = ref.RewardCriterion()(logp.clone().requires_grad_(True), gen, r)
        l_got = SC.RewardCriterion()(logp, gen, r)
        assert float(l_ref) == float(l_got)
    assert (want < 0).any()


# =====================================================================================================================================
# (3) the scoring layout: one training forward == the incremental decoder, log-probs and gradients (fp64)
# =====================================================================================================================================
@pytest.mark.parametrize("short,ragged,pos_offset", [((), (), 0), ((1,), ((0, 37), (2, 1)), 3)])
def test_scoring_layout_equals_forced_incremental_decode_fp64(short, ragged, pos_offset):
    V = 512
    p = O.init_params(vocab_size=V, layers=2, seed=3, std=0.05, dtype=torch.float64)
    p = {k: v.requires_grad_(True) for k, v in p.items()}
    img, vis_pe, prefix, seg, pos, am, sample, _ = scst_inputs(3, 6, 11, V, short=short, ragged=ragged, pos_offset=pos_offset)
    reward = torch.tensor([[0.7], [-1.3], [0.4]], dtype=torch.float64).expand(3, sample.shape[1])
    seq = sample.clone()
    seq[0, 4:] = 0                                       # a cleaned caption: the criterion's mask has zeros

    def run(fn):
        for t in p.values():
            t.grad = None
        vf, vp = O.vis_embed(p, img.double()), O.vis_pe_embed(p, vis_pe.double())
        lp = fn(p, vf, vp, prefix, seg, pos, am, sample, S.MASK_ID)
        SC.RewardCriterion()(lp, seq, reward).backward()
        return lp.detach(), {k: t.grad.clone() for k, t in p.items() if t.grad is not None}

    lp_ref, g_ref = run(forced_decode_logp)
    lp_lay, g_lay = run(layout_logp)
    assert torch.allclose(lp_lay, lp_ref, rtol=0, atol=1e-10), (lp_lay - lp_ref).abs().max()
    assert set(g_ref) == set(g_lay)
    for k in g_ref:
        d = float((g_lay[k] - g_ref[k]).abs().max())
        assert d <= 1e-10 * max(1.0, float(g_ref[k].abs().max())), (k, d)


@pytest.mark.skipif(not ref_loader.reference_available(), reason="needs the reference tree (VLP_REFERENCE_ROOT)")
def test_reference_decoder_sample_mode_equals_forced_decode():
    """The UNMODIFIED reference BertForSeq2SeqDecoder in train() with sample_mode='sample' (modeling.py:1229-1235, the SCST call of
    run_img2txt_dist.py:506-507), drop_prob 0, fp32, 2 layers, seeded: its (ids, logprobs) and the parameter gradients of RewardCriterion
    with a fixed signed reward equal the oracle's forced incremental decode on those ids -- the decode the scoring layout is pinned to above."""
    V = 1024
    dec = ref_loader.build_reference_model(dict(vocab_size=V, num_hidden_layers=2), seed=8, decoder=True, drop_prob=0.0,
                                           mask_word_id=S.MASK_ID, eos_id=S.SEP_ID).train()
    img, vis_pe, prefix, seg, pos, am, _, _ = scst_inputs(3, 6, 11, V, short=(1,), ragged=((0, 37),), pos_offset=1)
    torch.manual_seed(1234)
    ids, logprobs = dec(img, vis_pe, prefix, seg, pos, am, task_idx=None, sample_mode="sample")
    assert logprobs.requires_grad and tuple(ids.shape) == tuple(logprobs.shape) == (3, seg.shape[1] - prefix.shape[1])
    gen = SC.clean_captions(ids, S.SEP_ID)
    reward = torch.tensor([[1.7], [-0.6], [0.9]]).expand_as(logprobs)
    SC.RewardCriterion()(logprobs, gen, reward).backward()
    ref_g = {n: q.grad for n, q in dec.named_parameters() if q.grad is not None}
    p = O.params_from_state_dict(dec.state_dict(), requires_grad=True)
    vf, vp = O.vis_embed(p, img), O.vis_pe_embed(p, vis_pe)
    lp = forced_decode_logp(p, vf, vp, prefix, seg, pos, am, ids, S.MASK_ID)
    SC.RewardCriterion()(lp, gen, reward).backward()
    e_lp = float(((lp - logprobs).abs() / logprobs.abs()).max().detach())
    assert e_lp <= 1e-5, e_lp
    got = {k: t.grad for k, t in p.items() if t.grad is not None}
    assert set(got) == set(ref_g), set(got) ^ set(ref_g)
    for k, g in ref_g.items():
        # max-normalised; a key bias has the true gradient 0 (softmax is shift invariant): bounded against its query-bias sibling
        scale = ref_g[k.replace("key.bias", "query.bias")] if k.endswith("attention.self.key.bias") else g
        e = float((got[k] - g).abs().max() / scale.abs().max())
        assert e <= 1e-5, (k, e)


def test_layout_mirror_shapes_and_rules():
    img, vis_pe, prefix, seg, pos, am, sample, _ = scst_inputs(2, 5, 4, 300)
    T, in_len = sample.shape[1], prefix.shape[1]
    ids, s2, p2, m2, mpos = layout_mirror(prefix, sample, seg, pos, am, S.MASK_ID)
    Lo = in_len + 2 * T - 1
    assert ids.shape == (2, Lo) and m2.shape == (2, Lo, Lo) and mpos.shape == (2, T)
    assert bool((ids[:, mpos[0]] == S.MASK_ID).all()) and torch.equal(ids[:, in_len:in_len + T - 1], sample[:, :T - 1])
    assert torch.equal(p2[:, in_len + T - 1:], pos[:, in_len:in_len + T])
    # a [MASK] slot sees only itself among the [MASK] slots
    mm = m2[:, in_len + T - 1:, in_len + T - 1:]
    assert bool((mm * (1 - torch.eye(T, dtype=torch.long)) == 0).all())


# =====================================================================================================================================
# (4) entry script checks
# =====================================================================================================================================
def test_entry_script_scst_argument_checks():
    from vlp_amd import run_img2txt_dist as R
    base = ["--enable_butd", "--fp16", "--scst"]
    with pytest.raises(AssertionError, match="coco only"):
        R.derive_args(R.build_parser().parse_args(base + ["--dataset", "cc", "--max_pred", "0", "--mask_prob", "0"]))
    with pytest.raises(AssertionError, match="no mask for scst"):
        R.derive_args(R.build_parser().parse_args(base))
    with pytest.raises(AssertionError, match="no mask for scst"):
        R.derive_args(R.build_parser().parse_args(base + ["--max_pred", "0"]))
    args = R.derive_args(R.build_parser().parse_args(base + ["--max_pred", "0", "--mask_prob", "0"]))
    with pytest.raises(AssertionError, match="must init from maximum likelihood"):
        R.check_scst_start(args, None)
    R.check_scst_start(args, 3)                     # a resume
    args.model_recover_path = "model.1.bin"
    R.check_scst_start(args, None)
    plain = R.derive_args(R.build_parser().parse_args(["--enable_butd", "--fp16"]))
    R.check_scst_start(plain, None)


def test_compat_registers_the_cider_scorer_only_when_absent():
    from vlp_amd import compat
    compat.install()
    try:
        import pycocoevalcap.cider.cider as cc
        if getattr(sys.modules["pycocoevalcap.cider.cider"], "__vlp_amd_alias__", False):
            assert cc.Cider is SC.CiderD
    finally:
        compat.uninstall()
    assert "pycocoevalcap.cider.cider" not in sys.modules or not getattr(sys.modules["pycocoevalcap.cider.cider"], "__vlp_amd_alias__", False)


def test_scst_structs_match_c_layout_and_are_exported(tmp_path):
    import ctypes
    import subprocess
    from vlp_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    structs = {"vlp_embed_bwd_pos_args": _lib.EmbedBwdPosArgs, "vlp_scst_layout_args": _lib.ScstLayoutArgs,
               "vlp_token_logprob_fwd_args": _lib.TokenLogprobFwdArgs, "vlp_token_logprob_bwd_args": _lib.TokenLogprobBwdArgs}
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
    subprocess.check_call(["gcc", "-I", os.path.join(root, "include"), src, "-o", exe])
    for line in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.strip().splitlines():
        parts = line.split()
        st = structs[parts[0]]
        assert int(parts[1]) == ctypes.sizeof(st), parts[0]
        assert [int(x) for x in parts[2:]] == [getattr(st, f).offset for f, _ in st._fields_], parts[0]
    for name in ("vlp_embed_bwd_pos", "vlp_scst_layout", "vlp_token_logprob_fwd", "vlp_token_logprob_bwd"):
        assert name in _lib.SYMBOLS
