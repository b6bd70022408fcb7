"""GPU: temperature / top_k / top_p through BertForSeq2SeqDecoder.forward, Engine.decode_sample_group (plain, captured and replayed token
steps) and python -m vlp_amd.sample_img2txt.  2 layers, vocabulary 1024, 3 images, 6 steps: the setup of test_sample_mode_end_to_end."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from oracle import vlp_oracle as O                         # noqa: E402  (checker)
from oracle.make_golden import decode_inputs               # noqa: E402  (pure helper)
from tests import sample_filter_util as U                  # noqa: E402
from tests.step_seq_util import first_difference           # noqa: E402
from vlp_amd import decode_img2txt as D                    # noqa: E402
from vlp_amd import sample_img2txt as SI                   # noqa: E402
from vlp_amd import synthetic as S                         # noqa: E402
from vlp_amd.data import write_packed                      # noqa: E402
from vlp_amd.modeling import BertConfig, BertForSeq2SeqDecoder   # noqa: E402

DEV = torch.device("cuda:0")
MK = dict(vocab_size=1024, layers=2, tasks="img2txt", seed=41, std=0.05)
B, T = 3, 6
LOGIT_TOL = 1.5e-2       # fp16 evaluation noise of a logit against the fp32 oracle (test_40_decode_gpu.py MARGIN_TOL)
LOGP_TOL = 3e-2          # test_sample_mode_end_to_end's tolerance on a log-probability


@pytest.fixture(scope="module")
def params():
    return O.init_params(vocab_size=MK["vocab_size"], layers=MK["layers"], tasks=MK["tasks"], seed=MK["seed"], std=MK["std"])


def build_decoder(p, beam=1):
    cfg = BertConfig(MK["vocab_size"], num_hidden_layers=MK["layers"], type_vocab_size=6, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1)
    m = BertForSeq2SeqDecoder(cfg, mask_word_id=S.MASK_ID, eos_id=S.SEP_ID, enable_butd=True, len_vis_input=100, search_beam_size=beam)
    sd = dict(p)
    sd["cls.predictions.decoder.weight"] = p["bert.embeddings.word_embeddings.weight"]
    m.load_state_dict(sd, strict=True)
    return m.half().to(DEV).eval()


def inputs():
    dv = [t.to(DEV) for t in decode_inputs(B, T, 99)]
    return [dv[0].half(), dv[1].half()] + dv[2:]


def call(m, dv, seed_state=None, **kw):
    if seed_state is not None:
        m.engine.step_seed = seed_state
    ids, lp = m(*dv, sample_mode="sample", **kw)
    return {"ids": ids.clone(), "logp": lp.clone()}


@pytest.mark.parametrize("Ks", [1, 3])
def test_neutral_keywords_change_nothing(params, Ks):
    m, dv = build_decoder(params), inputs()
    for rnd in range(3):                                     # plain, captured, replayed
        a = call(m, dv, seed_state=100 * rnd, n_samples=Ks)
        b = call(m, dv, seed_state=100 * rnd, n_samples=Ks, temperature=1.0, top_k=0, top_p=1.0)
        assert first_difference(a, b) is None, (rnd, first_difference(a, b))
    assert not any(len(k) > 2 for ws in m.engine._ws.values() if "plans" in ws for k in ws["plans"])      # the plans of an unfiltered call only


def test_top_k_1_is_the_greedy_decode(params):
    m, dv = build_decoder(params), inputs()
    ids_g, _ = m(*dv, sample_mode="greedy")
    for rnd in range(3):
        o = call(m, dv, n_samples=1, top_k=1)
        assert torch.equal(o["ids"], ids_g), rnd
        assert torch.equal(o["logp"], torch.zeros_like(o["logp"])), rnd      # exactly 0


def test_filtered_samples_against_the_teacher_forced_oracle(params):
    """n_samples = 3, T = 0.8, top_k = 20, top_p = 0.9.  The oracle's logits differ from the engine's by fp16 evaluation noise, so the kept set
    may differ at its threshold: |S| (Engine's filter_kept) may differ from the restatement's on the oracle's logits only where top_p is
    within the noise of a cumulative mass (each mass moves by exp(+-LOGIT_TOL / T), a ratio of two sums by twice that) or where the
    top_k-th and the next logit are within the noise of each other (a tie on one side, a member more in S_k), and the reference
    log-probability is then normalised over the oracle's largest logits of the engine's count.  The last step's logits are still in the
    workspace: there the drawn ids are checked against the engine's own rows and cutoff exactly."""
    Ks, Tm, top_k, top_p = 3, 0.8, 20, 0.9
    m, dv = build_decoder(params), inputs()
    eng = m.engine
    pd = {k: v.to(DEV).half().float() for k, v in params.items()}
    in_len = dv[2].shape[1]
    vf, vp = O.vis_embed(pd, dv[0].float()), O.vis_pe_embed(pd, dv[1].float())

    def tiled(t):
        return t.repeat(Ks, *([1] * (t.dim() - 1)))
    vf, vp, prefix, seg, pos, am = [tiled(t) for t in (vf, vp, dv[2], dv[3], dv[4], dv[5])]
    mass_noise = 2 * (np.exp(LOGIT_TOL / Tm) - 1)
    for rnd in range(3):                                     # plain, captured, replayed
        ids, lps = m(*dv, sample_mode="sample", n_samples=Ks, temperature=Tm, top_k=top_k, top_p=top_p)
        assert tuple(ids.shape) == (Ks * B, T) and float(lps.max()) <= 0.0
        ws = eng._ws[("dec", B, in_len + 1, in_len + T, Ks, "group")]
        # decode row b*Ks + k -> sample-major row k*B + b
        kept = ws["filter_kept"][:T].view(T, B, Ks).permute(2, 1, 0).reshape(Ks * B, T).cpu().numpy()
        cut = ws["filter_cutoff"][:T].view(T, B, Ks).permute(2, 1, 0).reshape(Ks * B, T).cpu().numpy()
        assert kept.min() >= 1 and kept.max() <= 2 * top_k
        ids_c, lps_c = ids.cpu().numpy(), lps.cpu().numpy().astype(np.float64)
        worst, flips = 0.0, 0
        for s in range(T):
            x = torch.cat((prefix, ids[:, :s], torch.full((Ks * B, 1), S.MASK_ID, device=DEV, dtype=torch.long)), dim=1)
            Lk = in_len + s + 1
            emb, _ = O.embeddings(pd, vf, vp, x, seg[:, :Lk], 100, position_ids=pos[:, :Lk])
            hs = O.encoder(pd, emb, O.extended_attention_mask(am[:, :Lk, :Lk], torch.float32), 12)
            logits = O.lm_head(pd, hs[-1][:, -1:, :])[:, 0].double().cpu().numpy()
            for r in range(Ks * B):
                i = int(ids_c[r, s])
                ref = U.filter_reference(logits[r].astype(np.float16), Tm, top_k, top_p)
                assert logits[r, i] >= cut[r, s] - LOGIT_TOL, (rnd, s, r)                  # the id is in the engine's set, seen from the oracle
                n_keep = ref["kept"]
                if kept[r, s] != n_keep:
                    srt = np.sort(logits[r])[::-1]
                    assert ref["margin"] <= mass_noise or srt[top_k - 1] - srt[top_k] <= 2 * LOGIT_TOL, (rnd, s, r, kept[r, s], n_keep, ref["margin"])
                    n_keep, flips = int(kept[r, s]), flips + 1
                z = np.sort(logits[r])[::-1][:n_keep] / np.float64(np.float32(Tm))
                want = logits[r, i] / np.float64(np.float32(Tm)) - (z[0] + np.log(np.exp(z - z[0]).sum()))
                worst = max(worst, abs(want - lps_c[r, s]))
        print("call %d: largest |logp - oracle| %.3e, %d of %d thresholds moved by evaluation noise" % (rnd, worst, flips, Ks * B * T))
        assert worst < LOGP_TOL, (rnd, worst)
        # the last step against the engine's own logits
        own = ws["logits"][:, :MK["vocab_size"]].float()                                   # decode rows b*Ks + k
        last_ids = ids[:, T - 1].reshape(Ks, B).t().reshape(-1)
        last_cut, last_kept = ws["filter_cutoff"][T - 1], ws["filter_kept"][T - 1]
        assert bool((own[torch.arange(Ks * B, device=DEV), last_ids] >= last_cut).all())
        assert torch.equal((own >= last_cut.unsqueeze(1)).sum(dim=1).int(), last_kept)
        for r in range(Ks * B):
            ref = U.filter_reference(own[r].half().cpu().numpy(), Tm, top_k, top_p)
            if ref["margin"] >= U.MARGIN_MIN:
                assert int(last_kept[r]) == ref["kept"] and float(last_cut[r]) == ref["cutoff"]
                want = ref["logp"][int(last_ids[r])]
                got = lps_c.reshape(Ks, B, T)[r % Ks, r // Ks, T - 1]
                assert abs(want - got) <= 1e-5, (r, want, got)


def test_replayed_steps_equal_a_fresh_engine_and_carry_their_own_parameters(params):
    dv = inputs()
    P1 = dict(n_samples=3, temperature=0.8, top_k=20, top_p=0.9)
    P2 = dict(n_samples=3, temperature=1.5, top_k=0, top_p=0.5)
    P0 = dict(n_samples=3)
    m = build_decoder(params)
    seq = [(P1, 0), (P1, 50), (P1, 100), (P2, 150), (P0, 200), (P1, 250), (P2, 300), (P0, 350)]   # P1: plain, captured, replayed; then the others between
    outs = [call(m, dv, seed_state=st, **p) for p, st in seq]
    ws = m.engine._ws[("dec", B, dv[2].shape[1] + 1, dv[2].shape[1] + T, 3, "group")]
    for p in (P1, P2):
        assert all(("sample_group", s, p["temperature"], p["top_k"], p["top_p"]) in ws["plans"] for s in range(1, T)), sorted(ws["plans"], key=str)
    assert all(("sample_group", s) in ws["plans"] for s in range(1, T))
    for j in (2, 5, 6, 7):                                   # replays: of P1, of P1 after P2 and P0, of P2, of P0
        p, st = seq[j]
        fresh = call(build_decoder(params), dv, seed_state=st, **p)
        d = first_difference(outs[j], fresh)
        assert d is None, (j, d)
    assert first_difference(outs[2], outs[5]) is not None    # other seeds, other draws


def test_value_errors(params):
    m, dv = build_decoder(params), inputs()
    for kw in (dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=float("inf")), dict(temperature=float("nan")), dict(top_k=-1),
               dict(top_p=0.0), dict(top_p=1.01), dict(top_p=float("nan"))):
        for mode in ("sample", "greedy"):
            with pytest.raises(ValueError):
                m(*dv, sample_mode=mode, **kw)
    for kw in (dict(temperature=0.7), dict(top_k=5), dict(top_p=0.9)):
        with pytest.raises(ValueError, match="sample_mode"):
            m(*dv, sample_mode="greedy", **kw)
        with pytest.raises(ValueError, match="sample_mode"):
            m(*dv, **kw)
    with pytest.raises(NotImplementedError):
        m(*dv, sample_mode="nucleus")                        # no new mode name
    mb = build_decoder(params, beam=2)
    with pytest.raises(ValueError, match="search_beam_size"):
        mb(*dv, sample_mode="sample", top_k=5)
    m.train()
    try:
        with pytest.raises(ValueError, match="train"):
            m(*dv, sample_mode="sample", top_p=0.9)
        with torch.no_grad():                                # without gradients the filtered draw is fine in train() mode
            ids, lp = m(*dv, sample_mode="sample", top_p=0.9)
        assert tuple(ids.shape) == (B, T) and not lp.requires_grad
    finally:
        m.eval()


# ---- the command line ---------------------------------------------------------------------------------------------------
NV, TC, VOCAB = 100, 10, 1024
LIST = [("test", 391895), ("val", 522418), ("test", 184613), ("test", 318219), ("val", 554625), ("test", 574769), ("test", 60623)]


def fname(i):
    return "COCO_val2014_%012d.jpg" % i


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    """A packed store of 5 images, a 2-layer checkpoint, a vocabulary and a Karpathy-style image list (as tests/test_42_decode_cli_gpu.py)."""
    root = str(tmp_path_factory.mktemp("sample_cli"))
    rng = np.random.RandomState(5)
    test_ids = [i for sp, i in LIST if sp == "test"]
    keys = [fname(i)[:-4] for i in reversed(test_ids)]
    feats = np.abs(rng.randn(5, NV, 2048)).astype(np.float16)
    cls = rng.rand(5, NV, 1601).astype(np.float32)
    cls /= cls.sum(-1, keepdims=True)
    xy = rng.rand(5, NV, 2, 2) * 400
    boxes = np.concatenate([xy.min(2), xy.max(2) + 1.0, np.zeros((5, NV, 1)), rng.rand(5, NV, 1)], axis=-1).astype(np.float32)
    store = os.path.join(root, "store")
    write_packed(store, keys, feats, cls, boxes)
    bert = os.path.join(root, "bert")
    os.makedirs(bert)
    with open(os.path.join(bert, "bert_config.json"), "w") as f:
        f.write(BertConfig(VOCAB, num_hidden_layers=2, type_vocab_size=2).to_json_string())
    special = {S.PAD_ID: "[PAD]", S.UNK_ID: "[UNK]", S.CLS_ID: "[CLS]", S.SEP_ID: "[SEP]", S.MASK_ID: "[MASK]"}
    tokens = [special.get(i, "w%d" % i) for i in range(VOCAB)]
    with open(os.path.join(bert, "vocab.txt"), "w") as f:
        f.write("\n".join(tokens) + "\n")
    p = O.init_params(vocab_size=VOCAB, layers=2, tasks="img2txt", seed=27, std=0.1)
    sd = dict(p)
    sd["cls.predictions.decoder.weight"] = p["bert.embeddings.word_embeddings.weight"]
    ckpt = os.path.join(root, "model.3.bin")
    torch.save(sd, ckpt)
    src = os.path.join(root, "dataset.json")
    with open(src, "w") as f:
        json.dump({"images": [{"split": sp, "filename": fname(i), "filepath": "val2014", "imgid": n} for n, (sp, i) in enumerate(LIST)]}, f)
    return dict(root=root, store=store, bert=bert, ckpt=ckpt, src=src, test_ids=test_ids)


def argv(su, out, *extra):
    return ["--bert_model", su["bert"], "--model_recover_path", su["ckpt"], "--packed_features", su["store"], "--src_file", su["src"], "--split", "test",
            "--dataset", "coco", "--output_file", out, "--batch_size", "2", "--max_tgt_length", str(TC), "--new_segment_ids", "--fp16",
            "--enable_butd"] + list(extra)


def test_cli_writes_one_record_per_image_and_sample(setup):
    su = setup
    flags = ("--temperature", "0.9", "--top_k", "40", "--top_p", "0.95", "--num_samples", "3")
    files = []
    for name, seed in (("a", 11), ("b", 11), ("c", 12)):
        out = os.path.join(su["root"], "samples_%s.json" % name)
        res = SI.main(argv(su, out, "--seed", str(seed), *flags))
        with open(out) as f:
            files.append(f.read())
        assert res == {su["ckpt"]: json.loads(files[-1])}
    recs = json.loads(files[0])
    assert len(recs) == 5 * 3                                                       # images x samples
    assert [(r["image_id"], r["sample"]) for r in recs] == [(i, k) for i in su["test_ids"] for k in range(3)]     # by image, then by sample
    assert all(set(r) == {"image_id", "sample", "caption", "logprob"} and type(r["caption"]) is str and type(r["logprob"]) is float
               and r["logprob"] <= 0.0 for r in recs)
    assert files[0] == files[1] and files[0] != files[2]                            # the seed selects the draws
    assert any(len({r["caption"] for r in recs if r["image_id"] == i}) > 1 for i in su["test_ids"])      # the samples of an image differ


def test_cli_top_k_1_writes_the_greedy_captions(setup):
    su = setup
    out_s, out_g = os.path.join(su["root"], "samples_k1.json"), os.path.join(su["root"], "greedy.json")
    SI.main(argv(su, out_s, "--top_k", "1"))
    D.main(argv(su, out_g, "--beam_size", "1"))
    with open(out_s) as f:
        recs = json.load(f)
    with open(out_g) as f:
        greedy = json.load(f)
    assert [(r["image_id"], r["caption"]) for r in recs] == [(g["image_id"], g["caption"]) for g in greedy]
    assert all(r["sample"] == 0 and r["logprob"] == 0.0 for r in recs)
    assert len({g["caption"] for g in greedy}) > 1 and any(len(g["caption"].split()) >= 2 for g in greedy)


def test_cli_refuses_what_it_does_not_do(setup, capsys):
    su = setup
    never = os.path.join(su["root"], "never.json")
    for extra, word in ((("--beam_size", "3"), "decode_img2txt"), (("--forbid_duplicate_ngrams",), "decode_img2txt"),
                        (("--batch_size", "600", "--num_samples", "2"), "1200 sequences")):
        with pytest.raises(SystemExit):
            SI.main(argv(su, never, *extra))
        assert word in capsys.readouterr().err
    with pytest.raises(NotImplementedError, match="--fp16"):
        SI.main([a for a in argv(su, never) if a != "--fp16"])
    assert not os.path.exists(never)
