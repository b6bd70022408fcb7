"""GPU: diverse (group) beam search on the device (vlp_beam_select_groups, Engine.decode_beam(groups=, diversity=, group_select=),
BertForSeq2SeqDecoder(beam_groups=, diversity_penalty=), python -m vlp_amd.decode_img2txt --beam_groups).

  * the kernel against vlp_amd.diverse.beam_select_groups_host (numpy, fp32) on frames built to hurt: all six outputs bit for bit, guard bands,
    poisoned outputs, NaN around the inputs, next_ids with the engine's stride 2, two launches bit-equal, G = 1 against vlp_beam_select,
    refusals without a launch;
  * the model: the device selection equals the host path bit for bit (with and without blocking / min_len), the invariants of the traces, G = 1
    is the decoder as it was, run / capture / replay and a decoder that alternated every kind of call against a fresh one;
  * the command line: --beam_groups 1 changes no byte; --beam_groups 2 --n_best 4 --select consensus against consensus.consensus_utility.
"""
import functools
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from oracle import vlp_oracle as O                                  # noqa: E402  (checker: the parameters of a small model)
from oracle.make_golden import BEAM_CASES, decode_inputs            # noqa: E402  (pure helpers)
from tests import consensus_util as CU                              # noqa: E402
from tests import diverse_util as DU                                # noqa: E402
from tests import guard_util as GU                                  # noqa: E402
from vlp_amd import _lib as K_                                      # noqa: E402
from vlp_amd import consensus as CS                                 # noqa: E402
from vlp_amd import decode_img2txt as D                             # noqa: E402
from vlp_amd import eval_captions as EC                             # noqa: E402
from vlp_amd import scst as SC                                      # noqa: E402
from vlp_amd import synthetic as S                                  # noqa: E402
from vlp_amd.data import write_packed                               # noqa: E402
from vlp_amd.diverse import beam_select_groups_host                 # noqa: E402
from vlp_amd.modeling import BertConfig, BertForSeq2SeqDecoder      # noqa: E402
from vlp_amd.nbest import beam_nbest_host, by_image                 # noqa: E402

DEV = torch.device("cuda:0")
EOS = DU.EOS

# ------------------------------------------------------------------------------------------------
# vlp_beam_select_groups against the host specification
# ------------------------------------------------------------------------------------------------
# (B, K, G): the smallest group structures (Kg = 1, Kg = 2), three groups, G = 1, every beam a group of its own at the limit, two groups of 32
# (2048 candidates per group: 32 per lane) and 16 groups of 4 at the limit
SHAPES = [(3, 2, 2), (3, 4, 2), (2, 6, 3), (2, 6, 1), (1, 64, 64), (1, 64, 2), (2, 64, 16)]
PENALTIES = [0.0, 0.3, 100.0]          # 0.3: inexact products.  On these frames (v0 on a 0.25 grid) a key that is off in the last bit does not
                                       # change a pick; test_kernel_rounds_the_product_before_the_subtraction is what catches a contracted key
NAMES = ("out_scores", "out_ids", "out_ptrs", "out_eos", "src_rows", "next_ids")


@functools.lru_cache(maxsize=None)
def frame(B, K, first):
    return DU.hostile_frame(B, K, bool(first), 1000 * K + 10 * B + int(first))


@functools.lru_cache(maxsize=None)
def host(B, K, G, first, lam):
    """The specification's six arrays for a case; computed once, read only."""
    out = beam_select_groups_host(*frame(B, K, first), bool(first), EOS, G, lam, next_ids_stride=2)
    for a in out:
        a.setflags(write=False)
    return out


def device_inputs(B, K, first):
    """The float inputs sit between NaN guards (a stray read poisons a key), the ids between guards that hold a word of the vocabulary."""
    ks, ki, lt, le = frame(B, K, first)
    g_ks = GU.guarded_vec(ks.size, torch.float32, "nan", device=DEV).set(torch.from_numpy(np.array(ks)).to(DEV))
    g_ki = GU.guarded_vec(ki.size, torch.int64, 5, device=DEV).set(torch.from_numpy(np.array(ki)).to(DEV))
    if first:
        return g_ks, g_ki, None, None
    g_lt = GU.guarded_vec(lt.size, torch.float32, "nan", device=DEV).set(torch.from_numpy(np.array(lt)).to(DEV))
    g_le = GU.guarded_vec(le.size, torch.float32, "nan", device=DEV).set(torch.from_numpy(np.array(le)).to(DEV))
    return g_ks, g_ki, g_lt, g_le


def guarded_outputs(B, K):
    R = B * K
    return (GU.guarded_vec(R, torch.float32, "sentinel", device=DEV), GU.guarded_vec(R, torch.int64, "sentinel", device=DEV),
            GU.guarded_vec(R, torch.int64, "sentinel", device=DEV), GU.guarded_vec(R, torch.float32, "sentinel", device=DEV),
            GU.guarded_vec(R, torch.int64, "sentinel", device=DEV),
            GU.guarded(R, 1, ld=2, dtype=torch.int64, fill="sentinel", device=DEV))     # the engine's xids[:, 0]: stride 2


def launch(ins, outs, B, K, G, first, lam, plain=False):
    vec = [None if g is None else g.vec for g in ins]
    args = (vec[0], vec[1], vec[2], vec[3], outs[0].vec, outs[1].vec, outs[2].vec, outs[3].vec, outs[4].vec, outs[5].view[:, 0], B, K, bool(first), EOS)
    if plain:
        K_.beam_select(*args)
    else:
        K_.beam_select_groups(*args, G, lam)


def read(outs):
    return [GU.bits(g.view).cpu().numpy().reshape(-1) for g in outs]


def same_bits(got, want):
    return np.array_equal(got, np.ascontiguousarray(want).reshape(-1).view(got.dtype))


@pytest.mark.parametrize("lam", PENALTIES)
@pytest.mark.parametrize("first", [0, 1])
@pytest.mark.parametrize("B,K,G", SHAPES, ids=["B%d_K%d_G%d" % s for s in SHAPES])
def test_kernel_equals_the_host_specification(B, K, G, first, lam):
    want = host(B, K, G, first, lam)
    ins = device_inputs(B, K, first)
    runs = []
    for _ in range(2):
        outs = guarded_outputs(B, K)
        launch(ins, outs, B, K, G, first, lam)
        torch.cuda.synchronize()
        for g, name in zip(outs, NAMES):
            GU.assert_untouched(g, written="logical", name=name)         # nothing outside [B*K] / column 0 of next_ids
            GU.assert_written(g, written="logical", name=name)           # and every slot was written
        runs.append(read(outs))
    for g in ins:
        if g is not None:
            GU.assert_untouched(g, written=None, name="input")
    got = runs[0]
    for name, a, w in zip(NAMES, got, want[:5] + (want[5][:, 0],)):
        assert same_bits(a, w), (name, a, w)
    assert all(np.array_equal(a, b) for a, b in zip(*runs)), "two launches differ"
    if not first:                                                       # parents stay inside their group
        assert np.array_equal(got[2].reshape(B, K) // (K // G), np.broadcast_to(np.arange(K) // (K // G), (B, K)))


def test_hostile_frames_reach_what_they_are_for():
    """Taken together the cases hold picks decided by a tie, -inf picks, and penalties that change the picked words."""
    ties = minus_inf = changed = 0
    for B, K, G in SHAPES:
        for first in (0, 1):
            base = host(B, K, G, first, 0.0)
            for lam in PENALTIES:
                sc, ids = host(B, K, G, first, lam)[:2]
                minus_inf += int(np.isneginf(sc).sum())
                ties += int((sc[:, 1:] == sc[:, :-1]).sum())
                changed += int(G > 1 and lam > 0 and not np.array_equal(ids, base[1]))
    assert ties > 50 and minus_inf > 10 and changed >= 10, (ties, minus_inf, changed)
    ks, ki, lt, le = frame(3, 4, 0)
    assert le[1].all() and np.isneginf(ks[2]).all()                      # the image of ended parents, the image that is all -inf
    ks, ki, lt, le = frame(2, 6, 0)                                      # and the batches of two hold ordinary images: live and ended parents mixed
    assert all(0 < le[b].sum() < 6 and np.isfinite(ks[b]).any() for b in range(2)), le


def test_kernel_rounds_the_product_before_the_subtraction(monkeypatch):
    """DU.separating_frame (K = 18, G = 2, lambda = 0.3): a key formed by one fused multiply-subtract ties where the specification's two
    roundings do not, and slots 9 and 10 swap.  The specification with a fused key is shown to differ first, so a contracted kernel fails
    the bit-for-bit comparison here."""
    from vlp_amd import diverse as DV
    fr, lam, B, K, G = DU.separating_frame(), DU.SEPARATING_PENALTY, 1, 18, 2
    want = beam_select_groups_host(*fr, False, EOS, G, lam, next_ids_stride=2)
    with monkeypatch.context() as mp:
        mp.setattr(DV, "_key", DU.fused_key)
        fused = beam_select_groups_host(*fr, False, EOS, G, lam, next_ids_stride=2)
    assert want[1][0, 9:11].tolist() == [10, 11] and fused[1][0, 9:11].tolist() == [11, 10]
    assert want[0][0, 9:11].tolist() == [-3.75, -2.25] and fused[0][0, 9:11].tolist() == [-2.25, -3.75]
    ins = [GU.guarded_vec(a.size, torch.float32 if a.dtype == np.float32 else torch.int64, "nan" if a.dtype == np.float32 else 5,
                          device=DEV).set(torch.from_numpy(np.array(a)).to(DEV)) for a in fr]
    outs = guarded_outputs(B, K)
    launch(ins, outs, B, K, G, 0, lam)
    torch.cuda.synchronize()
    for g, name in zip(outs, NAMES):
        GU.assert_untouched(g, written="logical", name=name)
        GU.assert_written(g, written="logical", name=name)
    for name, a, w in zip(NAMES, read(outs), want[:5] + (want[5][:, 0],)):
        assert same_bits(a, w), (name, a.reshape(-1)[7:12], np.asarray(w).reshape(-1)[7:12])


@pytest.mark.parametrize("first", [0, 1])
def test_one_group_equals_vlp_beam_select(first):
    B, K = 2, 6
    ins = device_inputs(B, K, first)
    a, b = guarded_outputs(B, K), guarded_outputs(B, K)
    launch(ins, a, B, K, 1, first, 0.3)
    launch(ins, b, B, K, 1, first, 0.0, plain=True)
    torch.cuda.synchronize()
    for name, x, y in zip(NAMES, read(a), read(b)):
        assert np.array_equal(x, y), name


@pytest.mark.parametrize("what", ["K_mod_G", "G_zero", "G_gt_K", "K_65", "nan", "negative", "inf", "no_last", "null_scores", "null_next"])
def test_refusals_launch_nothing(what):
    B, K = 2, (65 if what == "K_65" else 6)
    G = {"K_mod_G": 4, "G_zero": 0, "G_gt_K": 12, "K_65": 5}.get(what, 3)
    lam = {"nan": float("nan"), "negative": -0.5, "inf": float("inf")}.get(what, 0.5)
    ks, ki = torch.zeros(B, K, K, device=DEV), torch.zeros(B, K, K, dtype=torch.long, device=DEV)
    lt, le = torch.zeros(B, K, device=DEV), torch.zeros(B, K, device=DEV)
    outs = guarded_outputs(B, K)
    with pytest.raises(RuntimeError, match="vlp_beam_select_groups"):
        K_.beam_select_groups(None if what == "null_scores" else ks, ki, None if what == "no_last" else lt, le, outs[0].vec, outs[1].vec, outs[2].vec,
                              outs[3].vec, outs[4].vec, None if what == "null_next" else outs[5].view[:, 0], B, K, False, EOS, G, lam)
    torch.cuda.synchronize()
    for g, name in zip(outs, NAMES):
        GU.assert_untouched(g, written=None, name=name)


# ------------------------------------------------------------------------------------------------
# the model
# ------------------------------------------------------------------------------------------------
MK, NB, NT = BEAM_CASES["beam_2l_K3"][0], 3, 6                       # the 2-layer model of the n-best tests, B = 3, 6 generated tokens
PLAIN = dict(forbid_duplicate_ngrams=False, min_len=0)
BLOCKED = dict(forbid_duplicate_ngrams=True, ngram_size=2, min_len=3)
TRACES = ("pred_seq", "scores", "wids", "ptrs")
NBEST = ("nbest_seq", "nbest_score", "nbest_value", "nbest_len", "nbest_ok")


@functools.lru_cache(maxsize=None)
def model_inputs():
    p = O.init_params(vocab_size=MK["vocab_size"], layers=MK["layers"], tasks=MK["tasks"], seed=MK["seed"], std=MK["std"])
    dv = [t.to(DEV) for t in decode_inputs(NB, NT, 213)]
    return p, [dv[0].half(), dv[1].half()] + dv[2:]


def make_model(**kw):
    p = model_inputs()[0]
    cfg = BertConfig(MK["vocab_size"], num_hidden_layers=MK["layers"], type_vocab_size=6)
    m = BertForSeq2SeqDecoder(cfg, mask_word_id=S.MASK_ID, eos_id=S.SEP_ID, enable_butd=True, len_vis_input=100, length_penalty=0.4, **kw)
    sd = dict(p)
    sd["cls.predictions.decoder.weight"] = p["bert.embeddings.word_embeddings.weight"]
    m.load_state_dict(sd, strict=True)
    return m.half().to(DEV).eval()


def search(m, **attrs):
    for k, v in attrs.items():
        setattr(m, k, v)
    with torch.no_grad():
        tr = m(*model_inputs()[1], task_idx=None)
    return {k: v.cpu() for k, v in tr.items()}


def equal_dicts(a, b):
    return set(a) == set(b) and all(a[k].dtype == b[k].dtype and torch.equal(GU.bits(a[k]), GU.bits(b[k])) for k in a)


def check_invariants(tr, m, K, G):
    """Parents stay inside their group; the n-best outputs are the host specification's on the returned traces."""
    Kg = K // G
    ptrs = tr["ptrs"][:, 1:NT].numpy()
    assert np.array_equal(ptrs // Kg, np.broadcast_to(np.arange(K) // Kg, ptrs.shape)), ptrs
    assert not tr["ptrs"][:, 0].any()
    frames = [tr[k][:, :NT].permute(1, 0, 2).contiguous().numpy() for k in ("scores", "wids", "ptrs")]
    N = tr["nbest_seq"].shape[1]
    want = beam_nbest_host(*frames, N, m.eos_id, m.length_penalty, tr["pred_seq"].shape[1])
    for name, w in zip(NBEST, want):
        got = tr[name].numpy()
        assert np.array_equal(np.ascontiguousarray(got).view(np.uint8), np.ascontiguousarray(by_image(w, N)).view(np.uint8)), name
    assert torch.equal(tr["nbest_seq"][:, 0], tr["pred_seq"])


def first_words_differ(tr, K, G):
    """Every frame before an eos appears: the first-ranked words of the G groups are pairwise different.  Returns the frames checked."""
    wids = tr["wids"][:, :NT].numpy()
    checked = 0
    for b in range(NB):
        for s in range(NT):
            if (wids[b, s] == S.SEP_ID).any():
                break
            heads = wids[b, s, ::K // G].tolist()
            assert len(set(heads)) == G, (b, s, wids[b, s])
            checked += 1
    return checked


@pytest.mark.parametrize("K,G,lam,extra", [(4, 2, 0.5, PLAIN), (6, 3, 100.0, PLAIN), (4, 2, 0.5, BLOCKED)], ids=["K4_G2", "K6_G3_l100", "K4_G2_ngram_min_len_3"])
def test_device_selection_equals_the_host_path(K, G, lam, extra):
    m = make_model(search_beam_size=K, n_best=K, beam_groups=G, diversity_penalty=lam, **extra)
    assert m.group_select == "device" and m.ngram_blocking == "device"
    on_host = search(m, group_select="host")
    check_invariants(on_host, m, K, G)
    if lam == 100.0:
        assert first_words_differ(on_host, K, G) >= NB                  # the specification first,
    on_dev = search(m, group_select="device")
    assert set(on_dev) == set(TRACES + NBEST) and equal_dicts(on_dev, on_host)
    check_invariants(on_dev, m, K, G)
    if lam == 100.0:
        assert first_words_differ(on_dev, K, G) >= NB                   # then the kernel
    if extra is BLOCKED:                                                # min_len = 3: no hypothesis of the list is shorter; no bigram twice
        ok, ln = on_dev["nbest_ok"].numpy(), on_dev["nbest_len"].numpy()
        assert (ln[ok == 1] >= 3).all()
        for b in range(NB):
            for n in range(K):
                w = on_dev["nbest_seq"][b, n, :ln[b, n]].tolist()
                grams = list(zip(w, w[1:]))
                assert not ok[b, n] or len(set(grams)) == len(grams), w
    # the penalty does something: the plain search of the same size keeps fewer distinct first words
    if extra is PLAIN:
        plain = search(make_model(search_beam_size=K, n_best=K, **extra))
        heads = lambda tr: sum(len(set(tr["wids"][b, 1].tolist())) for b in range(NB))
        print("distinct words in frame 1: plain %d, G=%d lambda=%g %d" % (heads(plain), G, lam, heads(on_dev)))
        assert not equal_dicts(plain, on_dev)


def test_one_group_is_the_decoder_without_the_keywords():
    a = search(make_model(search_beam_size=4, n_best=4, **BLOCKED))
    b = search(make_model(search_beam_size=4, n_best=4, beam_groups=1, diversity_penalty=0.0, **BLOCKED))
    assert equal_dicts(a, b)
    m = make_model(search_beam_size=4, beam_groups=1)
    m.diversity_penalty = 0.5
    with pytest.raises(ValueError, match="diversity_penalty=0.5"), torch.no_grad():
        m(*model_inputs()[1], task_idx=None)
    m.diversity_penalty, m.beam_groups = 0.0, 3
    with pytest.raises(ValueError, match="beam_groups=3"), torch.no_grad():
        m(*model_inputs()[1], task_idx=None)
    m.beam_groups, m.group_select = 2, "gpu"
    with pytest.raises(ValueError, match="group_select"), torch.no_grad():
        m(*model_inputs()[1], task_idx=None)
    with pytest.raises(ValueError, match="diversity"):
        m.engine.decode_beam(*model_inputs()[1], S.MASK_ID, 4, S.SEP_ID, groups=1, diversity=0.5)


def test_run_capture_replay_and_a_used_decoder_equals_a_fresh_one():
    """Three consecutive calls (run, capture, replay) return the same bits; then a decoder that alternated G, lambda, blocking and plain beam
    calls returns, for each kind of call, what a fresh decoder returns: (G, lambda) is part of the plan key, so no call replays another's."""
    kinds = [dict(beam_groups=2, diversity_penalty=0.02, **PLAIN), dict(beam_groups=2, diversity_penalty=100.0, **PLAIN),
             dict(beam_groups=4, diversity_penalty=0.5, **PLAIN), dict(beam_groups=1, diversity_penalty=0.0, **PLAIN),
             dict(beam_groups=2, diversity_penalty=0.02, **BLOCKED), dict(beam_groups=1, diversity_penalty=0.0, **BLOCKED)]
    fresh = [search(make_model(search_beam_size=4, n_best=4, **kw)) for kw in kinds[:3]]
    fresh += [search(make_model(search_beam_size=4, n_best=4, **kw)) for kw in kinds[3:]]
    for i, j in ((0, 1), (0, 2), (0, 3), (4, 5)):             # the calls that differ in one part of the plan key return different frames
        assert not equal_dicts(fresh[i], fresh[j]), (i, j)
    used = make_model(search_beam_size=4, n_best=4)
    for rep in range(3):
        assert equal_dicts(search(used, **kinds[0]), fresh[0]), rep
    for order in ((1, 0, 2, 3, 4, 5), (5, 4, 0, 3, 2, 1, 0)):
        for i in order:
            assert equal_dicts(search(used, **kinds[i]), fresh[i]), (order, i)


# ------------------------------------------------------------------------------------------------
# python -m vlp_amd.decode_img2txt --beam_groups
# ------------------------------------------------------------------------------------------------
NV, TC, VOCAB = 100, 8, 1024
LIST = [("test", 391895), ("val", 522418), ("test", 184613), ("test", 318219)]


def fname(i):
    return "COCO_val2014_%012d.jpg" % i


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    """A packed store of 3 images, a 2-layer checkpoint, a vocabulary, a Karpathy-style image list with references and a document-frequency table."""
    root = str(tmp_path_factory.mktemp("diverse_cli"))
    rng = np.random.RandomState(9)
    test_ids = [i for sp, i in LIST if sp == "test"]
    n = len(test_ids)
    keys = [fname(i)[:-4] for i in reversed(test_ids)]
    feats = np.abs(rng.randn(n, NV, 2048)).astype(np.float16)
    cls = rng.rand(n, NV, 1601).astype(np.float32)
    cls /= cls.sum(-1, keepdims=True)
    xy = rng.rand(n, NV, 2, 2) * 400
    boxes = np.concatenate([xy.min(2), xy.max(2) + 1.0, np.zeros((n, NV, 1)), rng.rand(n, NV, 1)], axis=-1).astype(np.float32)
    store = os.path.join(root, "store")
    write_packed(store, keys, feats, cls, boxes)
    bert = os.path.join(root, "bert")
    os.makedirs(bert)
    with open(os.path.join(bert, "bert_config.json"), "w") as f:
        f.write(BertConfig(VOCAB, num_hidden_layers=2, type_vocab_size=2).to_json_string())
    special = {S.PAD_ID: "[PAD]", S.UNK_ID: "[UNK]", S.CLS_ID: "[CLS]", S.SEP_ID: "[SEP]", S.MASK_ID: "[MASK]"}
    with open(os.path.join(bert, "vocab.txt"), "w") as f:
        f.write("\n".join(special.get(i, "w%d" % i) for i in range(VOCAB)) + "\n")
    p = O.init_params(vocab_size=VOCAB, layers=2, tasks="img2txt", seed=27, std=0.1)
    sd = dict(p)
    sd["cls.predictions.decoder.weight"] = p["bert.embeddings.word_embeddings.weight"]
    ckpt = os.path.join(root, "model.3.bin")
    torch.save(sd, ckpt)
    src = os.path.join(root, "dataset.json")
    with open(src, "w") as f:
        json.dump({"images": [{"split": sp, "filename": fname(i), "filepath": "val2014", "imgid": k,
                               "sentences": [{"tokens": ["w%d" % t for t in rng.randint(300, 340, size=5)]} for _ in range(2)]}
                              for k, (sp, i) in enumerate(LIST)]}, f)
    ex = [(i, [int(t) for t in rng.randint(300, 340, size=rng.randint(2, TC + 1))]) for i in range(40) for _ in range(3)]
    df = os.path.join(root, "df.npz")
    SC.DocFreq.from_examples(ex, TC, S.SEP_ID).save(df)
    return dict(root=root, store=store, bert=bert, ckpt=ckpt, src=src, test_ids=test_ids, df=df)


def run(su, name, *extra):
    out = os.path.join(su["root"], name)
    res = D.main(["--bert_model", su["bert"], "--model_recover_path", su["ckpt"], "--packed_features", su["store"], "--src_file", su["src"],
                  "--split", "test", "--dataset", "coco", "--output_file", out, "--batch_size", "2", "--beam_size", "4", "--forbid_duplicate_ngrams",
                  "--ngram_size", "2", "--min_len", "2", "--max_tgt_length", str(TC), "--new_segment_ids", "--fp16", "--enable_butd"] + list(extra))
    with open(out) as f:
        text = f.read()
    assert res == {su["ckpt"]: json.loads(text)}
    return text


def test_cli_beam_groups_1_changes_no_byte(setup):
    plain = run(setup, "plain.json")
    assert run(setup, "one.json", "--beam_groups", "1") == plain
    assert run(setup, "one_zero.json", "--beam_groups", "1", "--diversity_penalty", "0") == plain
    assert [r["image_id"] for r in json.loads(plain)] == setup["test_ids"]


def test_cli_diverse_beam_with_consensus(setup, monkeypatch):
    su = setup
    calls = []
    real = CS.consensus_select_device

    def spy(ids, n_samples, df, **kw):
        pick, utility = real(ids, n_samples, df, **kw)
        calls.append((ids.clone(), n_samples, df, pick, utility))
        return pick, utility
    monkeypatch.setattr(CS, "consensus_select_device", spy)
    nb = os.path.join(su["root"], "nbest_d.json")
    out = os.path.join(su["root"], "diverse.json")
    sel = json.loads(run(su, "diverse.json", "--beam_groups", "2", "--diversity_penalty", "1.0", "--n_best", "4", "--select", "consensus",
                         "--consensus_df", su["df"], "--nbest_file", nb))
    assert [r["image_id"] for r in sel] == su["test_ids"]
    assert all(set(r) == {"image_id", "caption", "rank", "logprob", "utility"} for r in sel)
    ids_read, hyps_read = EC.load_predictions(out, EC.references_of(su["src"], "test", "coco"))       # what eval_captions reads
    assert ids_read == su["test_ids"] and len(hyps_read) == len(sel)
    with open(nb) as f:
        per = {}
        for r in json.load(f):
            per.setdefault(r["image_id"], []).append(r)
    assert list(per) == su["test_ids"]
    assert len(calls) == 2 and all(tuple(c[0].shape) == (8, TC) and c[1] == 4 for c in calls)         # 3 images in batches of 2, rank-major rows
    sure = 0
    for n, (ids, _, df, pick, utility) in enumerate(calls):
        want, want_pick = CS.consensus_utility(ids, 4, df)                                            # the fp64 host specification on the same rows
        assert float(np.abs(utility.double().cpu().numpy() - want).max()) <= CU.bound(TC, 4)
        sure += CU.check_pick(pick.cpu().numpy(), utility.cpu().numpy(), want, 4, TC)
        u = utility.view(4, 2).cpu()
        for b in range(2 if n < 1 else 1):
            r = sel[2 * n + b]
            assert r["rank"] == int(pick[b]) and r["utility"] == float(u[r["rank"], b])
            written = {h["rank"]: h for h in per[r["image_id"]]}
            assert r["rank"] in written and r["caption"] == written[r["rank"]]["caption"] and r["logprob"] == written[r["rank"]]["logprob"]
            for k in range(4):                                                                        # the rows scored are the hypotheses written
                assert (k in written) or not bool(ids[k * 2 + b].any())
                if k in written:
                    assert written[k]["utility"] == float(u[k, b])
                    assert written[k]["caption"] == D.caption_of(ids[k * 2 + b].tolist() + [S.PAD_ID], D.Vocab(os.path.join(su["bert"], "vocab.txt")),
                                                                 S.SEP_ID, S.PAD_ID)
    print("consensus over the diverse beam: %d picks decisive on the host; picks %s" % (sure, [r["rank"] for r in sel]))
