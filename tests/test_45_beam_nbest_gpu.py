"""GPU: the n-best list of a beam search on the device (vlp_beam_nbest, Engine.beam_nbest, BertForSeq2SeqDecoder(n_best=..) / backtrack="device",
python -m vlp_amd.decode_img2txt --n_best).

  * the kernel against vlp_amd.nbest.beam_nbest_host (numpy, fp64) on synthetic frames: seq / len / ok exactly, value / score bit for bit;
    guard bands, poisoned outputs, zero padding, two runs bit-equal, refusals by return code without a launch;
  * the model: the device back-tracking equals the host's and the reference fixture; the n-best outputs equal the host specification applied to
    the returned traces, with n-gram blocking on the device / on the host / off;
  * the command line: --n_best 1 changes no byte, the n-best file, --select consensus against consensus.consensus_utility, --select logprob.
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
from oracle.make_golden import BEAM_CASES, decode_inputs, decode_fingerprint   # noqa: E402  (pure helpers)
from tests import consensus_util as CU                              # noqa: E402
from tests import guard_util as GU                                  # noqa: E402
from vlp_amd import _lib as K_                                      # noqa: E402
from vlp_amd import consensus as CS                                 # noqa: E402
from vlp_amd import decode_img2txt as D                             # noqa: E402
from vlp_amd import scst as SC                                      # noqa: E402
from vlp_amd import synthetic as S                                  # noqa: E402
from vlp_amd.data import write_packed                               # noqa: E402
from vlp_amd.modeling import BertConfig, BertForSeq2SeqDecoder      # noqa: E402
from vlp_amd.nbest import beam_nbest_host, by_image                 # noqa: E402

DEV = torch.device("cuda:0")
GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EOS = 3

# ------------------------------------------------------------------------------------------------
# vlp_beam_nbest against the host specification
# ------------------------------------------------------------------------------------------------
# (B, K, F, N, shift): image b is forced into kind KINDS[(b + shift) % 4].  The small shapes are the smallest at which each mechanism can go
# wrong (N = 1, N = K, one frame); (2, 64, 70, 16) has more candidates than lanes and F > 64; (1, 64, 256, 64) is every limit at once.
KINDS = ("early_last_and_dead_paths", "no_eos", "all_minus_inf", "random")
SHAPES = [(3, 3, 6, 1, 0), (3, 3, 6, 3, 0), (2, 5, 12, 5, 0), (1, 2, 1, 2, 3), (2, 64, 70, 16, 2), (1, 64, 256, 64, 3)]
PENALTIES = [0.0, 0.4, -0.3]


@functools.lru_cache(maxsize=None)
def frames(B, K, F, shift):
    """Random frames: back pointers in [0, K), scores from 4 values (ties decide most ranks), 10 % -inf, 20 % eos; then the forced images."""
    rng = np.random.RandomState(1000 * F + 10 * K + B)
    tot = rng.choice(np.array([-1.5, -0.75, -2.25, -3.0], dtype=np.float32), size=(F, B, K))
    tot[rng.rand(F, B, K) < 0.1] = -np.inf
    wids = rng.randint(4, 12, size=(F, B, K)).astype(np.int64)
    wids[rng.rand(F, B, K) < 0.2] = EOS
    ptrs = rng.randint(0, K, size=(F, B, K)).astype(np.int64)
    kinds = []
    for b in range(B):
        kind = KINDS[(b + shift) % 4]
        kinds.append(kind)
        if kind == "early_last_and_dead_paths" and F >= 3:
            wids[F // 2, b, :] = EOS                  # a frame in the middle whose K words are all eos: `last` comes early
            wids[0, b, 0], wids[0, b, 1:] = EOS, 5    # and every hypothesis longer than one word runs through an eos at its start: ok = 0
            ptrs[1, b, :] = 0
        elif kind == "no_eos":
            wids[:, b, :][wids[:, b, :] == EOS] = 5
        elif kind == "all_minus_inf":
            tot[:, b, :] = -np.inf
    for a in (tot, wids, ptrs):
        a.setflags(write=False)
    return tot, wids, ptrs, tuple(kinds)


def out_len_of(F):
    return F + F % 3                                  # 6 -> 6, 12 -> 12, 1 -> 2, 70 -> 71, 256 -> 257: with and without padding columns


@functools.lru_cache(maxsize=None)
def host(B, K, F, N, shift, lp):
    """The specification's five arrays for a case; computed once, read only."""
    tot, wids, ptrs, _ = frames(B, K, F, shift)
    out = beam_nbest_host(tot, wids, ptrs, N, EOS, lp, out_len_of(F))
    for a in out:
        a.setflags(write=False)
    return out


def device_inputs(B, K, F, shift):
    return [torch.from_numpy(np.array(a)).to(DEV) for a in frames(B, K, F, shift)[:3]]


def guarded_outputs(rows, T):
    return (GU.guarded(rows, T, dtype=torch.int64, fill="sentinel", device=DEV), GU.guarded_vec(rows, torch.float32, "sentinel", device=DEV),
            GU.guarded_vec(rows, torch.float64, "sentinel", device=DEV), GU.guarded_vec(rows, torch.int32, "sentinel", device=DEV),
            GU.guarded_vec(rows, torch.uint8, "sentinel", device=DEV))


def launch(ins, N, lp, outs):
    seq, score, value, length, ok = outs
    K_.beam_nbest(ins[0], ins[1], ins[2], N, EOS, lp, seq.view, score.vec, value.vec, length.vec, ok.vec)


def same_bits(got, want):
    return np.array_equal(np.ascontiguousarray(got).view(np.uint8), np.ascontiguousarray(want).view(np.uint8))


@pytest.mark.parametrize("lp", PENALTIES)
@pytest.mark.parametrize("B,K,F,N,shift", SHAPES, ids=["B%d_K%d_F%d_N%d" % s[:4] for s in SHAPES])
def test_kernel_equals_the_host_specification(B, K, F, N, shift, lp):
    T = out_len_of(F)
    want = host(B, K, F, N, shift, lp)
    outs = guarded_outputs(N * B, T)
    launch(device_inputs(B, K, F, shift), N, lp, outs)
    torch.cuda.synchronize()
    seq, score, value, length, ok = [g.view.cpu().numpy().reshape(w.shape) for g, w in zip(outs, want)]
    assert np.array_equal(seq, want[0]), "seq"
    assert np.array_equal(length, want[3]) and np.array_equal(ok, want[4]), (length, want[3], ok, want[4])
    assert same_bits(value, want[2]), (value, want[2])
    assert same_bits(score, want[1]), (score, want[1])
    for g, name in zip(outs, ("seq", "score", "value", "len", "ok")):
        GU.assert_untouched(g, written="logical", name=name)             # nothing outside [N*B, T] / [N*B]
        GU.assert_written(g, written="logical", name=name)               # and no poison left inside: the padding is written, as zeros
    assert (seq[np.arange(T)[None, :] >= length[:, None]] == 0).all()
    # what the forced images are there for
    kinds = frames(B, K, F, shift)[3]
    o, ln = by_image(ok, N), by_image(length, N)
    for b, kind in enumerate(kinds):
        if kind == "all_minus_inf":
            assert (ln[b] == 0).all() and (o[b] == 0).all() and (by_image(seq, N)[b] == 0).all()
        elif kind == "no_eos":
            assert (ln[b][np.isfinite(by_image(value, N)[b])] == F).all()          # only the last frame has candidates
        elif kind == "early_last_and_dead_paths" and F >= 3:
            assert (ln[b] <= F // 2 + 1).all() and (o[b][ln[b] > 1] == 0).all()


def test_forced_cases_reach_every_kind_of_row():
    """The cases above, taken together, hold rows that are not ok although they are finite, ranks decided by ties, and -inf ranks."""
    dead = ties = empty = 0
    for B, K, F, N, shift in SHAPES:
        for lp in PENALTIES:
            seq, score, value, length, ok = host(B, K, F, N, shift, lp)
            dead += int(((ok == 0) & (length > 0)).sum())
            empty += int((length == 0).sum())
            v = by_image(value, N)
            ties += int((v[:, 1:] == v[:, :-1]).sum())
    assert dead > 10 and ties > 10 and empty > 10, (dead, ties, empty)


def test_two_runs_are_bit_equal():
    B, K, F, N, shift = SHAPES[4]
    ins = device_inputs(B, K, F, shift)
    runs = []
    for _ in range(2):
        outs = guarded_outputs(N * B, out_len_of(F))
        launch(ins, N, 0.4, outs)
        torch.cuda.synchronize()
        runs.append([GU.bits(g.view).cpu() for g in outs])
    assert all(torch.equal(a, b) for a, b in zip(*runs))


@pytest.mark.parametrize("what", ["N_gt_K", "N_zero", "F_gt_256", "T_lt_F", "null_ok", "null_tot"])
def test_refusals_by_return_code(what):
    B, K, F, N = 2, 3, 6, 2
    if what == "F_gt_256":
        F = 257
    T = F - 1 if what == "T_lt_F" else F
    N = {"N_gt_K": 4, "N_zero": 0}.get(what, N)
    tot = torch.zeros(F, B, K, device=DEV)
    wids, ptrs = torch.zeros(F, B, K, dtype=torch.long, device=DEV), torch.zeros(F, B, K, dtype=torch.long, device=DEV)
    outs = guarded_outputs(max(N, 1) * B, T)
    seq, score, value, length, ok = outs
    with pytest.raises(RuntimeError, match="vlp_beam_nbest"):
        K_.beam_nbest(None if what == "null_tot" else tot, wids, ptrs, N, EOS, 0.0, seq.view, score.vec, value.vec, length.vec,
                      None if what == "null_ok" else ok.vec)
    torch.cuda.synchronize()
    for g, name in zip(outs, ("seq", "score", "value", "len", "ok")):
        GU.assert_untouched(g, written=None, name=name)                 # nothing was launched


# ------------------------------------------------------------------------------------------------
# the model
# ------------------------------------------------------------------------------------------------
CASE = "beam_2l_K3"


@functools.lru_cache(maxsize=None)
def model_case():
    mk, B, T, seed, dk = BEAM_CASES[CASE]
    g = dict(np.load(os.path.join(GOLDEN_DIR, CASE + ".npz")))
    p = O.init_params(vocab_size=mk["vocab_size"], layers=mk["layers"], tasks=mk["tasks"], seed=mk["seed"], std=mk["std"])
    inp = decode_inputs(B, T, seed)
    same_stream = bool(np.allclose(decode_fingerprint(p, inp), g["fingerprint"], rtol=1e-9, atol=0))
    dv = [t.to(DEV) for t in inp]
    return mk, B, T, dict(dk), p, [dv[0].half(), dv[1].half()] + dv[2:], g, same_stream


def make_model(**kw):
    mk, B, T, dk, p = model_case()[:5]
    cfg = BertConfig(mk["vocab_size"], num_hidden_layers=mk["layers"], type_vocab_size=6)
    m = BertForSeq2SeqDecoder(cfg, mask_word_id=S.MASK_ID, eos_id=S.SEP_ID, enable_butd=True, len_vis_input=100, **dict(dk, **kw))
    sd = dict(p)
    sd["cls.predictions.decoder.weight"] = p["bert.embeddings.word_embeddings.weight"]
    m.load_state_dict(sd, strict=True)
    return m.half().to(DEV).eval()


@functools.lru_cache(maxsize=None)
def host_path_traces():
    """The dict of the search as it was (n_best = 1, backtrack = "host"), on the CPU; computed once, read only."""
    m = make_model()
    assert m.backtrack == "host" and m.n_best == 1
    with torch.no_grad():
        tr = m(*model_case()[5], task_idx=None)
    assert set(tr) == {"pred_seq", "scores", "wids", "ptrs"}
    return {k: v.cpu() for k, v in tr.items()}


def frames_of(tr, T):
    """[B, L, K] traces -> the T frames [T, B, K] the search produced."""
    return [tr[k][:, :T].permute(1, 0, 2).contiguous().cpu().numpy() for k in ("scores", "wids", "ptrs")]


def check_against_host_specification(tr, m, N, T):
    B, L = tr["pred_seq"].shape
    want = beam_nbest_host(*frames_of(tr, T), N, m.eos_id, m.length_penalty, L)
    names = ("nbest_seq", "nbest_score", "nbest_value", "nbest_len", "nbest_ok")
    dtypes = (torch.int64, torch.float32, torch.float64, torch.int32, torch.uint8)
    for name, dt, w in zip(names, dtypes, want):
        got = tr[name]
        assert got.is_cuda and got.dtype == dt and tuple(got.shape) == (B, N) + ((L,) if name == "nbest_seq" else ()), name
        assert same_bits(got.cpu().numpy(), by_image(w, N)), name
    assert torch.equal(tr["nbest_seq"][:, 0], tr["pred_seq"])


def test_device_backtrack_equals_the_host_path_and_the_fixture(monkeypatch):
    mk, B, T, dk, p, inputs, g, same_stream = model_case()
    want = host_path_traces()
    m = make_model()
    m.backtrack = "device"

    def no_host(*a, **k):
        raise AssertionError("the device path must not back-track on the host")
    monkeypatch.setattr(BertForSeq2SeqDecoder, "_backtrack_batch", no_host)
    with torch.no_grad():
        tr = m(*inputs, task_idx=None)
    assert tr["pred_seq"].is_cuda and tr["pred_seq"].dtype == torch.int64
    for k in want:
        assert torch.equal(tr[k].cpu(), want[k]), k
    if same_stream:
        assert np.array_equal(tr["pred_seq"].cpu().numpy(), g["pred_seq"])
    check_against_host_specification(tr, m, 1, T)
    for rep in range(2):                  # later calls replay the captured token steps; the dict owns its tensors
        with torch.no_grad():
            tr2 = m(*[t.clone() for t in inputs], task_idx=None)
        assert all(torch.equal(tr[k], tr2[k]) and tr[k].data_ptr() != tr2[k].data_ptr() for k in tr), rep


@pytest.mark.parametrize("variant", ["ngram_device_min_len_2", "ngram_host", "plain"])
def test_model_n_best_equals_the_host_specification(variant):
    mk, B, T, dk, p, inputs, g, same_stream = model_case()
    assert dk["forbid_duplicate_ngrams"] and dk["min_len"] == 2 and dk["search_beam_size"] == 3
    m = make_model(n_best=3, **(dict(forbid_duplicate_ngrams=False, min_len=0) if variant == "plain" else {}))
    m.ngram_blocking = "host" if variant == "ngram_host" else "device"
    with torch.no_grad():
        tr = m(*inputs, task_idx=None)
    check_against_host_specification(tr, m, 3, T)
    if variant != "plain":
        want = host_path_traces()
        for k in want:
            assert torch.equal(tr[k].cpu(), want[k]), k               # rank 0 and the traces are the search's as it was
        if same_stream:
            assert np.array_equal(tr["pred_seq"].cpu().numpy(), g["pred_seq"])
    ok, ln = tr["nbest_ok"].cpu().numpy(), tr["nbest_len"].cpu().numpy()
    assert ok[:, 0].all() and (ln[:, 0] >= (2 if variant != "plain" else 1)).all()
    for b in range(B):                    # the finished hypotheses of one search are different captions
        rows = [tuple(tr["nbest_seq"][b, n, :ln[b, n]].tolist()) for n in range(3) if ok[b, n]]
        assert len(set(rows)) == len(rows)
    with torch.no_grad():
        tr2 = m(*[t.clone() for t in inputs], task_idx=None)
    assert all(torch.equal(tr[k], tr2[k]) for k in tr)


def test_model_refuses_more_hypotheses_than_beams():
    with pytest.raises(ValueError, match="n_best=4"):
        make_model(n_best=4)
    m = make_model(n_best=3)
    m.n_best = 4
    with pytest.raises(ValueError, match="n_best=4"), torch.no_grad():
        m(*model_case()[5], task_idx=None)
    m.n_best, m.backtrack = 1, "gpu"
    with pytest.raises(ValueError, match="backtrack"), torch.no_grad():
        m(*model_case()[5], task_idx=None)


# ------------------------------------------------------------------------------------------------
# python -m vlp_amd.decode_img2txt --n_best
# ------------------------------------------------------------------------------------------------
NV, TC, VOCAB = 100, 10, 1024
LIST = [("test", 391895), ("val", 522418), ("test", 184613), ("test", 318219), ("val", 554625), ("test", 574769), ("test", 60623)]


def fname(i):
    return "COCO_val2014_%012d.jpg" % i


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    """A packed store of 5 images, a 2-layer checkpoint, a vocabulary, a Karpathy-style image list and a document-frequency table."""
    root = str(tmp_path_factory.mktemp("nbest_cli"))
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
    with open(os.path.join(bert, "vocab.txt"), "w") as f:
        f.write("\n".join(special.get(i, "w%d" % i) for i in range(VOCAB)) + "\n")
    p = O.init_params(vocab_size=VOCAB, layers=2, tasks="img2txt", seed=27, std=0.1)
    sd = dict(p)
    sd["cls.predictions.decoder.weight"] = p["bert.embeddings.word_embeddings.weight"]
    ckpt = os.path.join(root, "model.3.bin")
    torch.save(sd, ckpt)
    src = os.path.join(root, "dataset.json")
    with open(src, "w") as f:
        json.dump({"images": [{"split": sp, "filename": fname(i), "filepath": "val2014", "imgid": n} for n, (sp, i) in enumerate(LIST)]}, f)
    # 40 images x 3 captions over the words 300..339: most n-grams of a decoded caption miss the table (df 0)
    ex = [(i, [int(t) for t in rng.randint(300, 340, size=rng.randint(2, TC + 1))]) for i in range(40) for _ in range(3)]
    df = os.path.join(root, "df.npz")
    SC.DocFreq.from_examples(ex, TC, S.SEP_ID).save(df)
    su = dict(root=root, store=store, bert=bert, ckpt=ckpt, src=src, test_ids=test_ids, df=df)
    su["plain"] = run(su, "plain.json")                               # the tool without the new flags: what the others are compared with
    return su


def argv(su, out, *extra):
    return ["--bert_model", su["bert"], "--model_recover_path", su["ckpt"], "--packed_features", su["store"], "--src_file", su["src"], "--split", "test",
            "--dataset", "coco", "--output_file", out, "--batch_size", "2", "--beam_size", "3", "--forbid_duplicate_ngrams", "--ngram_size", "2",
            "--min_len", "2", "--max_tgt_length", str(TC), "--new_segment_ids", "--fp16", "--enable_butd"] + list(extra)


def run(su, name, *extra):
    """D.main with --output_file <root>/<name>; returns the file's text."""
    out = os.path.join(su["root"], name)
    res = D.main(argv(su, out, *extra))
    with open(out) as f:
        text = f.read()
    assert res == {su["ckpt"]: json.loads(text)}
    return text


def by_image_id(records):
    out = {}
    for r in records:
        out.setdefault(r["image_id"], []).append(r)
    return out


def test_cli_n_best_1_changes_no_byte(setup):
    su = setup
    assert run(su, "one.json", "--n_best", "1") == su["plain"]
    plain = json.loads(su["plain"])
    assert [r["image_id"] for r in plain] == su["test_ids"] and len(set(r["caption"] for r in plain)) > 1


def test_cli_nbest_file(setup):
    su = setup
    nb = os.path.join(su["root"], "nbest.json")
    assert run(su, "three.json", "--n_best", "3", "--nbest_file", nb) == su["plain"]          # --select none: rank 0, the same file
    with open(nb) as f:
        hyps = json.load(f)
    assert all(set(r) == {"image_id", "rank", "caption", "logprob", "value"} for r in hyps)
    per = by_image_id(hyps)
    assert list(per) == su["test_ids"]                                                        # input order, ranks ascending within an image
    for r0, (imgid, rs) in zip(json.loads(su["plain"]), per.items()):
        ranks = [r["rank"] for r in rs]
        assert ranks[0] == 0 and ranks == sorted(set(ranks)) and ranks[-1] <= 2
        assert rs[0]["caption"] == r0["caption"]
        assert all(a["value"] >= b["value"] for a, b in zip(rs, rs[1:]))
        assert len(set(r["caption"] for r in rs)) == len(rs)
    assert max(len(rs) for rs in per.values()) >= 2
    # the alias
    nb2 = os.path.join(su["root"], "nbest_alias.json")
    run(su, "three_alias.json", "--n_best", "3", "--samples_file", nb2)
    with open(nb2) as f:
        assert json.load(f) == hyps


def test_cli_select_consensus(setup, monkeypatch):
    su = setup
    calls = []
    real = CS.consensus_select_device

    def spy(ids, n_samples, df, **kw):
        pick, utility = real(ids, n_samples, df, **kw)
        calls.append((ids.clone(), n_samples, df, pick, utility))
        return pick, utility
    monkeypatch.setattr(CS, "consensus_select_device", spy)
    nb = os.path.join(su["root"], "nbest_c.json")
    sel = json.loads(run(su, "consensus.json", "--n_best", "3", "--select", "consensus", "--consensus_df", su["df"], "--nbest_file", nb))
    with open(nb) as f:
        per = by_image_id(json.load(f))
    assert [r["image_id"] for r in sel] == su["test_ids"]
    assert all(set(r) == {"image_id", "caption", "rank", "logprob", "utility"} for r in sel)
    assert len(calls) == 3 and all(tuple(c[0].shape) == (6, TC) and c[1] == 3 for c in calls)   # 5 images in batches of 2, rank-major rows
    sure = 0
    for n, (ids, _, df, pick, utility) in enumerate(calls):
        assert torch.equal(ids, SC.clean_captions(ids, S.SEP_ID, S.PAD_ID))
        want, want_pick = CS.consensus_utility(ids, 3, df)                                    # the fp64 host specification on the same rows
        assert float(np.abs(utility.double().cpu().numpy() - want).max()) <= CU.bound(TC, 3)
        sure += CU.check_pick(pick.cpu().numpy(), utility.cpu().numpy(), want, 3, TC)         # the host's pick wherever it is decisive
        u = utility.view(3, 2).cpu()
        for b in range(2 if n < 2 else 1):                                                    # the last batch holds one image and one padding row
            r = sel[2 * n + b]
            assert r["rank"] == int(pick[b]) and r["utility"] == float(u[r["rank"], b])
            written = {h["rank"]: h for h in per[r["image_id"]]}
            assert r["rank"] in written and r["caption"] == written[r["rank"]]["caption"] and r["logprob"] == written[r["rank"]]["logprob"]
            for k in range(3):                                                                # what is not a hypothesis was emptied before the scoring
                assert (k in written) or not bool(ids[k * 2 + b].any())
                assert (k not in written) or written[k]["utility"] == float(u[k, b])
    print("consensus over the beam: %d of %d picks decisive on the host; picks %s" % (sure, 6, [r["rank"] for r in sel]))
    assert sure >= 1 and any(r["utility"] > 0 for r in sel)


def test_cli_select_logprob(setup):
    su = setup
    nb = os.path.join(su["root"], "nbest_l.json")
    sel = json.loads(run(su, "logprob.json", "--n_best", "3", "--select", "logprob", "--length_penalty", "0.4", "--nbest_file", nb))
    with open(nb) as f:
        per = by_image_id(json.load(f))
    assert [r["image_id"] for r in sel] == su["test_ids"]
    for r in sel:
        rs = per[r["image_id"]]                                       # the ok hypotheses (rank 0 is one of them here)
        lps = [h["logprob"] for h in rs]
        best = rs[lps.index(max(lps))]                                # the first of the largest
        assert set(r) == {"image_id", "caption", "rank", "logprob", "utility"} and r["utility"] is None
        assert (r["rank"], r["caption"], r["logprob"]) == (best["rank"], best["caption"], best["logprob"])
