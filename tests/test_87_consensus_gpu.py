"""GPU: consensus selection among the K samples of an image (vlp_cider_d_consensus, csrc/reward.hip) against the project's host specification
(vlp_amd.consensus.consensus_utility: scst.CiderD(df=<DocFreq>) in fp64, every sample against the image's other K - 1).
tests/test_consensus_cpu.py checks that specification against an independent restatement; tests/consensus_util.py holds what the two share.

(a) utilities within bound(T, K) of the host on eight cases and two tables (one with df far beyond 16 bits); before the kernel's output is
    looked at, every group has a non-zero host utility.  The pick: the first argmax of the device's own utilities exactly, never worse than the
    host maximum by more than 2 bound, and the host's pick wherever the host's two largest differ by more than 2 bound -- at least half of
    the groups of every case with T >= 21 (asserted on the host alone);
(b) pair: every off-diagonal entry within the per-score bound of the host score with that single reference, the diagonal 0, and utilities and
    picks the same bits with pair = NULL;
(c) K identical rows; hand-built hard rows (ids 65535 / 70000, keys around 2^63, df == n_docs, garbage behind the first 0);
(d) the contract: strided rows with poisoned padding, guard bands around every output and the workspace, bit-equal repeats, one graph capture
    and replay, refusals by return code;
(e) end to end: decode_sample_group -> clean_captions -> consensus_select_device on a 2-layer model, and python -m vlp_amd.sample_img2txt
    --select.

Bound: bound(T, K) = (4 T + 16) * 2^-24 * 10 + 2 (K + 1) * 2^-24 * 10 -- the project's per-score bound plus one rounding per accumulated
reference and per penalty product, on values <= 10.  Every test prints what it measured (pytest -s); an MI355X run is in profiles/."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from oracle import vlp_oracle as O                                  # noqa: E402  (checker: the parameters of a small model)
from oracle.make_golden import decode_inputs                        # noqa: E402  (pure helper)
from tests import consensus_util as CU                              # noqa: E402
from tests import guard_util as GU                                  # noqa: E402
from tests import scst_df_util as U                                 # noqa: E402
from vlp_amd import _lib as K_                                      # noqa: E402
from vlp_amd import consensus as CS                                 # noqa: E402
from vlp_amd import sample_img2txt as SI                            # noqa: E402
from vlp_amd import scst as SC                                      # noqa: E402
from vlp_amd import synthetic as S                                  # noqa: E402
from vlp_amd.data import write_packed                               # noqa: E402
from vlp_amd.modeling import BertConfig, BertForSeq2SeqDecoder      # noqa: E402

DEV = torch.device("cuda:0")
bound = CU.bound


def run_kernel(ids, K, tab, want_pair=True, workspace=None):
    """(utility f32 [K*G], pick int32 [G], pair f32 [G, K, K] or None) on the host."""
    G = ids.shape[0] // K
    h = torch.from_numpy(np.array(ids)).to(DEV)
    keys, vals = tab.to(DEV)
    utility = torch.full((K * G,), float("nan"), device=DEV)
    pick = torch.full((G,), -7, dtype=torch.int32, device=DEV)
    pair = torch.full((G, K, K), float("nan"), device=DEV) if want_pair else None
    K_.cider_d_consensus(h, K, keys, vals, tab.n_docs, utility, pick, pair=pair, workspace=workspace)
    torch.cuda.synchronize()
    return utility.cpu(), pick.cpu(), (pair.cpu() if want_pair else None)


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---- (a) utilities and picks against the host -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CU.CASES, ids=CU.CASE_IDS)
@pytest.mark.parametrize("which", [0, 1], ids=["n200", "n3200000"])
def test_utility_and_pick_against_the_host(case, which):
    G, T, K = case
    ids, tab, want, want_pick = CU.host(case, which)
    # on the host alone, before the kernel's output is looked at
    assert (want.reshape(K, G).max(axis=0) > 0).all()
    assert (int(tab.vals.max()) > 1 << 16) == bool(which)
    sure = int(CU.decisive(want, K, 2 * bound(T, K)).sum())
    if which == 0 and T >= 21:
        assert 2 * sure >= G, (sure, G)
    assert K_.cider_d_consensus_workspace_bytes(G, K, T) > 0
    got, pick, _ = run_kernel(ids, K, tab)
    err = float(np.abs(got.double().numpy() - want).max())
    print("G%d T%d K%d %s: max |utility - host| %.3e, bound %.3e, max utility %.3f, decisive groups %d/%d"
          % (G, T, K, "n3200000" if which else "n200", err, bound(T, K), float(want.max()), sure, G))
    assert err <= bound(T, K), (err, bound(T, K))
    assert pick.dtype == torch.int32
    assert CU.check_pick(pick.numpy(), got.numpy(), want, K, T) == sure


# ---- (b) pair ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CU.CASES, ids=CU.CASE_IDS)
def test_pair_scores_and_null_pair(case):
    G, T, K = case
    ids, tab, _, _ = CU.host(case, 0)
    want = CU.pair_host(ids, K, tab)
    assert float(want.max()) > 0
    got, pick, pair = run_kernel(ids, K, tab)
    err = float(np.abs(pair.double().numpy() - want).max())
    print("G%d T%d K%d: max |pair - host| %.3e, bound %.3e" % (G, T, K, err, U.bound(T)))
    assert err <= U.bound(T), (err, U.bound(T))
    diag = pair[:, torch.arange(K), torch.arange(K)]
    assert torch.equal(diag.view(torch.int32), torch.zeros(G, K, dtype=torch.int32))      # +0, bit for bit
    got0, pick0, _ = run_kernel(ids, K, tab, want_pair=False)
    assert same_bits(got, got0) and torch.equal(pick, pick0)


# ---- (c) special rows -------------------------------------------------------------------------------------------------------------------
def test_identical_samples():
    T, K = 21, 16
    row = CU.samples(1, T, 2)[0]
    ids = np.tile(row, (K, 1))
    tab = U.table(T, 0)
    want, _ = CS.consensus_utility(ids, K, tab)
    assert want[0] > 0
    got, pick, pair = run_kernel(ids, K, tab)
    assert same_bits(got, got[:1].expand(K).contiguous()) and int(pick[0]) == 0
    assert abs(float(got[0]) - want[0]) <= bound(T, K)
    # beside an image of different samples: image 0 identical, image 1 not
    both = np.stack([ids, CU.samples(1, T, K)], axis=1).reshape(2 * K, T)
    got2, pick2, _ = run_kernel(both, K, tab)
    assert same_bits(got2[0::2].contiguous(), got) and int(pick2[0]) == 0
    assert len(set(got2[1::2].tolist())) > 1


@pytest.mark.parametrize("K", [2, 4])
def test_hard_values(K):
    T = 8
    ids, ids0 = CU.hard_rows(True), CU.hard_rows(False)
    tab = U.hard_table()
    G = len(ids) // K
    # what the rows were built for
    assert (ids == 65535).any() and (ids == 70000).any() and (ids == 32766).any() and (ids == 32767).any() and (ids == 65534).any()
    assert int(tab.keys[-1]) > 2 ** 63 > U.key_of((32766, 1001, 32767, 1009)) and U.key_of((32767,)) >= 2 ** 63
    assert not np.array_equal(ids, ids0)
    want, want_pick = CS.consensus_utility(ids, K, tab)
    assert np.array_equal(CS.consensus_utility(ids0, K, tab)[0], want)            # garbage behind the first 0 is no text
    runs = [i for i in range(len(ids)) if (ids[i] == 1009).all()]                 # every n-gram has df == n_docs: zero norm, undivided sum
    assert len(runs) == 2 and all(want[i] == 0 for i in runs) and float(want.max()) > 0
    got, pick, pair = run_kernel(ids, K, tab)
    err = float(np.abs(got.double().numpy() - want).max())
    print("hard rows K%d: max |utility - host| %.3e, bound %.3e, host %s" % (K, err, bound(T, K), [round(float(v), 5) for v in want]))
    assert err <= bound(T, K), (err, bound(T, K))
    assert all(float(got[i]) == 0.0 for i in runs)
    CU.check_pick(pick.numpy(), got.numpy(), want, K, T)
    assert float(np.abs(pair.double().numpy() - CU.pair_host(ids, K, tab)).max()) <= U.bound(T)
    got0, pick0, pair0 = run_kernel(ids0, K, tab)
    assert same_bits(got, got0) and torch.equal(pick, pick0) and same_bits(pair, pair0)
    # an empty table is legal: every df is 0
    empty = SC.DocFreq(tab.keys[:0], tab.vals[:0], tab.n_docs)
    want_e, _ = CS.consensus_utility(ids, K, empty)
    got_e, pick_e, _ = run_kernel(ids, K, empty)
    assert float(np.abs(want_e - want).max()) > 1e-2
    assert float(np.abs(got_e.double().numpy() - want_e).max()) <= bound(T, K)
    CU.check_pick(pick_e.numpy(), got_e.numpy(), want_e, K, T)


# ---- (d) contract -----------------------------------------------------------------------------------------------------------------------
def _guarded_table(tab):
    gk = GU.guarded_vec(len(tab), dtype=torch.int64, fill=U.key_of((1000,)), device=DEV)          # guards: a real key
    gk.vec.copy_(torch.from_numpy(tab.keys.view(np.int64)).to(DEV))
    gv = GU.guarded_vec(len(tab), dtype=torch.int32, fill=7, device=DEV)
    gv.vec.copy_(torch.from_numpy(tab.vals).to(DEV))
    return gk.seal(), gv.seal()


@pytest.mark.parametrize("case", [(5, 21, 5), (3, 64, 16)], ids=["G5_T21_K5", "G3_T64_K16"])
def test_strides_guards_and_repeats(case):
    G, T, K = case
    ids, tab, _, _ = CU.host(case, 1)
    plain_u, plain_p, plain_pair = run_kernel(ids, K, tab)
    # rows with a stride larger than T; the padding and the guards hold 1000, a real word
    gh = GU.guarded(K * G, T, ld=T + 5, dtype=torch.int64, fill=1000, device=DEV).set(torch.from_numpy(np.array(ids)).to(DEV))
    assert gh.view.stride() == (T + 5, 1)
    gk, gv = _guarded_table(tab)
    need = K_.cider_d_consensus_workspace_bytes(G, K, T)
    assert need > 0 and need % 16 == 0
    outs = []
    for _ in range(2):
        gu = GU.guarded_vec(K * G, dtype=torch.float32, fill="sentinel", device=DEV)
        gp = GU.guarded_vec(G, dtype=torch.int32, fill="sentinel", device=DEV)
        gq = GU.guarded_vec(G * K * K, dtype=torch.float32, fill="sentinel", device=DEV)
        ws = GU.guarded_vec(need, dtype=torch.uint8, fill="sentinel", device=DEV)
        K_.cider_d_consensus(gh.view, K, gk.vec, gv.vec, tab.n_docs, gu.vec, gp.vec, pair=gq.vec, workspace=ws.vec)
        torch.cuda.synchronize()
        for g, name, written in ((gu, "utility", "logical"), (gp, "pick", "logical"), (gq, "pair", "logical"), (ws, "workspace", "logical"),
                                 (gh, "hyp", None), (gk, "df_keys", None), (gv, "df_vals", None)):
            GU.assert_untouched(g, written=written, name=name)
        for g, name in ((gu, "utility"), (gp, "pick"), (gq, "pair")):
            GU.assert_written(g, name=name)
        outs.append((gu.vec.clone().cpu(), gp.vec.clone().cpu(), gq.vec.clone().cpu().view(G, K, K)))
    assert same_bits(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]) and same_bits(outs[0][2], outs[1][2])
    assert same_bits(outs[0][0], plain_u) and torch.equal(outs[0][1], plain_p) and same_bits(outs[0][2], plain_pair)


def test_graph_capture_and_replay_equal_the_eager_run():
    case = (16, 21, 16)
    G, T, K = case
    ids, tab, _, _ = CU.host(case, 0)
    eager_u, eager_p, eager_pair = run_kernel(ids, K, tab)
    h = torch.from_numpy(np.array(ids)).to(DEV)
    keys, vals = tab.to(DEV)
    utility, pick, pair = torch.zeros(K * G, device=DEV), torch.zeros(G, dtype=torch.int32, device=DEV), torch.zeros(G, K, K, device=DEV)
    ws = torch.empty(K_.cider_d_consensus_workspace_bytes(G, K, T), dtype=torch.uint8, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                       # warm-up: code objects loaded
        K_.cider_d_consensus(h, K, keys, vals, tab.n_docs, utility, pick, pair=pair, workspace=ws)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):                          # any synchronising call fails the capture
        K_.cider_d_consensus(h, K, keys, vals, tab.n_docs, utility, pick, pair=pair, workspace=ws)
    utility.fill_(float("nan"))
    pick.fill_(-7)
    pair.fill_(float("nan"))
    ws.fill_(0x5A)
    graph.replay()
    torch.cuda.synchronize()
    assert same_bits(utility.cpu(), eager_u) and torch.equal(pick.cpu(), eager_p) and same_bits(pair.cpu(), eager_pair)


REFUSALS = ["K1", "K17", "T0", "T65", "G0", "G1025", "workspace_short", "workspace_misaligned", "n_docs_0", "n_docs_above_2p24", "keys_null", "sigma_0",
            "hyp_ld_short"]


@pytest.mark.parametrize("what", REFUSALS)
def test_refusals_by_return_code(what):
    G, K, T = {"K1": (2, 1, 4), "K17": (2, 17, 4), "T0": (2, 2, 0), "T65": (2, 2, 65), "G0": (0, 2, 4), "G1025": (1025, 2, 4)}.get(what, (2, 2, 4))
    hyp = torch.full((max(K * G, 1), max(T, 1)), 1000, dtype=torch.int64, device=DEV)
    tab = U.table(4, 0)
    gk, gv = _guarded_table(tab)
    gu = GU.guarded_vec(max(K * G, 1), dtype=torch.float32, fill="sentinel", device=DEV)
    gp = GU.guarded_vec(max(G, 1), dtype=torch.int32, fill="sentinel", device=DEV)
    gq = GU.guarded_vec(max(G * K * K, 1), dtype=torch.float32, fill="sentinel", device=DEV)
    need = K_.cider_d_consensus_workspace_bytes(G, K, T)
    if what in ("K1", "K17", "T0", "T65", "G0", "G1025"):
        assert need == 0
    else:
        assert need > 0                                                  # the shape itself is fine: the same call without the fault runs
        K_.cider_d_consensus(hyp, K, gk.vec, gv.vec, tab.n_docs, gu.vec, gp.vec, pair=gq.vec, workspace=torch.empty(need, dtype=torch.uint8, device=DEV))
        torch.cuda.synchronize()
        GU.assert_written(gu, name="utility")
        for g in (gu, gp, gq):
            g.fill_all("sentinel")
            g.seal()
    ws = GU.guarded_vec(max(need, 4096) + 16, dtype=torch.uint8, fill="sentinel", device=DEV)
    wp, wbytes = ws.vec.data_ptr(), max(need, 4096)
    if what == "workspace_short":
        wbytes = need - 1
    elif what == "workspace_misaligned":
        wp += 8
    assert ws.vec.data_ptr() % 16 == 0
    kp, vp, n, n_docs, sigma, ld = gk.vec.data_ptr(), gv.vec.data_ptr(), len(tab), tab.n_docs, 6.0, hyp.stride(0)
    if what == "n_docs_0":
        n_docs = 0
    elif what == "n_docs_above_2p24":
        n_docs = 2 ** 24 + 1
    elif what == "keys_null":
        kp = None
    elif what == "sigma_0":
        sigma = 0.0
    elif what == "hyp_ld_short":
        ld = T - 1
    a = K_.CiderDConsensusArgs(K_.ptr(hyp), ld, G, K, T, sigma, C.c_void_p(kp), C.c_void_p(vp), n, n_docs, K_.ptr(gu.vec), K_.ptr(gp.vec), K_.ptr(gq.vec),
                               C.c_void_p(wp), wbytes)
    rc = K_.load().vlp_cider_d_consensus(C.byref(a), K_.stream_ptr())
    assert rc == -1, rc                                                 # VLP_ERR_BAD_ARG
    assert "vlp_cider_d_consensus" in K_.load().vlp_last_error_string().decode()
    torch.cuda.synchronize()
    for g, name in ((gu, "utility"), (gp, "pick"), (gq, "pair"), (ws, "workspace"), (gk, "df_keys"), (gv, "df_vals")):
        GU.assert_untouched(g, written=None, name=name)                 # nothing was launched


# ---- (e) end to end ---------------------------------------------------------------------------------------------------------------------
MK = dict(vocab_size=1024, layers=2, tasks="img2txt", seed=41, std=0.05)
B, T_DEC = 3, 6


def _table(max_len_b, path=None, seed=3):
    """A table of 40 images x 3 captions over the words 300..339 for captions of max_len_b tokens; most sampled n-grams miss it (df 0)."""
    rng = np.random.RandomState(seed)
    ex = [(i, [int(t) for t in rng.randint(300, 340, size=rng.randint(2, max_len_b + 1))]) for i in range(40) for _ in range(3)]
    tab = SC.DocFreq.from_examples(ex, max_len_b, S.SEP_ID)
    if path:
        tab.save(path)
    return tab


def test_model_samples_to_consensus_pick():
    Ks = 8
    p = O.init_params(vocab_size=MK["vocab_size"], layers=MK["layers"], tasks=MK["tasks"], seed=MK["seed"], std=MK["std"])
    cfg = BertConfig(MK["vocab_size"], num_hidden_layers=MK["layers"], type_vocab_size=6, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1)
    m = BertForSeq2SeqDecoder(cfg, mask_word_id=S.MASK_ID, eos_id=S.SEP_ID, enable_butd=True, len_vis_input=100, search_beam_size=1)
    sd = dict(p)
    sd["cls.predictions.decoder.weight"] = p["bert.embeddings.word_embeddings.weight"]
    m.load_state_dict(sd, strict=True)
    m = m.half().to(DEV).eval()
    dv = [t.to(DEV) for t in decode_inputs(B, T_DEC, 99)]
    dv = [dv[0].half(), dv[1].half()] + dv[2:]
    tab = _table(T_DEC)
    with torch.no_grad():
        ids, _ = m(*dv, sample_mode="sample", n_samples=Ks, top_k=2)    # two words per step: the samples of an image overlap
    assert tuple(ids.shape) == (Ks * B, T_DEC)
    clean = SC.clean_captions(ids, S.SEP_ID, S.PAD_ID)
    pick, utility = CS.consensus_select_device(clean, Ks, tab)
    assert pick.is_cuda and utility.is_cuda and pick.dtype == torch.int32 and tuple(pick.shape) == (B,) and tuple(utility.shape) == (Ks * B,)
    torch.cuda.synchronize()
    want, want_pick = CS.consensus_utility(clean, Ks, tab)
    assert (want.reshape(Ks, B).max(axis=0) > 0).all() and len(set(map(tuple, clean.cpu().tolist()))) > B
    err = float(np.abs(utility.double().cpu().numpy() - want).max())
    print("model samples: max |utility - host| %.3e, bound %.3e, host pick %s, device pick %s" % (err, bound(T_DEC, Ks), list(want_pick), pick.tolist()))
    assert err <= bound(T_DEC, Ks)
    CU.check_pick(pick.cpu().numpy(), utility.cpu().numpy(), want, Ks, T_DEC)
    # the caller's buffers
    out = torch.zeros(Ks * B, device=DEV)
    pair = torch.zeros(B, Ks, Ks, device=DEV)
    pick2, u2 = CS.consensus_select_device(clean, Ks, tab, utility_out=out, pair_out=pair)
    torch.cuda.synchronize()
    assert u2 is out and same_bits(out.cpu(), utility.cpu()) and torch.equal(pick2, pick) and float(pair.max()) > 0


NV, TC, VOCAB = 100, 10, 1024
LIST = [("test", 391895), ("val", 522418), ("test", 184613), ("test", 318219), ("val", 554625), ("test", 574769), ("test", 60623)]


def fname(i):
    return "COCO_val2014_%012d.jpg" % i


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    """A packed store of 5 images, a 2-layer checkpoint, a vocabulary, a Karpathy-style image list and a document-frequency table."""
    root = str(tmp_path_factory.mktemp("consensus_cli"))
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
    df = os.path.join(root, "df.npz")
    _table(TC, df)
    return dict(root=root, store=store, bert=bert, ckpt=ckpt, src=src, test_ids=test_ids, df=df)


def argv(su, out, *extra):
    return ["--bert_model", su["bert"], "--model_recover_path", su["ckpt"], "--packed_features", su["store"], "--src_file", su["src"], "--split", "test",
            "--dataset", "coco", "--output_file", out, "--batch_size", "2", "--max_tgt_length", str(TC), "--new_segment_ids", "--fp16",
            "--enable_butd"] + list(extra)


FLAGS = ("--top_k", "3", "--num_samples", "4", "--seed", "11")


def _read(path):
    with open(path) as f:
        return f.read()


def test_cli_select_consensus(setup, monkeypatch):
    su = setup
    files, calls = [], []
    real = CS.consensus_select_device

    def spy(ids, n_samples, df, **kw):
        pick, utility = real(ids, n_samples, df, **kw)
        calls.append((ids.clone(), n_samples, df, pick, utility))
        return pick, utility
    monkeypatch.setattr(CS, "consensus_select_device", spy)
    for name in ("a", "b"):
        out, smp = os.path.join(su["root"], "sel_%s.json" % name), os.path.join(su["root"], "all_%s.json" % name)
        res = SI.main(argv(su, out, *FLAGS, "--select", "consensus", "--consensus_df", su["df"], "--samples_file", smp))
        files.append((_read(out), _read(smp)))
        assert res == {su["ckpt"]: json.loads(files[-1][0])}
    assert files[0] == files[1]                                         # the same --seed writes the same files
    sel, smp = json.loads(files[0][0]), json.loads(files[0][1])
    assert [r["image_id"] for r in sel] == su["test_ids"]               # one record per image, input order (5 images in batches of 2)
    assert [(r["image_id"], r["sample"]) for r in smp] == [(i, k) for i in su["test_ids"] for k in range(4)]
    assert all(set(r) == {"image_id", "caption", "sample", "logprob", "utility"} for r in sel + smp)
    assert any(r["utility"] > 0 for r in smp)
    for r in sel:
        mine = [s for s in smp if s["image_id"] == r["image_id"]]
        assert r == mine[r["sample"]]                                   # (sample, caption, logprob, utility) of that sample's record
        best = max(s["utility"] for s in mine)
        assert r["sample"] == [s["utility"] for s in mine].index(best)  # the image's first maximum
    # what the tool handed the selection: cleaned ids, three batches of 2 x 4 rows per run, one table object (uploaded once per run), and
    # utilities that are the host specification's
    assert len(calls) == 6 and all(tuple(c[0].shape) == (8, TC) and c[1] == 4 for c in calls)
    assert all(c[2] is calls[0][2] for c in calls[:3]) and all(c[2] is calls[3][2] for c in calls[3:])
    written = [s["utility"] for s in smp]
    for n, (ids, _, df, pick, utility) in enumerate(calls[:3]):
        assert torch.equal(ids, SC.clean_captions(ids, S.SEP_ID, S.PAD_ID))
        want, _ = CS.consensus_utility(ids, 4, df)
        assert float(np.abs(utility.double().cpu().numpy() - want).max()) <= bound(TC, 4)
        CU.check_pick(pick.cpu().numpy(), utility.cpu().numpy(), want, 4, TC)
        u = utility.view(4, 2).cpu()
        for b in range(2 if n < 2 else 1):                                # the last batch holds one image and one padding row
            assert written[(2 * n + b) * 4:(2 * n + b) * 4 + 4] == u[:, b].tolist()
            assert sel[2 * n + b]["sample"] == int(pick[b])


def test_cli_select_logprob_and_none(setup):
    su = setup
    out_n, out_p = os.path.join(su["root"], "none.json"), os.path.join(su["root"], "plain.json")
    SI.main(argv(su, out_n, *FLAGS, "--select", "none"))
    SI.main(argv(su, out_p, *FLAGS))
    assert _read(out_n) == _read(out_p)                                 # --select none: the same bytes as a run without the flag
    smp = json.loads(_read(out_p))
    assert len(smp) == 5 * 4 and all(set(r) == {"image_id", "sample", "caption", "logprob"} for r in smp)
    out_l = os.path.join(su["root"], "logprob.json")
    SI.main(argv(su, out_l, *FLAGS, "--select", "logprob"))
    sel = json.loads(_read(out_l))
    assert [r["image_id"] for r in sel] == su["test_ids"]
    for r in sel:
        mine = [s for s in smp if s["image_id"] == r["image_id"]]
        lps = [s["logprob"] for s in mine]
        assert r["utility"] is None and r["sample"] == lps.index(max(lps))
        assert {k: r[k] for k in ("image_id", "sample", "caption", "logprob")} == mine[r["sample"]]
    assert len({r["sample"] for r in sel}) > 1 or len({s["caption"] for s in smp}) > 5
    # a table built for another caption length is refused before anything is decoded
    never = os.path.join(su["root"], "never.json")
    other = os.path.join(su["root"], "df_other.npz")
    _table(TC + 1, other)
    with pytest.raises(ValueError, match="was built for --max_len_b %d" % (TC + 1)):
        SI.main(argv(su, never, *FLAGS, "--select", "consensus", "--consensus_df", other))
    assert not os.path.exists(never)
