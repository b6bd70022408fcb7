"""CPU: the CIDEr-D document-frequency table (vlp_amd.scst.DocFreq), the host scorer's table mode CiderD(df=<DocFreq>) and the --scst_df
plumbing.  The device kernels' twin is tests/test_82_scst_df_gpu.py.

(1) DocFreq.from_examples against a brute-force Counter over the strings array_to_str makes of the loader's reference rows; key order,
    uniqueness, n_docs, save / load; every refusal of a malformed table;
(2) the key of an n-gram;
(3) CiderD(df=table) against a restatement that shares no code with it (tests/scst_df_util.restated_scores, fp64) on the shapes of the GPU
    test, and tied to the pinned df='corpus' scorer: a table counted over exactly the call's reference sets, one hypothesis per set, gives
    the same scores to 1e-12;
(4) --scst_df: every refusal, what scst_step hands the reward functions, and `python -m vlp_amd.cider_df` on a tiny token file."""
import json
import os
import subprocess
import sys
from collections import Counter

import numpy as np
import pytest
import torch

from tests import scst_df_util as U
from vlp_amd import scst as SC

SEP = U.SEP
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- (1) the table --------------------------------------------------------------------------------------------------------------------
def _examples(seed=0, images=50, max_len_b=6):
    """About 50 images x 1..6 captions, shuffled; caption lengths 1 .. max_len_b + 3: shorter than max_len_b (a trailing 0), equal (no
    trailing 0) and longer (truncated)."""
    rng = np.random.RandomState(seed)
    ex = []
    for i in range(images):
        for _ in range(rng.randint(1, 7)):
            ex.append(("img%d" % i, [int(t) for t in rng.randint(1000, 1012, size=rng.randint(1, max_len_b + 4))]))
    return [ex[i] for i in rng.permutation(len(ex))]


def _reference_row(tokens, max_len_b):
    """The row BatchPrefetcher(caption_refs=R) builds: the first max_len_b tokens, [SEP], then 0 up to max_len_b + 1 columns."""
    row = [int(t) for t in tokens[:max_len_b]] + [SEP]
    return row + [0] * (max_len_b + 1 - len(row))


def _brute_force(examples, max_len_b):
    docs = {}
    for img, tokens in examples:
        words = SC.array_to_str(_reference_row(tokens, max_len_b)).split()
        docs.setdefault(img, set()).update(SC._ngrams(words, 4).keys())
    return Counter(g for grams in docs.values() for g in grams), len(docs)


@pytest.mark.parametrize("chunk", [1 << 16, 7])
def test_table_build_against_brute_force(chunk, tmp_path):
    max_len_b = 6
    ex = _examples()
    lens = [len(t) for _, t in ex]
    assert min(lens) < max_len_b and max_len_b in lens and max(lens) > max_len_b
    want, n_docs = _brute_force(ex, max_len_b)
    tab = SC.DocFreq.from_examples(ex, max_len_b, SEP, chunk=chunk)
    assert tab.n_docs == n_docs == 50 and len(tab) == len(want) and (tab.max_len_b, tab.sep_id) == (max_len_b, SEP)
    assert tab.keys.dtype == np.uint64 and tab.vals.dtype == np.int32
    assert (tab.keys[1:] > tab.keys[:-1]).all()                                          # strictly ascending: sorted and unique
    assert int(tab.vals.min()) >= 1 and int(tab.vals.max()) <= n_docs
    by_key = {SC.pack_ngram([int(w) for w in g]): v for g, v in want.items()}
    assert len(by_key) == len(want)
    assert dict(zip((int(k) for k in tab.keys), (int(v) for v in tab.vals))) == by_key
    for g, v in list(want.items())[::17]:
        assert tab.get(g, 0.0) == v and tab.get(tuple(int(w) for w in g), 0.0) == v
    assert tab.get(("1000", "999"), 0.0) == 0.0 and tab.get(("70000",), -1) == -1 and tab.get(("x",), -2) == -2
    # [SEP] and the trailing 0 are tokens of n-grams; the string of a caption of max_len_b tokens or more has no 0
    assert tab.get((str(SEP), "0"), 0) > 0 and tab.get(("0",), 0) == len({i for i, t in ex if len(t) < max_len_b})
    # an image's captions count once
    twice = SC.DocFreq.from_examples(ex + ex, max_len_b, SEP, chunk=chunk)
    assert np.array_equal(twice.keys, tab.keys) and np.array_equal(twice.vals, tab.vals) and twice.n_docs == n_docs
    # save / load
    path = os.path.join(tmp_path, "df.npz")
    tab.save(path)
    with np.load(path) as z:
        assert sorted(z.files) == ["keys", "max_len_b", "n_docs", "sep_id", "vals"]
    back = SC.DocFreq.load(path)
    assert np.array_equal(back.keys, tab.keys) and np.array_equal(back.vals, tab.vals)
    assert (back.n_docs, back.max_len_b, back.sep_id) == (tab.n_docs, max_len_b, SEP)


def test_malformed_tables_are_refused(tmp_path):
    k = np.array([5, 9, 1 << 63], dtype=np.uint64)
    v = np.array([1, 2, 3], dtype=np.int32)
    SC.DocFreq(k, v, 3)
    SC.DocFreq(k[:0], v[:0], 1)                                                           # an empty table is a table
    bad = {"not sorted": (k[[1, 0, 2]], v, 3), "duplicate": (k[[0, 1, 1]], v, 3), "below 1": (k, np.array([1, 0, 3], dtype=np.int32), 3),
           "above n_docs": (k, v, 2), r"2\*\*24": (k, v, 2 ** 24 + 1), "outside 1": (k, v, 0), "key 0": (np.array([0, 5, 9], dtype=np.uint64), v, 3),
           "uint64": (k.astype(np.int64), v, 3)}
    for msg, (kk, vv, n) in bad.items():
        with pytest.raises(ValueError, match=msg):
            SC.DocFreq(kk, vv, n)
    SC.DocFreq(k, v, 2 ** 24)
    # the same through load
    for i, (msg, (kk, vv, n)) in enumerate(bad.items()):
        path = os.path.join(tmp_path, "bad%d.npz" % i)
        np.savez(path, keys=kk, vals=vv, n_docs=np.int64(n), max_len_b=np.int64(20), sep_id=np.int64(SEP))
        with pytest.raises(ValueError, match=msg):
            SC.DocFreq.load(path)
    path = os.path.join(tmp_path, "other.npz")
    np.savez(path, keys=k, vals=v, n_docs=np.int64(3))
    with pytest.raises(ValueError, match="not a table"):
        SC.DocFreq.load(path)
    with pytest.raises(ValueError, match="outside 0..65534"):
        SC.DocFreq.from_examples([(0, [5, 65535])], 4, SEP)
    with pytest.raises(ValueError, match="no examples"):
        SC.DocFreq.from_examples([], 4, SEP)


# ---- (2) keys -------------------------------------------------------------------------------------------------------------------------
def test_key_packing():
    P = SC.pack_ngram
    assert P([0]) == 1 << 48 and P([65534]) == 65535 << 48 and P([0, 0, 0, 0]) == (1 << 48) | (1 << 32) | (1 << 16) | 1
    assert P([65534] * 4) == 2 ** 64 - 1
    keys = set()
    for k in range(1, 5):
        for pos in range(k):
            for t in (0, 65534):
                g = [7] * k
                g[pos] = t
                assert (P(g) >> (48 - 16 * pos)) & 0xffff == t + 1
                keys.add(P(g))
    assert len(keys) == 2 * (1 + 2 + 3 + 4)
    a = 1234
    assert len({P([a]), P([a, 0]), P([0, a]), P([0]), P([0, 0])}) == 5
    assert all(P(g) != 0 for g in ([0], [0, 0], [0, 0, 0, 0]))
    for bad in ([], [1] * 5, [-1], [65535], [3, 70000]):
        with pytest.raises(ValueError):
            P(bad)
    # a key with the top bit set sorts last: ids 32766 / 32767 straddle 2^63, numpy's uint64 order is the unsigned one
    assert P([32766, 65534, 65534, 65534]) < 2 ** 63 <= P([32767])
    ks = np.array(sorted([P([32767]), P([5]), P([65534, 1]), P([32766, 9])]), dtype=np.uint64)
    assert int(ks[-1]) == P([65534, 1]) and int(ks[0]) == P([5]) and (ks[1:] > ks[:-1]).all()
    tab = SC.DocFreq(ks, np.arange(1, 5, dtype=np.int32), 4)
    assert [tab.get(g, 0) for g in ((5,), (32766, 9), (32767,), (65534, 1), (65534,), (32767, 0))] == [1, 2, 3, 4, 0, 0]


# ---- (3) the scorer -------------------------------------------------------------------------------------------------------------------
CORPUS_SEED = {(1, 1, 4, 2): 2}            # the others: 0 (tests/scst_df_util.py says how the seeds were chosen)


@pytest.mark.parametrize("shape", U.SHAPES, ids=["G%d_R%d_T%d_m%d" % s for s in U.SHAPES])
@pytest.mark.parametrize("which", [0, 1], ids=["n200", "n3200000"])
def test_table_scorer_against_restatement(shape, which):
    G, R, T, mult = shape
    hyp, ref, count = U.make_corpus(G, R, T, mult, CORPUS_SEED.get(shape, 0))
    tab = U.table(T, which)
    assert tab.n_docs == (200 * U.SCALE if which else 200) and (int(tab.vals.max()) > 1 << 16) == bool(which)
    got = U.host_scores(hyp, ref, count, mult, df=tab)
    want, miss = U.restated_scores(hyp, ref, count, mult, tab)
    assert float(np.abs(got - want).max()) < 1e-12
    assert (got != 0).all()                       # with a table G = 1 is no longer the all-zero case of df='corpus'
    assert (0.05 <= miss <= 0.5) if T >= 3 else miss == 0, miss
    e32 = float(np.abs(U.restated_scores(hyp, ref, count, mult, tab, np.float32)[0] - got).max())
    assert e32 <= U.bound(T) / 4, (e32, U.bound(T))
    # the batch mode is another reward (a one-word string has one weight per vector, which the norms cancel)
    assert T < 3 or float(np.abs(got - U.host_scores(hyp, ref, count, mult)).max()) > 1e-3


@pytest.mark.parametrize("shape", [(8, 1, 5), (5, 3, 21), (16, 2, 9)])
def test_table_of_the_calls_own_sets_is_the_corpus_mode(shape):
    G, R, T = shape
    hyp, ref, count = U.make_corpus(G, R, T, 1, 4)
    pinned = U.host_scores(hyp, ref, count, 1)
    assert np.count_nonzero(pinned) >= G // 2
    same = U.host_scores(hyp, ref, count, 1, df=U.table_of_sets(ref, count))
    assert float(np.abs(same - pinned).max()) < 1e-12


def test_corpus_mode_and_other_strings():
    assert SC.CiderD().df == "corpus" and SC.CiderD(df="corpus").df == "corpus"
    for bad in ("coco-train-idxs", "", None, 3):
        with pytest.raises(NotImplementedError):
            SC.CiderD(df=bad)
    tab = U.table(5, 0)
    assert SC.CiderD(df=tab).df is tab


def test_reward_functions_pass_the_table_through():
    from vlp_amd.input_prep import CaptionRefs
    B, R, T = 6, 3, 9
    hyp, ref, count = U.make_corpus(B, R, T, 2, 1)
    tab = U.table(T, 0)
    want = U.host_scores(hyp, ref, count, 2, df=tab)
    refs = CaptionRefs(torch.from_numpy(ref), torch.from_numpy(count))
    r, s = SC.self_critical_reward_refs(torch.from_numpy(hyp[B:]), refs, torch.from_numpy(hyp[:B]), df=tab)
    assert np.array_equal(s, want) and np.array_equal(r, np.repeat((want[:B] - want[B:])[:, None], T, 1))
    one = np.ones(B, dtype=np.int32)
    r1, s1 = SC.self_critical_reward(hyp[B:], ref[:, 0], hyp[:B], B, df=tab)
    assert np.array_equal(s1, U.host_scores(hyp, ref, one, 2, df=tab))
    r2, s2 = SC.self_critical_reward_refs(hyp[B:], torch.from_numpy(ref[:, 0]), hyp[:B], df=tab)
    assert np.array_equal(s2, s1) and np.array_equal(r2, r1)
    # None is today's path
    r0, s0 = SC.self_critical_reward_refs(hyp[B:], refs, hyp[:B], df=None)
    assert np.array_equal(s0, U.host_scores(hyp, ref, count, 2)) and not np.array_equal(s0, s)
    with pytest.raises(TypeError):
        SC.self_critical_reward(hyp[B:], ref[:, 0], hyp[:B], B, df="corpus")


# ---- (4) the command line -------------------------------------------------------------------------------------------------------------
def _args(extra):
    from vlp_amd import run_img2txt_dist as R
    return R.derive_args(R.build_parser().parse_args(["--enable_butd", "--fp16"] + extra))


def test_scst_df_refusals(tmp_path):
    from vlp_amd import run_img2txt_dist as R
    scst = ["--scst", "--max_pred", "0", "--mask_prob", "0"]
    assert _args([]).scst_df == "batch" and _args(scst).scst_df == "batch"
    assert R.scst_doc_freq(_args(scst)) is None
    ex = _examples(images=6, max_len_b=4)
    tok = os.path.join(tmp_path, "tokens.json")
    json.dump([[i, t] for i, t in ex], open(tok, "w"))
    saved = os.path.join(tmp_path, "df.npz")
    SC.DocFreq.from_examples(ex, 20, SEP).save(saved)
    with pytest.raises(ValueError, match="needs --scst"):
        _args(["--scst_df", "train", "--packed_features", "x", "--token_file", tok])
    with pytest.raises(ValueError, match="needs --scst"):
        _args(["--scst_df", saved])
    with pytest.raises(ValueError, match="needs --packed_features"):
        _args(scst + ["--scst_df", "train"])
    with pytest.raises(ValueError, match="needs --packed_features"):
        _args(scst + ["--scst_df", "train", "--packed_features", "x"])                   # no --token_file
    with pytest.raises(ValueError, match="there is no file"):
        _args(scst + ["--scst_df", os.path.join(tmp_path, "missing.npz")])
    # a table of another caption format
    for other, kw in (("len.npz", dict(max_len_b=12, sep_id=SEP)), ("sep.npz", dict(max_len_b=20, sep_id=3))):
        path = os.path.join(tmp_path, other)
        SC.DocFreq.from_examples(ex, **kw).save(path)
        with pytest.raises(ValueError, match="was built for"):
            R.scst_doc_freq(_args(scst + ["--scst_df", path]))
    # a VQA token file has no captions
    vqa = os.path.join(tmp_path, "vqa.json")
    json.dump([[i, t, [1], 7] for i, t in ex], open(vqa, "w"))
    with pytest.raises(ValueError, match="caption --token_file"):
        R.scst_doc_freq(_args(scst + ["--scst_df", "train", "--packed_features", "x", "--token_file", vqa]))
    # what is accepted: with either reward and either reference mode
    a = _args(scst + ["--scst_df", saved, "--scst_reward", "device", "--scst_refs", "image", "--packed_features", "x"])
    loaded = R.scst_doc_freq(a)
    built = R.scst_doc_freq(_args(scst + ["--scst_df", "train", "--packed_features", "x", "--token_file", tok]))
    assert np.array_equal(loaded.keys, built.keys) and np.array_equal(loaded.vals, built.vals) and loaded.n_docs == built.n_docs == 6


def test_scst_step_hands_the_table_to_the_reward(monkeypatch):
    from tests.test_scst_reward_cpu import _Model, _Opt, _spies, _stub_batch
    from vlp_amd import run_img2txt_dist as R
    from vlp_amd.input_prep import CaptionRefs
    B, Nv, T = 3, 4, 6
    refs = CaptionRefs(torch.zeros(B, 5, T, dtype=torch.long), torch.ones(B, dtype=torch.int32))
    tab = U.table(5, 0)
    for reward_on, with_refs, who in (("host", False, "host"), ("host", True, "refs"), ("device", False, "device"), ("device", True, "device")):
        calls = _spies(monkeypatch, B, T)
        R.scst_step(_Model(B, T), _Opt(), _stub_batch(B, Nv, T, refs if with_refs else None), 1e-5, Nv, lambda logp, seq, reward: logp.sum(),
                    reward_on=reward_on, df=tab)
        assert [c[0] for c in calls] == [who] and calls[0][2] == {"df": tab}


def test_cider_df_command_line(tmp_path):
    ex = _examples(seed=3, images=5, max_len_b=4)
    tok, out = os.path.join(tmp_path, "tokens.json"), os.path.join(tmp_path, "df.npz")
    json.dump([[i, t] for i, t in ex], open(tok, "w"))
    r = subprocess.run([sys.executable, "-m", "vlp_amd.cider_df", "--token_file", tok, "--max_len_b", "4", "--out", out], cwd=ROOT, capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stderr
    got, want = SC.DocFreq.load(out), SC.DocFreq.from_examples(ex, 4, SEP)
    assert np.array_equal(got.keys, want.keys) and np.array_equal(got.vals, want.vals)
    assert (got.n_docs, got.max_len_b, got.sep_id) == (5, 4, SEP) and "5 images" in r.stdout
    from vlp_amd import cider_df
    out2 = os.path.join(tmp_path, "df2.npz")
    assert cider_df.main(["--token_file", tok, "--max_len_b", "4", "--sep_id", "3", "--out", out2]) == 0
    assert SC.DocFreq.load(out2).sep_id == 3
    vqa = os.path.join(tmp_path, "vqa.json")
    json.dump([[i, t, [1], 7] for i, t in ex], open(vqa, "w"))
    with pytest.raises(SystemExit):
        cider_df.main(["--token_file", vqa, "--max_len_b", "4", "--out", out2])
