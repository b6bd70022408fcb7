"""CPU: the n-best list of a beam search -- the host specification vlp_amd.nbest.beam_nbest_host, the argument checks of vlp_beam_nbest (they
run before anything touches a device) and the command line of python -m vlp_amd.decode_img2txt --n_best."""
import ctypes
import os

import numpy as np
import pytest

from oracle.make_golden import BEAM_CASES                  # (pure data)
from vlp_amd import synthetic as S
from vlp_amd.modeling import BertForSeq2SeqDecoder
from vlp_amd.nbest import beam_nbest_host, by_image

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


class Dec(object):
    def __init__(self, eos_id, length_penalty):
        self.eos_id, self.length_penalty = eos_id, length_penalty


def random_frames(rng, F, B, K, eos=3, ties=False):
    sc = rng.randn(F, B, K).astype(np.float32)
    if ties:
        sc = np.round(sc)
    ww, pp = rng.randint(0, 6, size=(F, B, K)), rng.randint(0, K, size=(F, B, K))
    return sc, ww.astype(np.int64), pp.astype(np.int64)


def test_rank_0_is_the_hypothesis_of_backtrack_batch():
    rng = np.random.RandomState(0)
    for trial in range(200):
        F, B, K = rng.randint(1, 8), rng.randint(1, 6), rng.randint(2, 5)
        sc, ww, pp = random_frames(rng, F, B, K, ties=trial % 5 == 0)
        if trial % 7 == 0:
            ww[rng.randint(0, F)] = 3                  # a frame whose words are all eos ends the search there
        if trial % 11 == 0:
            sc[:] = -np.inf                            # nothing finite: the reference returns [0]
        elif trial % 3 == 0:
            sc[rng.rand(F, B, K) < 0.3] = -np.inf
        lp = (0.3, 0.0, -0.4)[trial % 3]
        want = BertForSeq2SeqDecoder._backtrack_batch(Dec(3, lp), sc, ww, pp, F + 2)
        seq, score, value, length, ok = beam_nbest_host(sc, ww, pp, 1, 3, lp, F + 2)
        assert seq.dtype == np.int64 and score.dtype == np.float32 and value.dtype == np.float64 and length.dtype == np.int32 and ok.dtype == np.uint8
        assert seq.shape == (B, F + 2) and np.array_equal(seq, want), (trial, seq, want)
        # and the list of every size starts with it
        n = int(rng.randint(1, K + 1))
        seq_n = beam_nbest_host(sc, ww, pp, n, 3, lp, F + 2)[0]
        assert seq_n.shape == (n * B, F + 2) and np.array_equal(seq_n[:B], want)


@pytest.mark.parametrize("name", list(BEAM_CASES.keys()))
def test_rank_0_reproduces_the_reference_fixture(name):
    mk, B, T, seed, dk = BEAM_CASES[name]
    g = dict(np.load(os.path.join(GOLDEN_DIR, name + ".npz")))
    Kb, L = dk["search_beam_size"], g["pred_seq"].shape[1]
    tot, wids, ptrs = [np.ascontiguousarray(g[k][:, :T].transpose(1, 0, 2)) for k in ("scores", "wids", "ptrs")]      # [B, L, K] traces -> T frames
    for n in (1, Kb):
        seq, score, value, length, ok = beam_nbest_host(tot, wids, ptrs, n, S.SEP_ID, dk["length_penalty"], L)
        assert np.array_equal(seq[:B], g["pred_seq"])
        assert (ok[:B] == 1).all() and np.array_equal(length[:B], (g["pred_seq"] != 0).sum(axis=1))
        assert np.array_equal(value, score.astype(np.float64) + dk["length_penalty"] * length)


def test_ranks_are_ordered_and_ok_marks_the_finished_hypotheses():
    rng = np.random.RandomState(1)
    seen_not_ok = seen_ok_beyond_0 = 0
    for trial in range(100):
        F, B, K = rng.randint(2, 9), rng.randint(1, 5), rng.randint(2, 6)
        sc, ww, pp = random_frames(rng, F, B, K, ties=trial % 2 == 0)
        if trial % 4 == 1:
            sc[rng.rand(F, B, K) < 0.3] = -np.inf
        N = K
        seq, score, value, length, ok = beam_nbest_host(sc, ww, pp, N, 3, 0.25, F)
        v, o, s, ln = by_image(value, N), by_image(ok, N), by_image(seq, N), by_image(length, N)
        assert v.shape == (B, N) and s.shape == (B, N, F)
        assert (v[:, 1:] <= v[:, :-1]).all(), (trial, v)                    # value never increases with the rank
        for b in range(B):
            for n in range(N):
                words = s[b, n, :ln[b, n]].tolist()
                assert bool(o[b, n]) == (ln[b, n] > 0 and 3 not in words[:-1])
                assert (s[b, n, ln[b, n]:] == 0).all()
        seen_not_ok += int((o == 0).sum())
        seen_ok_beyond_0 += int(o[:, 1:].sum())
    assert seen_not_ok > 20 and seen_ok_beyond_0 > 20                       # both kinds of row were exercised


def test_the_frames_of_a_real_search_give_distinct_ok_rows():
    """Random back pointers can rebuild one word sequence twice; the frames of a search cannot.  Frames built the way the search builds them
    (K distinct continuations per step, a hypothesis that emitted eos goes on at -10000): the ok rows of an image are pairwise distinct."""
    rng = np.random.RandomState(2)
    F, B, K, V, eos = 7, 4, 4, 6, 3
    tot, wids, ptrs = np.zeros((F, B, K), np.float32), np.zeros((F, B, K), np.int64), np.zeros((F, B, K), np.int64)
    for b in range(B):
        prev, prev_eos = np.zeros(1, np.float32), np.zeros(1, bool)
        for f in range(F):
            step = np.log(rng.dirichlet(np.ones(V), size=len(prev))).astype(np.float32)
            cont = (prev[:, None] + step + np.where(prev_eos, np.float32(-10000.0), np.float32(0.0))[:, None]).reshape(-1)
            best = np.argsort(-cont, kind="stable")[:K]
            tot[f, b], ptrs[f, b], wids[f, b] = cont[best], best // V, best % V
            prev, prev_eos = tot[f, b].copy(), wids[f, b] == eos
    seq, score, value, length, ok = beam_nbest_host(tot, wids, ptrs, K, eos, 0.4, F + 1)
    s, o, ln = by_image(seq, K), by_image(ok, K), by_image(length, K)
    assert o.sum() > B
    for b in range(B):
        rows = [tuple(s[b, n, :ln[b, n]].tolist()) for n in range(K) if o[b, n]]
        assert len(set(rows)) == len(rows), rows
        assert (by_image(score, K)[b][o[b] == 0] < -5000).all()             # what is not ok went on after its eos


def test_host_specification_refuses_bad_shapes():
    sc, ww, pp = random_frames(np.random.RandomState(3), 4, 2, 3)
    for n, out_len in ((0, 4), (4, 4), (2, 3)):
        with pytest.raises(ValueError):
            beam_nbest_host(sc, ww, pp, n, 3, 0.0, out_len)
    with pytest.raises(ValueError):
        beam_nbest_host(sc, ww[:3], pp, 1, 3, 0.0, 4)


def test_c_entry_checks_its_arguments_before_any_launch():
    """vlp_beam_nbest validates everything before it looks at a device: null operands and every limit come back as VLP_ERR_BAD_ARG here, on a
    machine without a GPU (the pointers are never followed)."""
    from vlp_amd import _lib
    lib = _lib.load()
    fake = ctypes.c_void_p(4096)

    def call(F=6, B=2, K=3, N=2, T=6, null=None):
        ops = [None if i == null else fake for i in range(8)]          # tot wids ptrs | seq score value len ok
        return lib.vlp_beam_nbest(ops[0], ops[1], ops[2], F, B, K, 3, 0.4, N, T, ops[3], ops[4], ops[5], ops[6], ops[7], None)
    for kw in (dict(N=4), dict(N=0), dict(K=65, N=1), dict(F=257, T=300), dict(F=0), dict(T=5), dict(B=0)) + tuple(dict(null=i) for i in range(8)):
        rc = call(**kw)
        assert rc != 0, kw
        msg = lib.vlp_last_error_string().decode()
        assert "vlp_beam_nbest" in msg, (kw, msg)
    assert "null operand" in msg
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        import torch
        z = torch.zeros(2, 1, 2)
        _lib.beam_nbest(z, z.long(), z.long(), 1, 3, 0.0, torch.zeros(1, 2, dtype=torch.long), z, z, z, z)


# ---- python -m vlp_amd.decode_img2txt --n_best ----------------------------------------------------------------------------
BASE = ["--model_recover_path", "m.bin", "--packed_features", "store", "--fp16", "--enable_butd"]


def parse(*extra):
    from vlp_amd import decode_img2txt as D
    return D.parse_args(BASE + list(extra))


@pytest.mark.parametrize("extra,message", [
    (("--beam_size", "3", "--n_best", "4"), "--n_best must be in 1..--beam_size"),
    (("--beam_size", "3", "--n_best", "0"), "--n_best must be in 1..--beam_size"),
    (("--n_best", "2"), "needs --beam_size >= 2"),
    (("--beam_size", "3", "--select", "logprob"), "needs --n_best >= 2"),
    (("--beam_size", "3", "--n_best", "1", "--select", "consensus", "--consensus_df", "t.npz"), "needs --n_best >= 2"),
    (("--beam_size", "3", "--n_best", "3", "--select", "consensus"), "needs --consensus_df"),
    (("--beam_size", "3", "--n_best", "3", "--select", "logprob", "--consensus_df", "t.npz"), "needs --select consensus"),
    (("--beam_size", "20", "--n_best", "17", "--select", "consensus", "--consensus_df", "t.npz"), "2..16 hypotheses"),
    (("--beam_size", "3", "--nbest_file", "n.json"), "needs --n_best >= 2"),
    (("--beam_size", "3", "--n_best", "2", "--nbest_file", "a.json", "--samples_file", "b.json"), "alias of --nbest_file"),
])
def test_command_line_errors(capsys, extra, message):
    with pytest.raises(SystemExit) as e:
        parse(*extra)
    assert e.value.code == 2
    assert message in capsys.readouterr().err


def test_command_line_accepted_combinations():
    a = parse()
    assert (a.n_best, a.nbest_file, a.select, a.beam_size) == (1, None, "none", 1)
    a = parse("--beam_size", "3")
    assert a.n_best == 1 and a.select == "none"
    a = parse("--beam_size", "3", "--n_best", "3", "--nbest_file", "n.json")
    assert (a.n_best, a.nbest_file, a.select) == (3, "n.json", "none")
    a = parse("--beam_size", "5", "--n_best", "2", "--select", "logprob", "--samples_file", "s.json", "--length_penalty", "0.4")
    assert (a.n_best, a.nbest_file, a.select, a.length_penalty) == (2, "s.json", "logprob", 0.4)
    a = parse("--beam_size", "16", "--n_best", "16", "--select", "consensus", "--consensus_df", "t.npz")
    assert (a.n_best, a.select, a.consensus_df) == (16, "consensus", "t.npz")
    a = parse("--beam_size", "64", "--n_best", "64", "--select", "logprob")
    assert a.n_best == 64
    # the flags the tool had keep their names and defaults, and the sampling tool's parser is not touched by them
    from vlp_amd import decode_img2txt as D
    from vlp_amd import sample_img2txt as SI
    assert not hasattr(D.build_parser().parse_args(BASE), "n_best")
    assert not hasattr(SI.parse_args(BASE), "n_best")


def test_model_refuses_more_hypotheses_than_beams():
    from vlp_amd.modeling import BertConfig
    cfg = BertConfig(128, num_hidden_layers=1, type_vocab_size=6)
    with pytest.raises(ValueError, match="n_best=4"):
        BertForSeq2SeqDecoder(cfg, search_beam_size=3, n_best=4, enable_butd=True, len_vis_input=100)
    m = BertForSeq2SeqDecoder(cfg, search_beam_size=3, n_best=3, enable_butd=True, len_vis_input=100)
    assert m.n_best == 3 and m.backtrack == "host" and BertForSeq2SeqDecoder.backtrack == "host"
