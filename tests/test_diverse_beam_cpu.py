"""CPU: diverse (group) beam search -- the host specification vlp_amd.diverse.beam_select_groups_host, its limits, the argument checks of
vlp_beam_select_groups (they run before anything touches a device), the command line of python -m vlp_amd.decode_img2txt --beam_groups and
the model's constructor."""
import ctypes
import itertools

import numpy as np
import pytest

from tests import diverse_util as DU
from vlp_amd.diverse import beam_select_groups_host, check_limits

F32 = np.float32
NINF = -np.inf


def test_specification_by_hand():
    """One image, K = 4, G = 2 (Kg = 2), a later frame, lambda = 1.5, eos = 6, no parent has ended.

        row  last_total  kk_scores                 kk_ids       v0 = kk + last_total
        0    -1          -1    -2    -3    -4      7 8 9 5      -2     -3    -4    -5        i =  0 ..  3
        1    -1          -1    -2.5  -3    -4      7 5 9 8      -2     -3.5  -4    -5        i =  4 ..  7
        2    -1          -0.5  -1    -3    -3.5    7 6 9 5      -1.5   -2    -4    -4.5      i =  8 .. 11
        3    -2          -0.25 -2    -3    -inf    6 7 8 4      -2.25  -4    -5    -inf      i = 12 .. 15

    Group 0 (rows 0, 1; nothing is penalised): the maximum -2 is held by i = 0 and i = 4, a tie that the index resolves: pick i = 0 (row 0,
    word 7), then i = 4 (row 1, word 7).  Word 7 now has a count of 2.
    Group 1 (rows 2, 3): keys = v0 - 1.5 * c with c = 2 for word 7, 0 otherwise:
        row 2:  -1.5 - 3 = -4.5   -2     -4    -4.5
        row 3:  -2.25             -4 - 3 = -7  -5    -inf
    pick i = 9 (row 2, word 6, key -2), then i = 12 (row 3, word 6, key -2.25).  Without the penalty i = 8 (word 7, v0 = -1.5) would have been
    the group's first pick: it loses only because group 0 chose word 7 twice.  The -inf candidate i = 15 is never reached.
    The outputs carry v0, not the key; both picks of group 1 are eos."""
    ks = np.array([[[-1, -2, -3, -4], [-1, -2.5, -3, -4], [-0.5, -1, -3, -3.5], [-0.25, -2, -3, NINF]]], dtype=F32)
    ki = np.array([[[7, 8, 9, 5], [7, 5, 9, 8], [7, 6, 9, 5], [6, 7, 8, 4]]], dtype=np.int64)
    lt, le = np.array([[-1, -1, -1, -2]], dtype=F32), np.zeros((1, 4), F32)
    sc, ids, ptrs, eos, src, nxt = beam_select_groups_host(ks, ki, lt, le, False, 6, 2, 1.5, next_ids_stride=2)
    assert sc.dtype == F32 and ids.dtype == np.int64 and ptrs.dtype == np.int64 and eos.dtype == F32 and src.dtype == np.int64
    assert sc.tolist() == [[-2.0, -2.0, -2.0, -2.25]]
    assert ids.tolist() == [[7, 7, 6, 6]] and ptrs.tolist() == [[0, 1, 2, 3]] and eos.tolist() == [[0.0, 0.0, 1.0, 1.0]]
    assert src.tolist() == [0, 1, 2, 3] and nxt.shape == (4, 2) and nxt[:, 0].tolist() == [7, 7, 6, 6] and not nxt[:, 1].any()
    # the same frame without the penalty: group 1 takes word 7 first
    sc0, ids0, ptrs0 = beam_select_groups_host(ks, ki, lt, le, False, 6, 2, 0.0)[:3]
    assert ids0.tolist() == [[7, 7, 7, 6]] and ptrs0.tolist() == [[0, 1, 2, 2]] and sc0.tolist() == [[-2.0, -2.0, -1.5, -2.0]]
    # row 1's parent had ended: its continuations drop by 10000 and group 0 takes row 0's two best; word 7 then counts once
    le1 = np.array([[0, 1, 0, 0]], dtype=F32)
    sc1, ids1, ptrs1 = beam_select_groups_host(ks, ki, lt, le1, False, 6, 2, 1.5)[:3]
    assert ids1.tolist() == [[7, 8, 6, 6]] and ptrs1.tolist() == [[0, 0, 2, 3]] and sc1.tolist() == [[-2.0, -3.0, -2.0, -2.25]]
    # the first frame: every group sees the one row; lambda = 0 -> the groups pick the same words, lambda > 0 -> the next ones
    f_s, f_i = np.array([[-1, -2, -3, NINF]], dtype=F32), np.array([[7, 8, 9, 5]], dtype=np.int64)
    a = beam_select_groups_host(f_s, f_i, None, None, True, 6, 2, 0.0)
    assert a[1].tolist() == [[7, 8, 7, 8]] and a[2].tolist() == [[0, 0, 0, 0]] and a[4].tolist() == [0, 0, 0, 0]
    a = beam_select_groups_host(f_s, f_i, None, None, True, 6, 2, 100.0)
    assert a[1].tolist() == [[7, 8, 9, 7]] and a[0].tolist() == [[-1.0, -2.0, -3.0, -1.0]]      # group 1's keys: -101 -102 -3 -inf
    # four groups of one, lambda = 0.5: keys of word 7 / 8 / 9 are -1 -2 -3, then -1.5 -2 -3 (7 again), then -2 -2 -3 (a tie: the index
    # keeps 7), then -2.5 -2 -3 (8)
    a = beam_select_groups_host(f_s, f_i, None, None, True, 6, 4, 0.5)
    assert a[1].tolist() == [[7, 7, 7, 8]] and a[0].tolist() == [[-1.0, -1.0, -1.0, -2.0]]


def test_a_fused_key_is_not_the_specification(monkeypatch):
    """The product is rounded before the subtraction.  On DU.separating_frame (its docstring has the arithmetic) the two roundings order word
    10 before word 11 in group 1; a fused multiply-subtract (one rounding) ties the two keys and the index puts word 11 first.  The hostile
    frames of the GPU test cannot tell the two apart (their v0 sit on a 0.25 grid), which is why this frame exists."""
    from vlp_amd import diverse as DV
    fr, lam = DU.separating_frame(), DU.SEPARATING_PENALTY
    spec = beam_select_groups_host(*fr, False, DU.EOS, 2, lam)
    assert spec[1][0].tolist() == [11] * 7 + [10, 10] + [10, 11] + [102 + 18 * 9 + j for j in range(7)]
    assert spec[0][0, 9:11].tolist() == [-3.75, -2.25] and spec[2][0].tolist() == list(range(9)) + [9] * 9
    k11 = DV._key(np.array([-2.25], F32), F32(lam), np.array([7], F32))[0]
    k10 = DV._key(np.array([-3.75], F32), F32(lam), np.array([2], F32))[0]
    assert (float(k11) * 2 ** 21, float(k10) * 2 ** 21) == (-9122612.0, -9122611.0)
    assert DU.fused_key(np.array([-2.25], F32), F32(lam), np.array([7], F32))[0] == k10        # one rounding: a tie
    with monkeypatch.context() as mp:
        mp.setattr(DV, "_key", DU.fused_key)
        fused = beam_select_groups_host(*fr, False, DU.EOS, 2, lam)
    assert fused[1][0, 9:11].tolist() == [11, 10] and fused[0][0, 9:11].tolist() == [-2.25, -3.75]
    assert all(np.array_equal(a[0, [*range(9), *range(11, 18)]], b[0, [*range(9), *range(11, 18)]]) for a, b in zip(spec[:4], fused[:4]))


def test_groups_1_is_the_scan_of_beam_select_kernel():
    rng = np.random.RandomState(0)
    for trial in range(60):
        B, K = int(rng.randint(1, 4)), int(rng.randint(2, 7))
        first = trial % 3 == 0
        ks, ki, lt, le = DU.hostile_frame(B, K, first, 100 + trial)
        want = DU.scan_select(ks, ki, lt, le, first, DU.EOS)
        for lam in (0.0, 0.3, 100.0):
            got = beam_select_groups_host(ks, ki, lt, le, first, DU.EOS, 1, lam)
            for g, w, name in zip(got, want, ("scores", "ids", "ptrs", "eos", "src_rows")):
                assert g.dtype == w.dtype and np.array_equal(g.view(np.uint8), w.view(np.uint8)), (trial, lam, name, g, w)


@pytest.mark.parametrize("V", [12, 40])
@pytest.mark.parametrize("K", [2, 4, 6])
def test_top_k_lists_are_sufficient(V, K):
    """The specification fed the per-row top-K lists picks the (parent, word) pairs a brute force over the whole vocabulary picks.  The scores
    are continuous random draws, so there are no ties: with ties the two forms order equal scores differently by construction (the list by
    word id within a row and r*K + j across rows, the brute force by r*V + v) and may name different words of equal score."""
    rng = np.random.RandomState(1000 * V + K)
    B = 3
    for G in [g for g in range(1, K + 1) if K % g == 0]:
        for lam in (0.0, 0.3, 5.0):
            for first in (True, False):
                logp = np.log(rng.dirichlet(np.ones(V), size=(B,) if first else (B, K))).astype(F32)
                lt = None if first else (-3.0 * rng.rand(B, K)).astype(F32)
                le = None if first else (rng.rand(B, K) < 0.25).astype(F32)
                ks, ki = DU.topk_lists(logp, K)
                sc, ids, ptrs = beam_select_groups_host(ks, ki, lt, le, first, DU.EOS, G, lam)[:3]
                want = DU.brute_force(logp, lt, le, first, K, G, lam)
                for b in range(B):
                    assert list(zip(ptrs[b].tolist(), ids[b].tolist())) == want[b], (G, lam, first, b)


def test_parents_stay_inside_their_group():
    rng = np.random.RandomState(7)
    for K, G in ((4, 2), (6, 3), (6, 2), (6, 6), (8, 4)):
        B, Kg, V = 3, K // G, 9
        ks, ki = DU.topk_lists(np.log(rng.dirichlet(np.ones(V), size=B)).astype(F32), K)
        tot, ids, ptrs, eos = beam_select_groups_host(ks, ki, None, None, True, DU.EOS, G, 0.7)[:4]
        assert not ptrs.any()
        for s in range(1, 7):
            ks, ki = DU.topk_lists(np.log(rng.dirichlet(np.ones(V), size=(B, K))).astype(F32), K)
            tot, ids, ptrs, eos, src = beam_select_groups_host(ks, ki, tot, eos, False, DU.EOS, G, 0.7)[:5]
            assert np.array_equal(ptrs // Kg, np.broadcast_to(np.arange(K) // Kg, (B, K))), (K, G, s, ptrs)
            assert np.array_equal(src, (np.arange(B)[:, None] * K + ptrs).reshape(-1))


def test_check_limits():
    for K, G, lam in ((2, 1, 0.0), (2, 2, 0.5), (6, 3, 100.0), (64, 64, 1e30), (64, 1, 0.0), (12, 4, 0)):
        check_limits(K, G, lam)
    for K, G, lam in ((1, 1, 0.0), (65, 5, 0.0), (6, 0, 0.0), (6, 7, 0.0), (6, 4, 0.0), (6, -2, 0.0), (6, 3, -0.1), (6, 3, float("nan")),
                      (6, 3, float("inf")), (6, 3, None)):
        with pytest.raises(ValueError, match="diverse beam search"):
            check_limits(K, G, lam)
    ks, ki = np.zeros((1, 4, 4), F32), np.zeros((1, 4, 4), np.int64)
    with pytest.raises(ValueError):
        beam_select_groups_host(ks, ki, np.zeros((1, 4), F32), np.zeros((1, 4), F32), False, 3, 3, 0.0)
    with pytest.raises(ValueError):
        beam_select_groups_host(ks, ki, None, None, False, 3, 2, 0.0)
    with pytest.raises(ValueError):
        beam_select_groups_host(ks, ki[:, :3], np.zeros((1, 4), F32), np.zeros((1, 4), F32), False, 3, 2, 0.0)


def test_c_entry_checks_its_arguments_before_any_launch():
    """vlp_beam_select_groups validates everything before it looks at a device: every bad input comes back as VLP_ERR_BAD_ARG with the
    function's name, on a machine without a GPU (the pointers are never followed)."""
    from vlp_amd import _lib
    lib = _lib.load()
    assert "vlp_beam_select_groups" in _lib.SYMBOLS
    fake = ctypes.c_void_p(4096)
    names = ("kk_scores", "kk_ids", "last_total", "last_eos", "out_scores", "out_ids", "out_ptrs", "out_eos", "src_rows", "next_ids")

    def call(B=2, K=6, G=3, lam=0.5, first=0, null=(), no_struct=False):
        a = _lib.BeamSelectArgs(*([None if n in null else fake for n in names] + [2, B, K, first, 3]))
        return lib.vlp_beam_select_groups(None if no_struct else ctypes.byref(a), G, lam, None)
    bad = [dict(no_struct=True), dict(K=0), dict(K=65, G=5), dict(G=0), dict(G=-1), dict(G=4), dict(G=7), dict(B=0), dict(lam=float("nan")),
           dict(lam=-0.5), dict(lam=float("inf")), dict(null=("last_total",)), dict(null=("last_eos",))]
    bad += [dict(null=(n,), first=1) for n in names if not n.startswith("last_")]
    for kw in bad:
        rc = call(**kw)
        assert rc == -1, kw                                       # VLP_ERR_BAD_ARG
        msg = lib.vlp_last_error_string().decode()
        assert "vlp_beam_select_groups" in msg, (kw, msg)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        import torch
        z = torch.zeros(2, 2)
        _lib.beam_select_groups(z, z.long(), None, None, z, z.long(), z.long(), z, z.long().view(-1), z.long().view(-1), 2, 2, True, 3, 2, 0.5)


# ---- python -m vlp_amd.decode_img2txt --beam_groups ------------------------------------------------------------------------
BASE = ["--model_recover_path", "m.bin", "--packed_features", "store", "--fp16", "--enable_butd"]


def parse(*extra):
    from vlp_amd import decode_img2txt as D
    return D.parse_args(BASE + list(extra))


@pytest.mark.parametrize("extra,message", [
    (("--beam_size", "4", "--beam_groups", "0"), "--beam_groups must be in 1..--beam_size"),
    (("--beam_size", "4", "--beam_groups", "8"), "--beam_groups must be in 1..--beam_size"),
    (("--beam_groups", "2"), "--beam_groups must be in 1..--beam_size"),
    (("--beam_size", "6", "--beam_groups", "4"), "must divide --beam_size"),
    (("--beam_size", "6", "--diversity_penalty", "0.5"), "needs --beam_groups >= 2"),
    (("--beam_size", "6", "--beam_groups", "1", "--diversity_penalty", "0.5"), "needs --beam_groups >= 2"),
    (("--beam_size", "6", "--beam_groups", "2", "--diversity_penalty", "-0.5"), "--diversity_penalty must be finite and >= 0"),
    (("--beam_size", "6", "--beam_groups", "2", "--diversity_penalty", "inf"), "--diversity_penalty must be finite and >= 0"),
    (("--beam_size", "6", "--beam_groups", "2", "--diversity_penalty", "nan"), "--diversity_penalty must be finite and >= 0"),
])
def test_command_line_errors(capsys, extra, message):
    with pytest.raises(SystemExit) as e:
        parse(*extra)
    assert e.value.code == 2
    assert message in capsys.readouterr().err


def test_command_line_accepted_combinations():
    a = parse()
    assert (a.beam_groups, a.diversity_penalty, a.beam_size) == (1, 0.0, 1)
    a = parse("--beam_size", "6")
    assert (a.beam_groups, a.diversity_penalty) == (1, 0.0)
    a = parse("--beam_size", "6", "--beam_groups", "3", "--diversity_penalty", "0.5")
    assert (a.beam_groups, a.diversity_penalty) == (3, 0.5)
    a = parse("--beam_size", "6", "--beam_groups", "6")
    assert (a.beam_groups, a.diversity_penalty) == (6, 0.0)
    a = parse("--beam_size", "4", "--beam_groups", "2", "--diversity_penalty", "1", "--n_best", "4", "--select", "consensus", "--consensus_df", "t.npz",
              "--nbest_file", "n.json", "--forbid_duplicate_ngrams", "--min_len", "3")
    assert (a.beam_groups, a.n_best, a.select, a.nbest_file, a.min_len) == (2, 4, "consensus", "n.json", 3)
    from vlp_amd import sample_img2txt as SI
    assert not hasattr(SI.parse_args(BASE), "beam_groups")


def test_model_constructor_refusals():
    from vlp_amd.modeling import BertConfig, BertForSeq2SeqDecoder
    cfg = BertConfig(128, num_hidden_layers=1, type_vocab_size=6)

    def make(**kw):
        return BertForSeq2SeqDecoder(cfg, enable_butd=True, len_vis_input=100, **kw)
    for kw, match in ((dict(search_beam_size=6, beam_groups=4), "beam_groups=4"),
                      (dict(search_beam_size=6, beam_groups=0), "beam_groups=0"),
                      (dict(search_beam_size=6, beam_groups=12), "beam_groups=12"),
                      (dict(search_beam_size=1, beam_groups=2), "beam_groups=2"),
                      (dict(search_beam_size=6, diversity_penalty=0.5), "diversity_penalty=0.5"),
                      (dict(search_beam_size=6, beam_groups=3, diversity_penalty=-1.0), "diversity_penalty=-1.0"),
                      (dict(search_beam_size=6, beam_groups=3, diversity_penalty=float("nan")), "diversity_penalty=nan"),
                      (dict(search_beam_size=6, beam_groups=3, diversity_penalty=float("inf")), "diversity_penalty=inf")):
        with pytest.raises(ValueError, match=match):
            make(**kw)
    m = make(search_beam_size=6, beam_groups=3, diversity_penalty=0.5, n_best=6)
    assert (m.beam_groups, m.diversity_penalty, m.group_select, BertForSeq2SeqDecoder.group_select) == (3, 0.5, "device", "device")
    m = make(search_beam_size=3)
    assert (m.beam_groups, m.diversity_penalty) == (1, 0.0)
    assert make().beam_groups == 1                                  # greedy decoders are not bothered


def test_group_counts_over_all_divisors():
    """Every G dividing K fills every slot exactly once and group g's picks come from its rows, on hostile frames (ties, -inf, ended parents)."""
    for K in (2, 4, 6, 12):
        for G, first in itertools.product([g for g in range(1, K + 1) if K % g == 0], (True, False)):
            ks, ki, lt, le = DU.hostile_frame(3, K, first, 10 * K + G)
            for lam in (0.0, 0.3, 100.0):
                sc, ids, ptrs, eos, src, nxt = beam_select_groups_host(ks, ki, lt, le, first, DU.EOS, G, lam)
                assert np.array_equal(eos, (ids == DU.EOS).astype(F32)) and np.array_equal(nxt[:, 0], ids.reshape(-1))
                if first:
                    assert not ptrs.any() and np.array_equal(src, np.repeat(np.arange(3), K))
                else:
                    assert np.array_equal(ptrs // (K // G), np.broadcast_to(np.arange(K) // (K // G), (3, K)))
