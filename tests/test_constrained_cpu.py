"""CPU: constrained beam search -- the host specification vlp_amd.constrained (state, advance, wanted, bank, the banked selection,
constraints_met), its limits, and the command line of python -m vlp_amd.decode_img2txt --constraints_file with its WordPiece split."""
import json

import numpy as np
import pytest

from vlp_amd import constrained as CB
from vlp_amd.diverse import beam_select_groups_host

F32 = np.float32
NINF = -np.inf
EOS = 6


def st(met=0, cur=-1, off=0):
    return met | ((cur + 1) << 8) | (off << 16)


# three phrases: 0 = [10, 11, 12], 1 = [10, 20] (shares its first piece with 0), 2 = [30]; slot 3 is unused
CID = np.array([[10, 11, 12], [10, 20, 0], [30, 0, 0], [0, 0, 0]], np.int32)
CLN = np.array([3, 2, 1, 0], np.int32)


def test_advance_wanted_bank_by_hand():
    assert CB.bank(0, CLN) == 0 and CB.wanted(0, CID, CLN).tolist() == [10, 10, 30, -1] and CB.full_mask(CLN) == 0b0111
    # two phrases share the first piece: the lowest unmet one begins
    s = CB.advance(0, 10, CID, CLN)
    assert s == st(0, 0, 1) and CB.bank(s, CLN) == 1 and CB.wanted(s, CID, CLN).tolist() == [11, 10, 30, -1]
    s2 = CB.advance(s, 11, CID, CLN)
    assert s2 == st(0, 0, 2) and CB.bank(s2, CLN) == 2 and CB.wanted(s2, CID, CLN).tolist() == [12, 10, 30, -1]
    # a phrase dropped mid-way: no fallback to phrase 1 although "10 20" would read on from the 10 two words back; the start rule sees 20
    d = CB.advance(s, 20, CID, CLN)
    assert d == 0 and CB.bank(d, CLN) == 0
    # dropped by a word that itself starts a phrase: the start rule applies to it
    d = CB.advance(s2, 10, CID, CLN)
    assert d == st(0, 0, 1)
    d = CB.advance(s2, 30, CID, CLN)                 # len == 1: met at once
    assert d == st(0b100) and CB.bank(d, CLN) == 1 and CB.wanted(d, CID, CLN).tolist() == [10, 10, -1, -1]
    # finishing phrase 0; then 10 begins phrase 1, the lowest that is not met
    m = CB.advance(s2, 12, CID, CLN)
    assert m == st(0b001) and CB.bank(m, CLN) == 3 and CB.wanted(m, CID, CLN).tolist() == [-1, 10, 30, -1]
    n = CB.advance(m, 10, CID, CLN)
    assert n == st(0b001, 1, 1) and CB.bank(n, CLN) == 4 and CB.wanted(n, CID, CLN).tolist() == [-1, 20, 30, -1]
    f = CB.advance(CB.advance(n, 20, CID, CLN), 30, CID, CLN)
    assert f == st(0b111) and CB.bank(f, CLN) == 6 == int(CLN.sum()) and CB.wanted(f, CID, CLN).tolist() == [-1] * 4
    # a frozen ended beam keeps its parent's state whatever the word, and wants nothing
    assert CB.advance(s2, 12, CID, CLN, parent_ended=True) == s2
    assert CB.wanted(s2, CID, CLN, ended=True).tolist() == [-1] * 4
    # an unrelated word leaves an idle state alone
    assert CB.advance(m, 99, CID, CLN) == m


def test_constraints_met():
    assert CB.constraints_met([1, 10, 11, 12, 2, 30], CID, CLN) == 0b101
    assert CB.constraints_met([10, 11, 10, 20], CID, CLN) == 0           # dropped, restarted phrase 0, dropped again
    assert CB.constraints_met([10, 11, 12, 10, 20, 30, EOS, 0, 0], CID, CLN) == 0b111
    assert CB.constraints_met(np.array([10, 11, EOS, 12, 30]), CID, CLN, eos_id=EOS) == 0     # cut at the first eos
    assert CB.constraints_met([], CID, CLN) == 0
    assert CB.constraints_met([5, 6, 7], np.zeros((1, 1), np.int32), np.zeros(1, np.int32)) == 0


def test_limits_and_checks():
    CB.check_limits(2, 1, 1)
    CB.check_limits(64, 8, 8)
    for bad in ((1, 1, 1), (65, 1, 1), (4, 0, 1), (4, 9, 1), (4, 1, 0), (4, 1, 9)):
        with pytest.raises(ValueError):
            CB.check_limits(*bad)
    ci, cl = CB.pack_constraints([[[7, 8], [9]], []], 2)
    assert ci.shape == (2, 2, 2) and cl.tolist() == [[2, 1], [0, 0]] and ci[0].tolist() == [[7, 8], [9, 0]]
    assert CB.pack_constraints([[], []], 2)[0].shape == (2, 1, 1)
    assert CB.pack_constraints([[[7]], []], 2, C=3, Lc=4)[0].shape == (2, 3, 4)
    CB.check_constraints(ci, cl, 100, EOS)
    with pytest.raises(ValueError, match="end-of-sequence"):
        CB.check_constraints(*CB.pack_constraints([[[7, EOS]]], 1), 100, EOS)
    with pytest.raises(ValueError, match="outside the vocabulary"):
        CB.check_constraints(*CB.pack_constraints([[[7, 100]]], 1), 100, EOS)
    with pytest.raises(ValueError, match="cons_len"):
        CB.check_constraints(np.zeros((1, 1, 2), np.int32), np.array([[3]], np.int32), 100, EOS)
    with pytest.raises(ValueError, match="empty phrase"):
        CB.pack_constraints([[[]]], 1)
    with pytest.raises(ValueError, match="at most"):
        CB.pack_constraints([[[1]] * 9], 1)
    with pytest.raises(ValueError, match="entries"):
        CB.pack_constraints([[]], 2)
    # unused slots may hold anything: only the used ids are checked
    CB.check_constraints(np.full((1, 2, 2), EOS, np.int32), np.zeros((1, 2), np.int32), 100, EOS)


def random_frame(rng, B, K, first):
    shape = (B, K) if first else (B, K, K)
    ks = (-rng.integers(0, 40, size=shape) * 0.25).astype(F32)
    ks = np.sort(ks, axis=-1)[..., ::-1].copy()
    ki = rng.integers(0, 50, size=shape).astype(np.int64)
    lt = (-rng.integers(0, 40, size=(B, K)) * 0.25).astype(F32)
    le = (rng.random((B, K)) < 0.3).astype(F32)
    return ks, ki, lt, le


@pytest.mark.parametrize("first", [True, False])
def test_no_constraints_is_the_plain_selection(first):
    """Every cons_len == 0: no extra slot, one bank, no unmet eos -- the picks of the plain selection (diverse.py with one group)."""
    rng = np.random.default_rng(5)
    for B, K, C in ((1, 2, 1), (3, 5, 2), (2, 8, 8)):
        ks, ki, lt, le = random_frame(rng, B, K, first)
        R = 1 if first else K
        want = rng.integers(-1, 50, size=(B, R, C)).astype(np.int32)            # whatever the want buffer holds: wanted() of such a search is -1
        want[:] = -1
        wv = np.full((B, R, C), NINF, F32)
        ref = beam_select_groups_host(ks, ki, None if first else lt, None if first else le, first, EOS, 1, 0.0, next_ids_stride=2)
        got = CB.beam_select_constrained_host(ks, ki, want, wv, None if first else lt, None if first else le,
                                              None if first else np.zeros((B, K), np.int32), np.zeros((B, C, 3), np.int32),
                                              np.zeros((B, C), np.int32), first, EOS, next_ids_stride=2)
        for a, b in zip(ref, got[:6]):
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
        assert not got[6].any() and (got[7] == -1).all()


def test_wanted_slots_are_deduplicated():
    """K = 2, C = 3, first frame.  The list holds words 7 and 8; wanted = [8, 9, 9]: slot 0 repeats a list id, slot 2 repeats slot 1 -- one
    extra candidate (word 9, i = 3) exists.  It is the only one in bank 1, so the cursor (Tb = 3) reaches it first."""
    ks, ki = np.array([[-1.0, -2.0]], F32), np.array([[7, 8]], np.int64)
    cid = np.array([[[8], [9], [9]]], np.int32)
    cln = np.ones((1, 3), np.int32)
    want, wv = np.array([[8, 9, 9]], np.int32), np.array([[-55.0, -7.0, -66.0]], F32)
    out = CB.beam_select_constrained_host(ks, ki, want, wv, None, None, None, cid, cln, True, EOS)
    # candidates: i=0 word 7 bank 0 v0 -1; i=1 word 8 bank 1 (phrase 0 met) v0 -2; i=3 word 9 bank 1 (phrase 1 met; the lowest c) v0 -7
    assert out[1].tolist() == [[8, 7]] and out[0].tolist() == [[-2.0, -1.0]]
    assert out[6].tolist() == [[0b001, 0]] and out[7].tolist() == [[-1, 9, 9], [8, 9, 9]]
    # with a third beam the deduplicated slot shows: -7, never the -55 / -66 of the absent slots
    ks3, ki3 = np.array([[-1.0, -2.0, -3.0]], F32), np.array([[7, 8, 5]], np.int64)
    out = CB.beam_select_constrained_host(ks3, ki3, want, wv, None, None, None, cid, cln, True, EOS)
    assert out[1].tolist() == [[8, 7, 9]] and out[0].tolist() == [[-2.0, -1.0, -7.0]] and out[6].tolist() == [[0b001, 0, 0b010]]
    # -1 is absent as well
    out = CB.beam_select_constrained_host(ks3, ki3, np.array([[-1, -1, -1]], np.int32), wv, None, None, None, cid, cln, True, EOS)
    assert out[1].tolist() == [[8, 7, 5]]


def test_unmet_eos_is_forbidden_and_picked_last():
    """K = 2, a later frame, one phrase [9].  Row 0 (state 0) offers eos at -0.5 and word 7 at -1; row 1's parent had ended.  The eos is unmet:
    it gets -10000 and is dead; word 7 and the wanted word 9 (-8) are the live candidates; with K = 3 picks the dead ones follow by value."""
    cid, cln = np.array([[[9]]], np.int32), np.array([[1]], np.int32)
    ks = np.array([[[-0.5, -1.0], [-0.25, -0.75]]], F32)
    ki = np.array([[[EOS, 7], [EOS, 3]]], np.int64)
    want, wv = np.array([[[9], [-1]]], np.int32), np.array([[[-8.0], [NINF]]], F32)
    lt, le, ps = np.array([[-1.0, -2.0]], F32), np.array([[0.0, 1.0]], F32), np.array([[0, 0]], np.int32)
    tr = {}
    out = CB.beam_select_constrained_host(ks, ki, want, wv, lt, le, ps, cid, cln, False, EOS, trace=tr)
    assert out[1].tolist() == [[9, 7]] and out[0].tolist() == [[-9.0, -2.0]] and out[2].tolist() == [[0, 0]]
    assert out[6].tolist() == [[1, 0]] and out[7].tolist() == [[-1], [9]] and tr["unmet_eos"] == 1 and tr["dead_picks"] == 0
    # K = 3 at the same rule: one live candidate short -> the best dead one, the unmet eos at -0.5 - 10000 - 1 (row 1: -0.25 - 10000 - 2)
    ks = np.array([[[-0.5, -1.0, -30.0], [-0.25, -0.75, -1.0], [-0.25, -0.75, -1.0]]], F32)
    ki = np.array([[[EOS, 7, 9], [EOS, 3, 4], [EOS, 3, 4]]], np.int64)
    want, wv = np.array([[[9], [-1], [-1]]], np.int32), np.array([[[-30.0], [NINF], [NINF]]], F32)
    lt, le, ps = np.array([[-1.0, -2.0, -3.0]], F32), np.array([[0.0, 1.0, 1.0]], F32), np.zeros((1, 3), np.int32)
    tr = {}
    out = CB.beam_select_constrained_host(ks, ki, want, wv, lt, le, ps, cid, cln, False, EOS, trace=tr)
    assert out[1].tolist() == [[9, 7, EOS]] and out[0].tolist() == [[-31.0, -2.0, F32(-0.5) + F32(-10000.0) + F32(-1.0)]]
    assert out[3].tolist() == [[0.0, 0.0, 1.0]] and out[7][2].tolist() == [-1] and tr["dead_picks"] == 1
    # once the phrase is met the eos is an ordinary word
    ps = np.array([[1, 0, 0]], np.int32)
    out = CB.beam_select_constrained_host(ks, ki, want, wv, lt, le, ps, cid, cln, False, EOS)
    assert out[1][0, 0] == EOS and out[0][0, 0] == F32(-1.5)


def test_last_frame_forbids_every_unmet_end():
    """The frame of test_unmet_eos_is_forbidden_and_picked_last as the search's last: word 7 leaves the phrase unmet and is forbidden as the eos
    is; the wanted word 9 is the one live candidate, the dead follow by value.  With the phrase met before, nothing changes."""
    cid, cln = np.array([[[9]]], np.int32), np.array([[1]], np.int32)
    ks = np.array([[[-0.5, -1.0], [-0.25, -0.75]]], F32)
    ki = np.array([[[EOS, 7], [EOS, 3]]], np.int64)
    want, wv = np.array([[[9], [-1]]], np.int32), np.array([[[-8.0], [NINF]]], F32)
    lt, le, ps = np.array([[-1.0, -2.0]], F32), np.array([[0.0, 1.0]], F32), np.array([[0, 0]], np.int32)
    tr = {}
    out = CB.beam_select_constrained_host(ks, ki, want, wv, lt, le, ps, cid, cln, False, EOS, trace=tr, last=True)
    assert out[1].tolist() == [[9, EOS]] and out[0].tolist() == [[-9.0, F32(-0.5) + F32(-10000.0) + F32(-1.0)]]
    assert tr["unmet_eos"] == 2 and tr["dead_picks"] == 1 and out[6].tolist() == [[1, 0]]
    ps = np.array([[1, 0]], np.int32)
    a = CB.beam_select_constrained_host(ks, ki, want, wv, lt, le, ps, cid, cln, False, EOS, last=True)
    b = CB.beam_select_constrained_host(ks, ki, want, wv, lt, le, ps, cid, cln, False, EOS, last=False)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)) and a[1].tolist() == [[EOS, 7]]
    # the first frame as the last (a one-token target)
    out = CB.beam_select_constrained_host(ks[:, 0], ki[:, 0], want[:, 0], wv[:, 0], None, None, None, cid, cln, True, EOS, last=True)
    assert out[1].tolist() == [[9, EOS]] and out[0].tolist() == [[-8.0, -10000.5]]


def test_bank_cursor_order():
    """K = 4, a later frame, one phrase [10, 11] (Tb = 2).  Parents: row 0 idle, row 1 with one token matched, row 2 and 3 idle.
        bank 2: row 1 + word 11 (-9)                    bank 1: row 0 + word 10 (-5), row 2 + word 10 (-4)
        bank 0: everything else; the best are row 3 + word 5 (-1) and row 0 + word 5 (-1.5)
    The cursor starts at 2: picks bank 2, bank 1 (the better: row 2), bank 0, then wraps to bank 2 -- empty, so on to bank 1's second."""
    cid, cln = np.array([[[10, 11]]], np.int32), np.array([[2]], np.int32)
    ki = np.array([[[5, 10, 1, 2], [5, 11, 1, 2], [5, 10, 1, 2], [5, 3, 1, 2]]], np.int64)
    ks = np.array([[[-1.5, -5, -6, -7], [-3, -9, -10, -11], [-2, -4, -6, -7], [-1, -5, -6, -7]]], F32)
    want = np.array([[[10], [11], [10], [10]]], np.int32)                     # all in the lists but row 3's
    wv = np.array([[[-5], [-9], [-4], [-20]]], F32)
    lt, le = np.zeros((1, 4), F32), np.zeros((1, 4), F32)
    ps = np.array([[0, st(0, 0, 1), 0, 0]], np.int32)
    tr = {}
    out = CB.beam_select_constrained_host(ks, ki, want, wv, lt, le, ps, cid, cln, False, EOS, trace=tr)
    assert out[1].tolist() == [[11, 10, 5, 10]] and out[2].tolist() == [[1, 2, 3, 0]] and out[0].tolist() == [[-9.0, -4.0, -1.0, -5.0]]
    assert out[6].tolist() == [[1, st(0, 0, 1), 0, st(0, 0, 1)]] and out[4].tolist() == [1, 2, 3, 0]
    assert out[7].tolist() == [[-1], [11], [10], [11]] and tr["wraps"] >= 1 and tr["dropped"] > 0


# ---- the command line ------------------------------------------------------------------------------------------------------------------
VOCAB = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]", "a", "dog", "fris", "##bee", "##s"]
BASE = ["--fp16", "--model_recover_path", "x.bin", "--packed_features", "p", "--beam_size", "3"]


def write(tmp_path, name, obj):
    path = tmp_path / name
    path.write_text(obj if isinstance(obj, str) else json.dumps(obj))
    return str(path)


def parse(*extra):
    from vlp_amd import decode_img2txt as D
    return D.parse_args(BASE + list(extra))


def test_word_piece_split(tmp_path):
    from vlp_amd import decode_img2txt as D
    vocab = D.Vocab(write(tmp_path, "vocab.txt", "\n".join(VOCAB) + "\n"))
    assert D.word_pieces("frisbee", vocab) == [7, 8] and D.word_pieces("frisbees", vocab) == [7, 8, 9]
    assert D.word_pieces("dog", vocab) == [6] and D.word_pieces("dogs", vocab) == [6, 9] and D.word_pieces("cat", vocab) is None
    assert D.word_pieces("bee", vocab) is None                      # only the continuation ##bee exists
    assert D.phrase_ids("a frisbee", vocab) == [5, 7, 8] and D.phrase_ids("A Dog", vocab, do_lower_case=True) == [5, 6]
    assert D.phrase_ids([6, 9], vocab) == [6, 9] and D.phrase_ids([6, 9], None) == [6, 9]
    for bad, msg in (("a cat", "without \\[UNK\\]"), ("A dog", "without \\[UNK\\]"), ("a [SEP]", "special token"), ([6, 3], "special token"),
                     ("", "empty"), ([], "empty"), ([6, 10], "outside the vocabulary"), ([6, -1], "outside the vocabulary"), (7, "string or a list"),
                     ([6, "dog"], "string or a list")):
        with pytest.raises(ValueError, match=msg):
            D.phrase_ids(bad, vocab)
    with pytest.raises(ValueError, match="needs a vocabulary"):
        D.phrase_ids("a dog", None)


def test_command_line(tmp_path):
    vocab = write(tmp_path, "vocab.txt", "\n".join(VOCAB) + "\n")
    good = write(tmp_path, "c.json", {"17": ["a frisbee", [6]], "4": []})
    a = parse("--constraints_file", good, "--vocab_file", vocab)
    assert a.constraints == {"17": [[5, 7, 8], [6]], "4": []}
    assert parse().constraints is None and parse().constraints_file is None
    ids_only = write(tmp_path, "ids.json", {"17": [[6, 9]]})
    assert parse("--constraints_file", ids_only).constraints == {"17": [[6, 9]]}          # id lists need no vocabulary
    from vlp_amd import decode_img2txt as D
    assert D.constraint_shape(a.constraints) == (2, 3) and D.constraint_shape({}) == (1, 1)
    assert D.met_list(0b10, [[5, 7, 8], [6]]) == [False, True]


@pytest.mark.parametrize("content,flags,message", [
    ({"1": ["a dog"]}, ("--beam_groups", "3"), "exclude each other"),
    ({"1": ["a dog"]}, ("--beam_size", "1"), "needs --beam_size >= 2"),
    ({"1": ["a cat"]}, (), "without [UNK]"),
    ({"1": ["a [MASK]"]}, (), "special token"),
    ({"1": [[6]] * 9}, (), "at most 8"),
    ({"1": [[6] * 9]}, (), "at most 8"),
    ({"1": "a dog"}, (), "maps an image id to a list of phrases"),
    ("{not json", (), "--constraints_file"),
])
def test_command_line_refusals(tmp_path, capsys, content, flags, message):
    vocab = write(tmp_path, "vocab.txt", "\n".join(VOCAB) + "\n")
    path = write(tmp_path, "c.json", content)
    with pytest.raises(SystemExit) as e:
        parse("--constraints_file", path, "--vocab_file", vocab, *flags)
    assert e.value.code == 2
    assert message in capsys.readouterr().err


def test_command_line_needs_a_vocabulary_for_text(tmp_path, capsys):
    path = write(tmp_path, "c.json", {"1": ["a dog"]})
    with pytest.raises(SystemExit):
        parse("--constraints_file", path)
    assert "needs a vocabulary" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        parse("--constraints_file", str(tmp_path / "missing.json"))
    assert "--constraints_file" in capsys.readouterr().err
