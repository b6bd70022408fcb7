"""CPU: the host restatement of temperature / top-k / top-p sampling (tests/sample_filter_util.py) against a sort-based brute force, the
threshold grid's margin condition, the command line of vlp_amd.sample_img2txt, and the C declaration of vlp_sample_rows_filtered."""
import os
import subprocess

import numpy as np
import pytest

from tests import sample_filter_util as U
from vlp_amd import decode_img2txt as D
from vlp_amd import sample_img2txt as SI

PARAMS = [(T, k, p) for T in (0.5, 1.0, 2.0) for k in (0, 1, 2, 3, 5, 11, 12, 40) for p in (1.0, 0.9, 0.5, 0.3, 0.05)]


def small_rows():
    rng = np.random.RandomState(3)
    rows = [rng.randn(12).astype(np.float16) * np.float16(2),
            np.round(rng.randn(12) * 2).astype(np.float16) / np.float16(2),                     # coarse values: many ties
            np.array([1, 3, 3, 3, 0, -1, 2, 2, 3, -2, 0, 1], dtype=np.float16),                  # four equal maxima
            np.array([0.5] * 12, dtype=np.float16),                                            # one value
            np.array([-np.inf, 1.5, -np.inf, -np.inf, 0.25, -np.inf, -np.inf, -np.inf, -np.inf, -np.inf, -np.inf, -np.inf], dtype=np.float16),
            np.array([0.0, -0.0, 1.0, -1.0, 0.0, -0.0, 2.0, -np.inf, 0.0, 1.0, -0.0, 0.5], dtype=np.float16),     # -0 and +0 are one value
            np.array([4.0], dtype=np.float16)]
    return rows


@pytest.mark.parametrize("T,top_k,top_p", PARAMS)
def test_restatement_equals_the_sort_based_definition(T, top_k, top_p):
    for row in small_rows():
        V = row.shape[0]
        r = U.filter_reference(row, T, top_k, top_p)
        S = U.brute_force_set(row, T, top_k, top_p)
        assert np.array_equal(r["S"], S), (row, r["S"], S)
        l = row.astype(np.float64)
        assert r["kept"] == int(S.sum()) >= 1 and r["cutoff"] == l[S].min() and S[int(np.argmax(l))]
        assert np.array_equal(S, l >= r["cutoff"])                                              # a pure value threshold
        if top_k == 0 or top_k >= V:
            if top_p == 1.0:
                assert S.all() and r["margin"] == float("inf")
        else:
            assert r["kept"] >= min(top_k, V) or top_p < 1.0                                    # ties at the threshold are kept
        z = l[S] / float(np.float32(T))
        want = z - (z.max() + np.log(np.exp(z - z.max()).sum()))
        assert np.allclose(r["logp"][S], want, rtol=0, atol=1e-12) and np.all(np.isneginf(r["logp"][~S]))
        assert abs(r["probs"].sum() - 1.0) < 1e-12 and np.all(r["probs"][~S] == 0) and np.all(r["probs"][np.isneginf(l)] == 0)


def test_top_k_keeps_ties_and_top_p_takes_whole_groups():
    row = np.array([1, 3, 3, 3, 0, -1, 2, 2], dtype=np.float16)
    r = U.filter_reference(row, 1.0, 1, 1.0)
    assert r["kept"] == 3 and r["cutoff"] == 3.0 and np.allclose(r["logp"][[1, 2, 3]], -np.log(3.0))
    r = U.filter_reference(row, 1.0, 4, 1.0)                       # the 4th largest is a 2: both 2s stay
    assert r["kept"] == 5 and r["cutoff"] == 2.0
    e = np.exp(row.astype(np.float64) - 3.0)
    m3 = 3 * e[1] / e.sum()
    r = U.filter_reference(row, 1.0, 0, m3 * 0.999)                  # the three 3s suffice
    assert r["kept"] == 3 and abs(r["margin"] - (m3 - np.float32(m3 * 0.999)) / np.float32(m3 * 0.999)) < 1e-9
    r = U.filter_reference(row, 1.0, 0, m3 * 1.001)                  # they do not: the 2s come in, both
    assert r["kept"] == 5 and r["cutoff"] == 2.0
    r = U.filter_reference(row, 1.0, 0, 1.0)
    assert r["kept"] == 8 and r["cutoff"] == -1.0
    assert U.filter_reference(row, 1.0, 8, 1.0)["kept"] == 8 and U.filter_reference(row, 1.0, 13, 1.0)["kept"] == 8       # top_k >= V: off


def test_threshold_grid_margins_hold_on_the_host_reference_alone():
    """The grid of tests/test_43_sample_filter_gpu.py: with the base seed at most 1 case in 10 needs other rows to reach MARGIN_MIN, and every
    case reaches it.  The counts under the 1e-3 first asked for are printed: that margin is out of reach of these rows (sample_filter_util.py)."""
    total = regenerated = under_asked = 0
    for V in U.GRID_V:
        cases = U.grid_cases(V)
        assert len(cases) == len(U.GRID_T) * 7 * len(U.GRID_TOP_P)
        n_re = sum(c["regenerated"] for c in cases)
        base = [U.RowRef(x) for x in U.random_rows(U.GRID_BASE_SEED + V, U.GRID_ROWS, V)]
        n_asked = sum(min(r.filter(c["T"], c["top_k"], c["top_p"])["margin"] for r in base) < U.MARGIN_ASKED for c in cases)
        print("V=%d: %d cases, %d regenerated for a margin of %g, %d under a margin of %g with the base rows" %
              (V, len(cases), n_re, U.MARGIN_MIN, n_asked, U.MARGIN_ASKED))
        assert all(min(r["margin"] for r in c["refs"]) >= U.MARGIN_MIN for c in cases)
        total, regenerated, under_asked = total + len(cases), regenerated + n_re, under_asked + n_asked
    print("all: %d cases, %d regenerated, %d under %g" % (total, regenerated, under_asked, U.MARGIN_ASKED))
    assert regenerated * 10 <= total, (regenerated, total)


# ---- the command line ---------------------------------------------------------------------------------------------------
def test_parser_adds_four_flags_and_leaves_the_decode_parser_alone():
    ours = {a.dest: a.default for a in SI.build_parser()._actions if a.dest != "help"}
    base = {a.dest: a.default for a in D.build_parser()._actions if a.dest != "help"}
    new = {"temperature": 1.0, "top_k": 0, "top_p": 1.0, "num_samples": 1}
    assert not set(base) & set(new)                                   # decode_img2txt's parser has not gained a destination
    assert ours == dict(base, **new)
    assert all(type(ours[k]) is type(v) for k, v in new.items())
    a = SI.parse_args(["--temperature", "0.7", "--top_k", "50", "--top_p", "0.9", "--num_samples", "5", "--batch_size", "64", "--seed", "9"])
    assert (a.temperature, a.top_k, a.top_p, a.num_samples, a.batch_size, a.seed, a.beam_size) == (0.7, 50, 0.9, 5, 64, 9, 1)
    a = SI.parse_args(["--num_samples", "16", "--batch_size", "64"])      # 1024 sequences: the limit itself
    assert a.num_samples * a.batch_size == 1024


@pytest.mark.parametrize("argv,word", [
    (["--temperature", "0"], "--temperature"), (["--temperature", "-1"], "--temperature"), (["--temperature", "inf"], "--temperature"),
    (["--temperature", "nan"], "--temperature"), (["--top_k", "-1"], "--top_k"), (["--top_p", "0"], "--top_p"), (["--top_p", "1.01"], "--top_p"),
    (["--top_p", "nan"], "--top_p"), (["--num_samples", "0"], "--num_samples"), (["--num_samples", "17"], "--num_samples"),
    (["--beam_size", "3"], "decode_img2txt"), (["--forbid_duplicate_ngrams"], "decode_img2txt"),
    (["--batch_size", "65", "--num_samples", "16"], "1040 sequences"), (["--batch_size", "0"], "sequences")])
def test_parser_refuses(argv, word, capsys):
    with pytest.raises(SystemExit) as e:
        SI.parse_args(argv)
    assert e.value.code == 2
    assert word in capsys.readouterr().err


def test_sequence_logprob_stops_after_the_first_sep():
    assert SI.sequence_logprob([5, 6, 102, 7, 102], [-1.0, -2.0, -0.5, -9.0, -9.0], 102) == -3.5
    assert SI.sequence_logprob([5, 6, 7], [-1.0, -2.0, -0.25], 102) == -3.25
    assert SI.sequence_logprob([102, 6], [-0.125, -2.0], 102) == -0.125


# ---- the C ABI ----------------------------------------------------------------------------------------------------------
def test_declaration_compiles_as_c_and_is_bound(tmp_path):
    import ctypes
    from vlp_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = os.path.join(tmp_path, "decl.c")
    with open(src, "w") as f:
        f.write('#include <stdio.h>\n#include "vlp_hip.h"\n'
                "typedef int (*fn_t)(const void*, int64_t, int32_t, int32_t, int32_t, const uint64_t*, uint64_t, uint32_t, float, int32_t, float,\n"
                "                    int64_t*, int64_t, int64_t*, int64_t, float*, int64_t, float*, int32_t*, void*);\n"
                "fn_t entry = vlp_sample_rows_filtered;\n"              # an incompatible declaration is a compile error
                'int main(void) { printf("%d\\n", entry != 0); return 0; }\n')
    obj = os.path.join(tmp_path, "decl.o")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(root, "include"), "-c", src, "-o", obj])
    res, args = _lib.SYMBOLS["vlp_sample_rows_filtered"]
    assert res is ctypes.c_int and len(args) == 20
    assert args[8] is ctypes.c_float and args[9] is ctypes.c_int32 and args[10] is ctypes.c_float
    assert callable(_lib.sample_rows_filtered)
