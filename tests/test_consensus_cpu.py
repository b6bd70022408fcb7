"""CPU: consensus selection among the K samples of an image on the host (vlp_amd.consensus) and the --select plumbing of
python -m vlp_amd.sample_img2txt.  The device kernel's twin is tests/test_87_consensus_gpu.py; tests/consensus_util.py holds what the two share.

(1) consensus_utility against scst_df_util.restated_scores in fp64 (shares no code with scst.CiderD) to 1e-9 on the cases of the GPU test,
    both tables; the fp32 restatement within bound(T, K) -- what fp32 arithmetic alone costs; the pick is the first maximum;
(2) K identical rows, K = 2, ties of select_by_logprob, the argument errors;
(3) sample_img2txt.parse_args: the four rules of --select; a table built for another caption format is refused."""
import os

import numpy as np
import pytest
import torch

from tests import consensus_util as CU
from tests import scst_df_util as U
from vlp_amd import consensus as CS
from vlp_amd import sample_img2txt as SI
from vlp_amd import scst as SC


# ---- (1) the specification ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CU.CASES, ids=CU.CASE_IDS)
@pytest.mark.parametrize("which", [0, 1], ids=["n200", "n3200000"])
def test_host_utility_against_the_restatement(case, which):
    G, T, K = case
    ids, tab, utility, pick = CU.host(case, which)
    assert utility.shape == (K * G,) and utility.dtype == np.float64 and pick.shape == (G,)
    r64 = CU.restated(ids, K, tab, np.float64)
    assert float(np.abs(r64 - utility).max()) <= 1e-9
    assert (utility.reshape(K, G).max(axis=0) > 0).all()              # every group has a non-zero utility
    r32 = CU.restated(ids, K, tab, np.float32)
    e32 = float(np.abs(r32 - utility).max())
    print("G%d T%d K%d table %d: fp32 restatement err %.3e, bound %.3e" % (G, T, K, which, e32, CU.bound(T, K)))
    assert e32 <= CU.bound(T, K), (e32, CU.bound(T, K))
    assert np.array_equal(pick, CU.first_argmax(utility, K))          # the first maximum
    CU.check_pick(pick, utility, utility, K, T)
    if which == 0 and T >= 21:                                        # the condition of the GPU test's rule (c): it is not vacuous
        sure = int(CU.decisive(utility, K, 2 * CU.bound(T, K)).sum())
        assert 2 * sure >= G, (sure, G)


def test_tensor_and_array_inputs_agree():
    ids, tab, utility, pick = CU.host((3, 5, 4), 0)
    u2, p2 = CS.consensus_utility(torch.from_numpy(np.array(ids)), 4, tab)
    assert np.array_equal(u2, utility) and np.array_equal(p2, pick)


# ---- (2) special groups and errors ------------------------------------------------------------------------------------------------------
def test_identical_rows_give_equal_utilities_and_pick_0():
    T, K = 21, 16
    row = CU.samples(1, T, 2)[0]
    ids = np.tile(row, (K, 1))
    utility, pick = CS.consensus_utility(ids, K, U.table(T, 0))
    assert utility[0] > 0 and (utility == utility[0]).all() and list(pick) == [0]
    # an image of identical rows beside one of different rows: row k*G + g
    other = CU.samples(1, T, K)
    both = np.stack([ids, other], axis=1).reshape(2 * K, T)
    u2, p2 = CS.consensus_utility(both, K, U.table(T, 0))
    assert (u2[0::2] == u2[0]).all() and abs(u2[0] - utility[0]) < 1e-12 and p2[0] == 0
    assert np.array_equal(u2[1::2], CS.consensus_utility(other, K, U.table(T, 0))[0])


def test_two_samples_score_each_other():
    G, T = 5, 21                                                      # long enough for repeated n-grams: only they make the score asymmetric
    ids, tab = CU.samples(G, T, 2), U.table(T, 0)
    utility, pick = CS.consensus_utility(ids, 2, tab)
    pair = CU.pair_host(ids, 2, tab)
    assert np.array_equal(utility[:G], pair[:, 0, 1]) and np.array_equal(utility[G:], pair[:, 1, 0])
    assert not np.array_equal(pair[:, 0, 1], pair[:, 1, 0])          # not symmetric: the clipping uses the reference's weight
    assert np.array_equal(pick, (utility[G:] > utility[:G]).astype(pick.dtype))


def test_select_by_logprob_first_maximum():
    lp = np.array([-3.0, -1.0, -2.0,      # sample 0 of images 0, 1, 2
                   -3.0, -1.0, -0.5,      # sample 1
                   -4.0, -0.5, -0.5])     # sample 2
    assert list(CS.select_by_logprob(lp, 3)) == [0, 2, 1]
    assert list(CS.select_by_logprob(torch.tensor(lp), 3)) == [0, 2, 1]
    assert list(CS.select_by_logprob([0.0, 0.0, 0.0, 0.0], 2)) == [0, 0]


def test_argument_errors():
    tab = U.table(4, 0)
    ids = CU.samples(2, 4, 3)
    for K in (1, 17, 0):
        with pytest.raises(ValueError):
            CS.consensus_utility(np.tile(ids, (6, 1))[:max(K, 1) * 2], K, tab)
        with pytest.raises(ValueError):
            CS.select_by_logprob(np.zeros(max(K, 1) * 2), K)
        with pytest.raises(ValueError):
            CS.consensus_select_device(torch.from_numpy(np.tile(ids, (6, 1))[:max(K, 1) * 2]), K, tab)
    with pytest.raises(ValueError):
        CS.consensus_utility(ids[:5], 3, tab)                         # 5 rows are not 3 samples of every image
    with pytest.raises(ValueError):
        CS.select_by_logprob(np.zeros(5), 3)
    with pytest.raises(ValueError):
        CS.consensus_select_device(torch.from_numpy(ids[:5]), 3, tab)
    for df in (None, "corpus", {}):
        with pytest.raises(TypeError):
            CS.consensus_utility(ids, 3, df)
        with pytest.raises(TypeError):
            CS.consensus_select_device(torch.from_numpy(ids), 3, df)


# ---- (3) the command line ---------------------------------------------------------------------------------------------------------------
BASE = ["--bert_model", "bert", "--model_recover_path", "m.bin", "--packed_features", "store", "--src_file", "d.json", "--fp16"]


def test_parse_args_select_rules(capsys):
    for extra, word in ((["--select", "consensus", "--num_samples", "4"], "--consensus_df"),
                        (["--consensus_df", "t.npz", "--num_samples", "4"], "--select consensus"),
                        (["--select", "logprob", "--consensus_df", "t.npz", "--num_samples", "4"], "--select consensus"),
                        (["--select", "consensus", "--consensus_df", "t.npz", "--num_samples", "1"], "--num_samples"),
                        (["--select", "logprob"], "--num_samples"),
                        (["--samples_file", "s.json", "--num_samples", "4"], "--select"),
                        (["--select", "best", "--num_samples", "4"], "invalid choice")):
        with pytest.raises(SystemExit):
            SI.parse_args(BASE + extra)
        assert word in capsys.readouterr().err, extra
    a = SI.parse_args(BASE + ["--select", "consensus", "--consensus_df", "t.npz", "--num_samples", "16", "--samples_file", "s.json"])
    assert (a.select, a.consensus_df, a.num_samples, a.samples_file) == ("consensus", "t.npz", 16, "s.json")
    a = SI.parse_args(BASE + ["--select", "logprob", "--num_samples", "2"])
    assert (a.select, a.consensus_df, a.samples_file) == ("logprob", None, None)
    # --select none parses exactly as no flag at all, and the default output path is the samples file's
    flags = ["--temperature", "0.8", "--top_k", "50", "--num_samples", "5", "--seed", "7"]
    plain, none = SI.parse_args(BASE + flags), SI.parse_args(BASE + flags + ["--select", "none"])
    assert vars(plain) == vars(none) and plain.select == "none" and plain.consensus_df is None and plain.samples_file is None
    assert SI.output_path(plain, "out/model.3.bin", 1) == "out/model.3-%s-samples.json" % plain.split
    sel = SI.parse_args(BASE + flags + ["--select", "logprob"])
    assert SI.output_path(sel, "out/model.3.bin", 1) == "out/model.3-%s-selected.json" % sel.split
    old = {k: v for k, v in vars(plain).items() if k not in ("select", "consensus_df", "samples_file")}
    assert old["num_samples"] == 5 and old["top_k"] == 50 and old["temperature"] == 0.8 and old["top_p"] == 1.0


def test_table_of_another_caption_format_is_refused(tmp_path):
    ex = [(i, [1000 + (i + j) % 12 for j in range(1 + i % 5)]) for i in range(20)]
    path = os.path.join(tmp_path, "df.npz")
    SC.DocFreq.from_examples(ex, 10, 102).save(path)
    tab = SI.consensus_doc_freq(path, 10, 102)
    assert isinstance(tab, SC.DocFreq) and tab.n_docs == 20 and (tab.max_len_b, tab.sep_id) == (10, 102)
    with pytest.raises(ValueError, match="was built for --max_len_b 10 and .SEP. id 102; this run has --max_tgt_length 20"):
        SI.consensus_doc_freq(path, 20, 102)
    with pytest.raises(ValueError, match="SEP. id 3"):
        SI.consensus_doc_freq(path, 10, 3)
    with pytest.raises(ValueError, match="there is no file"):
        SI.consensus_doc_freq(os.path.join(tmp_path, "missing.npz"), 10, 102)
    unknown = os.path.join(tmp_path, "unknown.npz")                   # a table that does not say what it was built for
    SC.DocFreq(tab.keys, tab.vals, tab.n_docs).save(unknown)
    with pytest.raises(ValueError, match="was built for"):
        SI.consensus_doc_freq(unknown, 10, 102)
