"""CPU: the host side of scoring given captions -- the counting rule (vlp_amd.caption_score), the arithmetic of records, summary and
selection, key filtering by split, the parser errors of python -m vlp_amd.score_img2txt, the C layout of vlp_token_score's arguments and
the torch restatement of its integer outputs that the GPU test compares the kernel with."""
import math
import os
import subprocess

import pytest
import torch

from tests import caption_score_util as U
from vlp_amd import caption_score as CS

SEP = 102


# ---- counting rule ---------------------------------------------------------------------------------------------------------
def test_counting_rule_hand_written():
    T = 5
    caps = [[7], [7, 8, 9], [1, 2, 3, 4], [1, 2, 3, 4, 5], [1, 2, 3, 4, 5, 6, 7, 8, 9], []]
    ids, counted, trunc = CS.counted_positions(caps, T, SEP)
    assert ids.tolist() == [[7, SEP, -1, -1, -1], [7, 8, 9, SEP, -1], [1, 2, 3, 4, SEP], [1, 2, 3, 4, 5], [1, 2, 3, 4, 5], [SEP, -1, -1, -1, -1]]
    assert counted.sum(1).tolist() == [2, 4, 5, 5, 5, 1]
    assert torch.equal(counted, ids >= 0) and counted.dtype == torch.bool and ids.dtype == torch.long
    assert trunc.tolist() == [False, False, False, True, True, False]          # n >= T: cut, no [SEP] counted
    assert [CS.is_truncated(len(c), T) for c in caps] == trunc.tolist()


def test_counting_rule_padded_tensor_with_lengths_and_refusals():
    T = 4
    padded = torch.tensor([[5, 6, 0, 0, 0, 0], [5, 6, 7, 8, 9, 10], [3, 0, 0, 0, 0, 0]])
    ids, counted, trunc = CS.counted_positions(padded, T, SEP, lengths=torch.tensor([2, 6, 0]))
    assert ids.tolist() == [[5, 6, SEP, -1], [5, 6, 7, 8], [SEP, -1, -1, -1]] and trunc.tolist() == [False, True, False]
    ids2, _, trunc2 = CS.counted_positions(padded[:, :3], T, SEP)                   # no lengths: every column is a token
    assert ids2.tolist() == [[5, 6, 0, SEP], [5, 6, 7, SEP], [3, 0, 0, SEP]] and not trunc2.any()
    with pytest.raises(ValueError, match="outside the vocabulary"):
        CS.counted_positions([[1, -1]], T, SEP)
    with pytest.raises(ValueError, match="outside the vocabulary"):
        CS.counted_positions([[1, 50]], T, SEP, vocab_size=50)
    CS.counted_positions([[1, 2, 3, 4, 50]], T, SEP, vocab_size=50)                 # behind the cut: never fed, not checked
    with pytest.raises(ValueError, match="lengths"):
        CS.counted_positions(padded, T, SEP, lengths=[1, 2])
    with pytest.raises(ValueError, match="length 7"):
        CS.counted_positions(padded, T, SEP, lengths=[1, 7, 0])
    with pytest.raises(ValueError, match="output positions"):
        CS.counted_positions([[1]], 0, SEP)


# ---- records, summary, selection ---------------------------------------------------------------------------------------------
def test_record_and_summary_arithmetic():
    counted = [True, True, True, False, False]
    logp = torch.tensor([-0.5, -2.0, -0.25, 0.0, 0.0])
    ent = torch.tensor([1.0, 3.0, 0.5, 0.0, 0.0])
    rank = torch.tensor([0, 4, 7, -1, -1], dtype=torch.int32)
    r = CS.caption_record(logp, ent, rank, counted)
    assert r["tokens"] == 3 and r["top1"] == 1 and r["top5"] == 2 and type(r["tokens"]) is int and type(r["top1"]) is int
    assert r["logprob"] == -2.75 and r["entropy"] == 1.5 and r["ppl"] == math.exp(2.75 / 3)
    r2 = CS.caption_record([-1.0, 0, 0, 0, 0], [2.0, 0, 0, 0, 0], [0, -1, -1, -1, -1], [True, False, False, False, False])
    s = CS.summarize([r, r2])
    assert s["captions"] == 2 and s["tokens"] == 4 and s["logprob"] == -3.75 and s["ppl"] == math.exp(3.75 / 4)
    assert s["top1"] == 0.5 and s["top5"] == 0.75 and s["top5"] >= s["top1"]
    assert abs(s["entropy"] - (4.5 + 2.0) / 4) < 1e-15
    # fp64 on the host: 2^-30 is lost against 1024 in fp32 and kept here
    r3 = CS.caption_record(torch.tensor([-1024.0, -2.0 ** -30]), [0.0, 0.0], [0, 0], [True, True])
    assert r3["logprob"] == -1024.0 - 2.0 ** -30
    empty = CS.summarize([])
    assert empty == {"captions": 0, "tokens": 0, "logprob": 0.0, "ppl": None, "top1": None, "top5": None, "entropy": None}
    assert CS.perplexity(-1e6, 1) == float("inf") and CS.perplexity(0.0, 0) is None


def _rec(image_id, index, logprob, tokens):
    return {"image_id": image_id, "index": index, "logprob": logprob, "tokens": tokens, "caption": "c%s_%d" % (image_id, index)}


def test_selection_ties_and_length_norm():
    recs = [_rec(9, 0, -4.0, 2), _rec(3, 0, -6.0, 3), _rec(9, 1, -4.0, 4), _rec(3, 1, -5.0, 2), _rec(9, 2, -9.0, 9), _rec(3, 2, -5.0, 2)]
    none = CS.select_likelihood(recs, "none")
    assert [(r["image_id"], r["index"]) for r in none] == [(9, 0), (3, 1)]          # image order of first occurrence; ties to the lowest index
    mean = CS.select_likelihood(recs, "mean")
    assert [(r["image_id"], r["index"]) for r in mean] == [(9, 1), (3, 0)]          # -1 < -2 per token;  -2 > -2.5
    assert all(set(r) == {"image_id", "caption", "index", "logprob"} for r in none + mean)
    assert mean[0]["logprob"] == -4.0 and mean[0]["caption"] == "c9_1"              # the total stays what is written
    tie = CS.select_likelihood([_rec(1, 0, -4.0, 4), _rec(1, 1, -2.0, 2)], "mean")
    assert tie[0]["index"] == 0
    with pytest.raises(ValueError, match="length_norm"):
        CS.select_likelihood(recs, "sum")
    assert CS.caption_indices([9, 3, 9, 3, 9, 3, 4]) == [0, 0, 1, 1, 2, 2, 0]


def test_key_filtering_by_split():
    from vlp_amd.decode_img2txt import select_images
    img_dat = [{"split": sp, "filename": U.fname(i)} for sp, i in U.LIST]
    images = select_images(img_dat, "val", "coco")
    ex = [(U.fname(i)[:-4], [n, n + 1]) for n, (_, i) in enumerate(U.LIST)] + [(U.fname(522418)[:-4], [50])]
    kept = CS.filter_examples(ex, images)
    assert kept == [(522418, U.fname(522418)[:-4], [1, 2]), (554625, U.fname(554625)[:-4], [4, 5]), (522418, U.fname(522418)[:-4], [50])]
    every = CS.filter_examples(ex)
    assert len(every) == len(ex) and all(a == b for a, b, _ in every)                # without a split the key is the id
    assert CS.filter_examples([(391895, [1])], [(7, "391895")]) == [(7, 391895, [1])]    # an integer key names the store row "391895"


# ---- the tool's parser -----------------------------------------------------------------------------------------------------------
BASE = ["--bert_model", "dir", "--model_recover_path", "m.bin", "--packed_features", "store", "--token_file", "t.json", "--fp16"]


def _without(flag, n=2):
    i = BASE.index(flag)
    return BASE[:i] + BASE[i + n:]


@pytest.mark.parametrize("argv,message", [
    (_without("--fp16", 1), "add --fp16"),
    (_without("--packed_features"), "--packed_features DIR is required"),
    (_without("--token_file"), "--token_file FILE is required"),
    (BASE + ["--length_norm", "mean"], "--length_norm mean says how --select likelihood compares"),
    (BASE + ["--samples_file", "s.json"], "--samples_file s.json receives the per-caption records"),
    (BASE + ["--split", "val"], "--src_file and --split go together"),
    (BASE + ["--select", "logprob"], "invalid choice"),
])
def test_parser_errors(argv, message, capsys):
    from vlp_amd import score_img2txt as SI
    with pytest.raises(SystemExit) as e:
        SI.parse_args(argv)
    assert e.value.code == 2
    assert message in capsys.readouterr().err


def test_parser_accepts_and_token_file_kinds(tmp_path):
    import json
    from vlp_amd import score_img2txt as SI
    a = SI.parse_args(BASE)
    assert (a.select, a.length_norm, a.src_file, a.split, a.max_tgt_length, a.batch_size) == ("none", "none", None, None, 20, 4)
    a = SI.parse_args(BASE + ["--select", "likelihood", "--length_norm", "mean", "--samples_file", "s.json", "--src_file", "d.json", "--split", "val"])
    assert (a.select, a.length_norm, a.samples_file, a.split) == ("likelihood", "mean", "s.json", "val")
    vqa = os.path.join(tmp_path, "vqa.json")
    json.dump([["k", [1, 2], [3], 11]], open(vqa, "w"))
    with pytest.raises(ValueError, match="holds VQA examples"):
        SI.load_captions(SI.parse_args(_without("--token_file") + ["--token_file", vqa]))
    none = os.path.join(tmp_path, "none.json")
    json.dump([], open(none, "w"))
    with pytest.raises(ValueError, match="holds no examples"):
        SI.load_captions(SI.parse_args(_without("--token_file") + ["--token_file", none]))
    cap = os.path.join(tmp_path, "cap.json")
    json.dump([["k", [1, 2]], [5, [3]]], open(cap, "w"))
    assert SI.load_captions(SI.parse_args(_without("--token_file") + ["--token_file", cap])) == [("k", "k", [1, 2]), (5, 5, [3])]


# ---- the kernel's interface and the test's own reference -----------------------------------------------------------------------
def test_token_score_struct_matches_c_layout_and_is_registered(tmp_path):
    import ctypes
    from vlp_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    st = _lib.TokenScoreArgs
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "vlp_hip.h"', "int main(void) {",
             'printf("%zu", sizeof(vlp_token_score_args));']
    lines += ['printf(" %%zu", offsetof(vlp_token_score_args, %s));' % f for f, _ in st._fields_]
    lines.append("return 0; }")
    src, exe = os.path.join(tmp_path, "layout.c"), os.path.join(tmp_path, "layout")
    open(src, "w").write("\n".join(lines))
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(root, "include"), src, "-o", exe])
    out = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert out[0] == ctypes.sizeof(st)
    assert out[1:] == [getattr(st, f).offset for f, _ in st._fields_]
    assert "vlp_token_score" in _lib.SYMBOLS
    assert hasattr(_lib.load(), "vlp_token_score")                                    # compiled into the one product library


def test_rank_top_reference_on_hand_rows():
    x = torch.tensor([[1.0, 3.0, 3.0, 2.0, 3.0], [2.0, 2.0, 2.0, 2.0, 2.0], [0.0, -1.0, 5.0, 5.0, -2.0]]).half()
    rank, top_id, top = U.rank_top_reference(x, torch.tensor([2, 3, 9]))                # the last id is clamped to 4
    assert rank.tolist() == [1, 3, 4] and top_id.tolist() == [1, 0, 2] and top.tolist() == [3.0, 2.0, 5.0]
    rank, top_id, _ = U.rank_top_reference(x, torch.tensor([1, 0, 2]))
    assert rank.tolist() == [0, 0, 0] and top_id.tolist() == [1, 0, 2]                  # rank == 0 exactly when top_id == id
    for name, (row, id, want_rank, want_top) in U.hard_score_rows(1000).items():
        rank, top_id, _ = U.rank_top_reference(row.view(1, -1), torch.tensor([id]))
        assert want_rank is None or int(rank) == want_rank, name
        assert want_top is None or int(top_id) == want_top, name
        assert (int(rank) == 0) == (int(top_id) == id), name


def test_tool_token_examples_cover_the_cases():
    ex = U.token_examples([391895, 184613, 318219, 574769, 60623], {0, 100, 101, 102, 103})
    assert len(ex) == 13 and len(ex) % 2 == 1 and len(ex) % 3 == 1                     # batches of 2 and of 3 both end short
    keys = [k for k, _ in ex]
    per = {k: keys.count(k) for k in keys}
    assert sorted(per.values()) == [2, 2, 3, 3, 3]
    assert keys[-1] == keys[0] and keys[-2] != keys[0]                                  # one key repeated non-adjacently
    assert sum(len(t) >= U.T for _, t in ex) == 1 and max(len(t) for _, t in ex) > U.T  # one caption is cut
