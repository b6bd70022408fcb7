"""CPU: the host side of VQA 2.0 on real data -- the answer-score rule of SparseAnswers.from_answer_ids against a brute-force leave-one-out
loop, its dense round trip, VQA examples through BatchPrefetcher, the imdb conversion and the command line of vlp_amd.eval_vqa2."""
import json
import os
import random

import numpy as np
import pytest
import torch

from vlp_amd import eval_vqa2 as E
from vlp_amd import run_img2txt_dist as R
from vlp_amd import synthetic as S
from vlp_amd.data import (BatchPrefetcher, PackedRegionStore, TextPreprocessor, batch_seed, examples_have_answers, vqa_examples_from_imdb,
                          write_packed)
from vlp_amd.input_prep import MaskSpec, SparseAnswers

NA = 3129


# ---- the score rule, written out: for every distinct answer the mean over the n leave-one-out subsets of min(1, matches / 3) ------------
def brute_force_scores(answers, unk_index=0):
    """{answer: score} by literally building the n subsets."""
    n = len(answers)
    out = {}
    for a in answers:
        if a == unk_index or a in out:
            continue
        accs = []
        for left_out in range(n):
            subset = [answers[j] for j in range(n) if j != left_out]
            matches = sum(1 for x in subset if x == a)
            accs.append(min(1.0, matches / 3))
        out[a] = sum(accs) / n
    return out


def brute_force_dense(rows, num_answers, unk_index=0):
    y = torch.zeros(len(rows), num_answers, dtype=torch.float32)
    for b, answers in enumerate(rows):
        for a, sc in brute_force_scores(answers, unk_index).items():
            y[b, a] = sc
    return y


CASES = [[5] * c + [100 + k for k in range(10 - c)] for c in range(1, 11)]             # counts 1..10 of answer 5 among 10
CASES += [[7, 7, 9, 7, 3, 9, 11, 7, 3, 2],                                             # mixed
          [4, 4, 4],                                                                   # fewer than 10 answers
          [8],                                                                         # a single answer: its only subset is empty
          [0] * 10,                                                                    # unknown only
          [0, 0, 6, 0, 6, 12, 0, 0, 0, 6],                                             # unknown among others
          [3128, 1, 3128, 1, 3128, 1, 3128, 2, 2, 2],                                  # the last index of the vocabulary
          []]                                                                          # no answers at all (a test-split question)


def test_scores_follow_the_leave_one_out_rule():
    sa = SparseAnswers.from_answer_ids(CASES)
    assert sa.idx.dtype == torch.int32 and sa.score.dtype == torch.float32 and tuple(sa.idx.shape) == tuple(sa.score.shape) == (len(CASES), 10)
    for b, answers in enumerate(CASES):
        want = brute_force_scores(answers)
        order = []
        for a in answers:                                   # distinct answers in order of first appearance, the unknown index takes no slot
            if a != 0 and a not in order:
                order.append(a)
        k = len(order)
        assert sa.idx[b, :k].tolist() == order and sa.idx[b, k:].tolist() == [-1] * (10 - k)
        assert sa.score[b, :k].tolist() == [float(np.float32(want[a])) for a in order] and sa.score[b, k:].tolist() == [0.0] * (10 - k)
    # the published table for 10 answers: 0.3, 0.6, 0.9, then 1.0
    firsts = [float(sa.score[c - 1, 0]) for c in range(1, 11)]
    assert firsts == [float(np.float32(v)) for v in (0.3, 0.6, 0.9, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0)]
    assert sa.idx[13].tolist() == [-1] * 10 and sa.idx[16].tolist() == [-1] * 10         # unknown only / nothing: every slot empty
    assert sa.idx[14].tolist()[:3] == [6, 12, -1]


def test_dense_round_trip_is_exact():
    sa = SparseAnswers.from_answer_ids(CASES)
    assert torch.equal(sa.dense(NA), brute_force_dense(CASES, NA))
    # another unknown index, a smaller vocabulary, fewer slots
    rows = [[1, 1, 0, 2], [2, 2, 2, 2], [0, 0]]
    sb = SparseAnswers.from_answer_ids(rows, unk_index=2, slots=3, num_answers=4)
    assert tuple(sb.idx.shape) == (3, 3) and torch.equal(sb.dense(4), brute_force_dense(rows, 4, unk_index=2))
    assert sb.idx[1].tolist() == [-1, -1, -1]


def test_contract_checks():
    sa = SparseAnswers.from_answer_ids(CASES)
    sa.check(len(CASES), NA)                                                            # verified by construction
    assert sa.to("cpu").verified_for == NA
    with pytest.raises(RuntimeError, match="int32"):
        sa.check(len(CASES) + 1, NA)
    with pytest.raises(RuntimeError, match="outside|-1"):
        sa.check(len(CASES), 100)                                                       # verified for 3129 answers only: the values are looked at
    dup = SparseAnswers(torch.tensor([[3, 5, 3, -1]], dtype=torch.int32), torch.zeros(1, 4))
    with pytest.raises(RuntimeError, match="distinct"):
        dup.check(1, NA)
    SparseAnswers(torch.tensor([[3, 5, -1, -1]], dtype=torch.int32), torch.zeros(1, 4)).check(1, NA)      # empty slots may repeat
    with pytest.raises(RuntimeError, match="S <= 16|1 <= S"):
        SparseAnswers(torch.zeros(1, 17, dtype=torch.int32), torch.zeros(1, 17)).check(1, NA)
    with pytest.raises(ValueError, match="outside"):
        SparseAnswers.from_answer_ids([[NA]])
    with pytest.raises(ValueError, match="distinct answers"):
        SparseAnswers.from_answer_ids([[1, 2, 3, 4]], slots=3)


# ---- loader ---------------------------------------------------------------------------------------------------------------------
def make_store(path, n=5, nv=100, seed=0):
    rng = np.random.RandomState(seed)
    ids = ["COCO_val2014_%012d" % (7 + i) for i in range(n)]
    feats = np.abs(rng.standard_normal((n, nv, 2048))).astype(np.float16)
    cls = rng.rand(n, nv, 1601).astype(np.float16)
    box = rng.rand(n, nv, 6).astype(np.float32)
    write_packed(str(path), ids, feats, cls, box)
    return PackedRegionStore(str(path)), ids


def procs(max_len_b=12):
    kw = dict(max_pred=1, mask_prob=0.0, vocab_size=2048, cls_id=S.CLS_ID, sep_id=S.SEP_ID, mask_id=S.MASK_ID, unk_id=S.UNK_ID,
              max_len=100 + max_len_b + 3, max_len_b=max_len_b, len_vis_input=100, always_truncate_tail=True)
    return TextPreprocessor(mode="s2s", **kw), TextPreprocessor(mode="bi", **kw)


def vqa_examples(ids, seed=1):
    rng = np.random.RandomState(seed)
    out = []
    for q in range(11):
        answers = CASES[(3 * q) % len(CASES)]
        out.append((ids[q % len(ids)], rng.randint(1000, 2000, size=rng.randint(3, 18)).tolist(), answers, 5000 + q))
    return out


def run_prefetcher(store, examples, workers, B=4, steps=4):
    p_s2s, p_bi = procs()
    pf = BatchPrefetcher(store, examples, B, p_s2s, p_bi, s2s_prob=0.0, device="cpu", steps=steps, seed=3, num_workers=workers)
    out = []
    for batch in pf:          # the slots are recycled: copy
        out.append([t.clone() if torch.is_tensor(t) else type(t)(*(x.clone() if torch.is_tensor(x) else x for x in t)) for t in batch])
    return pf, out


def test_prefetcher_delivers_sparse_answers(tmp_path):
    store, ids = make_store(tmp_path)
    examples = vqa_examples(ids)
    assert examples_have_answers(examples)
    pf, got = run_prefetcher(store, examples, 1)
    _, got3 = run_prefetcher(store, examples, 3)
    B = 4
    order = pf.epoch_order()
    _, p_bi = procs()
    for s, batch in enumerate(got):
        assert len(batch) == 12
        ans = batch[11]
        assert isinstance(ans, SparseAnswers) and ans.idx.dtype == torch.int32 and ans.score.dtype == torch.float32 and ans.verified_for == NA
        assert tuple(ans.idx.shape) == (B, 10)
        rng = random.Random(batch_seed(3, 0, 0, s))
        chunk = [examples[order[(s * B + j) % len(order)]] for j in range(B)]
        want = SparseAnswers.from_answer_ids([e[2] for e in chunk])
        assert torch.equal(ans.idx, want.idx) and torch.equal(ans.score, want.score)
        assert torch.equal(ans.dense(NA), brute_force_dense([e[2] for e in chunk], NA))
        for j, e in enumerate(chunk):
            rng.choices([0, 1], weights=[0.0, 1.0])                                     # the prefetcher's own draw of the preprocessor
            t = p_bi(e[1], rng)                                                         # TextPreprocessor(mode="bi") on this batch's generator
            assert batch[0][j].tolist() == t["input_ids"] and batch[1][j].tolist() == t["segment_ids"]
            assert batch[3][j].tolist() == t["masked_ids"] and batch[4][j].tolist() == t["masked_pos"]
            assert isinstance(batch[2], MaskSpec) and int(batch[2].is_s2s[j]) == 0 and int(batch[7][j]) == 0
            assert int(batch[2].second_end[j]) == 100 + t["len_b"] + 3 == batch[2].lens_host[j]
    # the same batches whatever the number of workers
    for a, b in zip(got, got3):
        for x, y in zip(a, b):
            if torch.is_tensor(x):
                assert torch.equal(x, y)
            else:
                assert all(torch.equal(u, v) if torch.is_tensor(u) else u == v for u, v in zip(x, y))


def test_caption_examples_keep_the_dummy_answer_tensor(tmp_path):
    store, ids = make_store(tmp_path)
    examples = [(e[0], e[1]) for e in vqa_examples(ids)]
    assert not examples_have_answers(examples)
    _, got = run_prefetcher(store, examples, 2, steps=2)
    for batch in got:
        assert torch.is_tensor(batch[11]) and tuple(batch[11].shape) == (4, 1) and float(batch[11].abs().max()) == 0


def test_mixed_files_and_vqa_without_answers_raise(tmp_path):
    store, ids = make_store(tmp_path / "store")
    examples = vqa_examples(ids)
    mixed = examples[:3] + [(examples[3][0], examples[3][1])]
    with pytest.raises(ValueError, match="same form"):
        BatchPrefetcher(store, mixed, 2, *procs(), device="cpu")
    tok = os.path.join(tmp_path, "captions.json")
    with open(tok, "w") as f:
        json.dump([[e[0], e[1]] for e in examples], f)
    args = R.derive_args(R.build_parser().parse_args(["--tasks", "vqa2", "--enable_butd", "--packed_features", str(tmp_path / "store"), "--token_file", tok]))
    with pytest.raises(ValueError, match=r"--tasks vqa2 needs answers.*\[image id, question token ids, answer ids"):
        R.build_packed_loader(args, "cpu")


# ---- imdb conversion ------------------------------------------------------------------------------------------------------------
def test_vqa_examples_from_imdb():
    imdb = np.array([
        {"has_answer": True, "dataset_name": "vqa2"},
        {"image_name": "COCO_val2014_000000000042", "feature_path": "COCO_val2014_000000000042.npy", "question_str": "what is this",
         "question_id": 42000, "answers": ["cat", "cat", "dog", "a cat", "cat", "cat", "cat", "kitten", "cat", "cat"]},
        {"image_name": "COCO_val2014_000000000073", "feature_path": "COCO_val2014_000000000073.npy", "question_str": "how many",
         "question_id": 73001, "answers": ["2"] * 10},
    ], dtype=object)
    words = {"what": 11, "is": 12, "this": 13, "how": 14, "many": 15}
    vocab = {"cat": 5, "dog": 9, "2": 77}

    def tokenize(q):
        return [words[w] for w in q.split()]

    def answer_index(a):
        return vocab.get(a, 0)

    got = vqa_examples_from_imdb(imdb, tokenize, answer_index)
    assert got == [["COCO_val2014_000000000042", [11, 12, 13], [5, 5, 9, 0, 5, 5, 5, 0, 5, 5], 42000],
                   ["COCO_val2014_000000000073", [14, 15], [77] * 10, 73001]]
    assert examples_have_answers(got) and json.loads(json.dumps(got)) == got           # the token file's form
    got2 = vqa_examples_from_imdb(imdb, tokenize, answer_index, store_key=lambda e: e["image_name"].split("_")[-1])
    assert [e[0] for e in got2] == ["000000000042", "000000000073"]
    test_split = np.array([{"has_answer": False}, {"image_name": "COCO_test2015_000000000001", "feature_path": "COCO_test2015_000000000001.npy",
                                                    "question_str": "how many", "question_id": 1}], dtype=object)
    assert vqa_examples_from_imdb(test_split, tokenize, answer_index) == [["COCO_test2015_000000000001", [14, 15], [], 1]]


# ---- command line ---------------------------------------------------------------------------------------------------------------
# the reference script's flags and defaults (vlp/eval_vqa2.py:57-109)
REFERENCE_FLAGS = {
    "bert_model": "bert-base-cased", "model_recover_path": None, "fp16": False, "amp": False, "seed": 123, "do_lower_case": False,
    "new_segment_ids": False, "batch_size": 4, "beam_size": 1, "length_penalty": 0, "forbid_duplicate_ngrams": False, "forbid_ignore_word": None,
    "min_len": None, "ngram_size": 3, "max_tgt_length": 20, "src_file": "/mnt/dat/COCO/annotations/dataset_coco.json",
    "ref_file": "pythia/data/v2_mscoco_val2014_annotations.json", "dataset": "coco", "len_vis_input": 100, "image_root": "/mnt/dat/COCO/images",
    "split": "val", "drop_prob": 0.1, "enable_butd": False,
    "region_bbox_file": "coco_detection_vg_thresh0.2_feat_gvd_checkpoint_trainvaltest.h5",
    "region_det_file_prefix": "feat_cls_1000/coco_detection_vg_100dets_gvd_checkpoint_trainval", "output_dir": "tmp", "file_valid_jpgs": "",
}


def test_flags_and_defaults_match_the_reference():
    ours = {a.dest: a.default for a in E.build_parser()._actions if a.dest != "help"}
    for name, default in REFERENCE_FLAGS.items():
        assert name in ours, name
        assert ours[name] == default and type(ours[name]) is type(default), (name, ours[name], default)
    assert set(ours) - set(REFERENCE_FLAGS) == {"packed_features", "token_file", "answer_vocab_file", "output_file", "config_path", "num_hidden_layers"}


def test_main_needs_fp16_a_packed_store_and_a_token_file(tmp_path):
    with pytest.raises(NotImplementedError, match="--fp16"):
        E.main(["--enable_butd", "--packed_features", str(tmp_path), "--token_file", "x", "--model_recover_path", "x"])
    with pytest.raises(NotImplementedError, match="--amp only engages"):
        E.main(["--enable_butd", "--amp", "--packed_features", str(tmp_path), "--token_file", "x", "--model_recover_path", "x"])
    with pytest.raises(NotImplementedError, match="--packed_features"):
        E.main(["--enable_butd", "--fp16", "--token_file", "x", "--model_recover_path", "x"])
    with pytest.raises(NotImplementedError, match="--token_file"):
        E.main(["--enable_butd", "--fp16", "--packed_features", str(tmp_path), "--model_recover_path", "x"])


def test_question_files_and_output_paths(tmp_path):
    tok = os.path.join(tmp_path, "captions.json")
    with open(tok, "w") as f:
        json.dump([["img", [1, 2, 3]]], f)
    with pytest.raises(ValueError, match="caption examples"):
        E.load_questions(tok)
    with open(tok, "w") as f:
        json.dump([["img", [1, 2, 3], [4] * 10, 9]], f)
    assert E.load_questions(tok) == [("img", [1, 2, 3], [4] * 10, 9)]
    voc = os.path.join(tmp_path, "answers.txt")
    with open(voc, "w") as f:
        f.write("<unk>\nyes\nno\n\n")
    assert E.load_answer_vocab(voc) == ["<unk>", "yes", "no"]
    args = E.build_parser().parse_args(["--split", "minival"])
    assert E.output_path(args, "/x/model.30.bin", 1) == "/x/model.30-minival-vqa2.json"
    args.output_file = "/y/out.json"
    assert E.output_path(args, "/x/model.30.bin", 1) == "/y/out.json" and E.output_path(args, "/x/model.30.bin", 2) == "/y/out.model.30.json"
    # the preprocessor of eval_vqa2.py:138-144: bidirectional, nothing masked, the tail is cut
    args = E.build_parser().parse_args(["--max_tgt_length", "5", "--new_segment_ids"])
    t = E.question_preprocessor(args)(list(range(1000, 1009)))
    assert t["input_ids"] == [S.CLS_ID] + [S.UNK_ID] * 100 + [S.SEP_ID] + list(range(1000, 1005)) + [S.SEP_ID]
    assert t["segment_ids"] == [0] * 102 + [1] * 6 and t["masked_pos"] == [] and not t["is_s2s"] and t["len_b"] == 5
