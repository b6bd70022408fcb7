"""CPU: the caption metrics on the host (vlp_amd/caption_metrics.py, DocFreq.from_token_lists, python -m vlp_amd.eval_captions --metrics_on host).

The metrics are written from the published definitions; what is checked here is the pinned example, each class against a restatement that
shares no code with it, the degenerate rules, the invariances, the tokenisation rule and the command-line tool with its errors."""
import json
import os
from collections import Counter

import numpy as np
import pytest

from tests import caption_eval_util as CU
from vlp_amd import caption_metrics as CM
from vlp_amd import eval_captions as EC
from vlp_amd import scst as SC


def test_pinned_example():
    b, r = SC.Bleu(), CM.Rouge()
    h, refs = "the cat sat on the mat", ["the cat is on the mat", "there is a cat on the mat"]
    correct, len_h, reflen = b.sentence_stats(h, refs)
    assert (tuple(correct), len_h, reflen) == ((5, 3, 1, 0), 6, 6)
    assert r.sentence_lcs(h.split(), [x.split() for x in refs]) == [(5, 6), (4, 7)]
    assert abs(r.sentence_score(h.split(), [x.split() for x in refs]) - 5.0 / 6.0) < 1e-15
    assert abs(r.compute_score({0: refs}, {0: [h]})[0] - 5.0 / 6.0) < 1e-15
    correct, len_h, reflen = b.sentence_stats("a b c d", ["a b d c"])
    assert (tuple(correct), len_h, reflen) == ((4, 1, 0, 0), 4, 4)
    assert CM.lcs_len("a b c d".split(), "a b d c".split()) == 3


def test_rouge_against_brute_force_lcs():
    rng = np.random.RandomState(0)
    r = CM.Rouge()
    nonzero = 0
    for case in range(200):
        vocab = (1, 2, 3, 12)[case % 4]
        h = rng.randint(0, vocab, size=rng.randint(0, 30)).tolist()
        refs = [rng.randint(0, vocab, size=rng.randint(0, 30)).tolist() for _ in range(rng.randint(1, 4))]
        pairs = [(CU.brute_lcs(h, x), len(x)) for x in refs]
        assert r.sentence_lcs(h, refs) == pairs
        prec = max([l / len(h) for l, n in pairs if len(h) and n] or [0.0])
        rec = max([l / n for l, n in pairs if len(h) and n] or [0.0])
        want = (1 + 1.44) * prec * rec / (rec + 1.44 * prec) if prec > 0 and rec > 0 else 0.0
        got = r.sentence_score(h, refs)
        assert abs(got - want) <= 1e-15, (case, got, want)
        nonzero += got > 0
    assert nonzero >= 150


def test_degenerate_rules():
    r = CM.Rouge()
    assert r.sentence_score([], [["a", "b"]]) == 0.0                         # an empty hypothesis
    assert r.sentence_score(["a"], [[]]) == 0.0                              # an empty reference: precision 0, recall 0
    assert r.sentence_score(["a", "b"], [[], ["a", "b"]]) == 1.0             # ... next to a normal one it changes nothing
    assert r.sentence_score(["a"], [["b"]]) == 0.0
    m = CM.CaptionMetrics()
    one = m.score([[["a", "b", "c"], ["a", "c"]]], [["a", "b", "c"]])
    assert one["CIDEr"] == 0.0 and one["images"] == 1                        # one document: every idf is log(1) - log(1)
    assert one["ROUGE_L"] == 1.0 and abs(one["Bleu_4"] - (1e-15 / 1e-9) ** 0.25) < 1e-9       # no 4-gram to guess; the other factors are 1 - O(1e-9)
    assert abs(one["Bleu_3"] - 1.0) < 1e-8
    empty = m.score([[["a", "b"]], [["c"]]], [[], ["c"]])
    assert empty["per_image"]["ROUGE_L"].tolist() == [0.0, 1.0] and empty["per_image"]["CIDEr"][0] == 0.0
    assert empty["per_image"]["bleu_stats"][0].tolist() == [0, 0, 0, 0, 0, 2]


def _restated_corpus_bleu(stats):
    c = np.array(stats, dtype=np.float64)
    out, p = [], 1.0
    for k in range(4):
        guess = sum(max(0, int(s[4]) - k) for s in stats)
        p *= (c[:, k].sum() + 1e-15) / (guess + 1e-9)
        out.append(p ** (1.0 / (k + 1)))
    ratio = (c[:, 4].sum() + 1e-15) / (c[:, 5].sum() + 1e-9)
    return [v * (np.exp(1 - 1 / ratio) if ratio < 1 else 1.0) for v in out]


def test_corpus_bleu_against_a_restatement_and_the_brevity_penalty():
    hyp, ref, count = CU.make_corpus(64, 5, 21, 0)
    stats, _, _ = CU.host_counts(hyp, ref, count)
    got = CM.corpus_bleu(stats)
    want = _restated_corpus_bleu(stats.tolist())
    assert np.abs(got - want).max() <= 1e-15 and 0 < got[3] < got[0] < 1
    # short hypotheses: every one a prefix of its reference, half as long
    refs = [[list("abcdefghij")], [list("klmnopqr")]]
    hyps = [list("abcde"), list("klmn")]
    b = SC.Bleu()
    st = [list(c) + [lh, rl] for c, lh, rl in (b.sentence_stats(" ".join(h), [" ".join(r[0])]) for h, r in zip(hyps, refs))]
    assert [s[4:] for s in st] == [[5, 10], [4, 8]]
    short = CM.corpus_bleu(st)
    assert np.abs(short - np.exp(1 - 18.0 / 9.0)).max() < 1e-8                # precision 1 at every order, ratio 9 / 18
    assert np.abs(CM.corpus_bleu([s[:5] + [s[4]] for s in st]) - 1.0).max() < 1e-8


def test_doc_freq_from_token_lists():
    docs = [[[5, 6, 5, 6], [5, 6]], [[6, 5], []], [[]], [[65534, 1, 65534]]]
    tab = SC.DocFreq.from_token_lists(docs)
    want = Counter()
    for d in docs:
        seen = set()
        for s in d:
            seen.update(CU.U.grams_of(s))
        want.update(seen)
    assert tab.n_docs == 4 and len(tab) == len(want)
    for gram, df in want.items():
        assert tab.get(gram) == df, gram
    assert tab.get((5, 6)) == 1 and tab.get((5,)) == 2 and tab.get((6, 5)) == 2      # (5, 6) twice in one image counts once
    # no key holds a field of id 0 (1 after the +1): a word string has no 0
    fields = np.stack([(tab.keys >> np.uint64(s)) & np.uint64(0xffff) for s in (48, 32, 16, 0)], 1)
    assert not (fields == 1).any() and tab.get((0,)) == 0
    for bad in ([[[0, 5]]], [[[65535]]], [[[-1]]]):
        with pytest.raises(ValueError):
            SC.DocFreq.from_token_lists(bad)
    assert len(SC.DocFreq.from_token_lists([[[]], [[]]])) == 0
    # chunking never splits an image
    many = [[[int(t) for t in np.random.RandomState(i).randint(1, 9, size=6)] for _ in range(3)] for i in range(37)]
    a, b = SC.DocFreq.from_token_lists(many), SC.DocFreq.from_token_lists(many, chunk=5)
    assert np.array_equal(a.keys, b.keys) and np.array_equal(a.vals, b.vals)


def test_caption_metrics_host_invariances():
    G, R, T = 40, 4, 21
    hyp, ref, count = CU.make_corpus(G, R, T, 0)
    m = CM.CaptionMetrics()
    base = m.score_rows(hyp, ref, count)
    assert base["scored_on_host"] == 0 and 0 < base["Bleu_4"] < base["Bleu_1"] < 1 and 0 < base["ROUGE_L"] < 1 and base["CIDEr"] > 0
    # df over the evaluated images: the per-image CIDEr of the class with that table
    refs, hyps = CU.word_lists(hyp, ref, count)
    tab = SC.DocFreq.from_token_lists(refs)
    assert np.array_equal(base["per_image"]["CIDEr"], CU.host_cider(hyp, ref, count, tab))
    perm = np.random.RandomState(1).permutation(G)
    p = m.score_rows(hyp[perm], ref[perm], count[perm])
    for k in CM.METRICS[:4]:
        assert p[k] == base[k]                                                # integer sums
    assert abs(p["ROUGE_L"] - base["ROUGE_L"]) < 1e-14 and abs(p["CIDEr"] - base["CIDEr"]) < 1e-12
    assert np.array_equal(p["per_image"]["bleu_stats"], base["per_image"]["bleu_stats"][perm])
    assert np.array_equal(p["per_image"]["ROUGE_L"], base["per_image"]["ROUGE_L"][perm])
    assert np.abs(p["per_image"]["CIDEr"] - base["per_image"]["CIDEr"][perm]).max() < 1e-12
    # garbage behind a row's first 0 and in the invalid reference rows
    h2, r2 = hyp.copy(), ref.copy()
    changed = 0
    for rows in (h2, r2.reshape(G * R, T)):
        for row in rows:
            z = np.flatnonzero(row == 0)
            if len(z) and z[0] + 1 < T:
                row[z[0] + 1:] = 1005
                changed += 1
    for g in range(G):
        r2[g, count[g]:] = 1007
    assert changed > G
    q = m.score_rows(h2, r2, count)
    for k in CM.METRICS:
        assert q[k] == base[k]
    with pytest.raises(ValueError):
        m.score([[["a"]]], [["a"]], on="gpu")
    with pytest.raises(ValueError):
        m.score([[]], [["a"]])


def test_punctuation_rule():
    assert CM.tokenize_caption("A man , with a  DOG . -LRB- red -rrb- ball ; it's `` fun '' ... ! ? : - --") == ["a", "man", "with", "a", "dog", "red", "ball", "it's", "fun"]
    assert CM.tokenize_caption("") == [] and CM.tokenize_caption(" . ") == []
    assert len(CM.PUNCTUATIONS) == 17


def test_cli_on_the_host(tmp_path, capsys):
    src, prd, ids = CU.write_cli_case(tmp_path)
    out_file, per_file = os.path.join(tmp_path, "m.json"), os.path.join(tmp_path, "per.json")
    out = EC.main(["--predictions", prd, "--src_file", src, "--split", "val", "--dataset", "coco", "--metrics_on", "host", "--output_file", out_file,
                   "--per_image_file", per_file])
    printed = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert printed == json.load(open(out_file)) == out
    assert sorted(out) == sorted(CM.METRICS + ("images", "scored_on_host"))
    assert out["images"] == 7 and out["scored_on_host"] == 2                  # the two images that fit no kernel call; never more than 2 of 7
    assert 0 < out["Bleu_4"] < out["Bleu_1"] <= 1 and 0 < out["ROUGE_L"] < 1 and out["CIDEr"] > 0
    per = json.load(open(per_file))
    assert [p["image_id"] for p in per] == ids and sorted(ids) == list(range(100, 107))
    # what does not fit the kernel: the fallback of --metrics_on device would score exactly these two, and no more than 2 of 7
    refs = EC.references_of(src, "val", "coco")
    unfit = [i for i in ids if len(refs[i]) > CM.MAX_R or any(len(r) > CM.MAX_T for r in refs[i])]
    assert sorted(unfit) == [102, 104] and len(unfit) <= 2
    assert len(refs) == 7 and len(refs[104]) == 9 and max(len(r) for r in refs[102]) == 70
    # the values are those of the classes on the tokenised captions
    preds = {p["image_id"]: p["caption"] for p in json.load(open(prd))}
    assert all(c[0].isupper() and c.endswith(" .") for c in preds.values())
    want = CM.CaptionMetrics().score([refs[i] for i in ids], [[w for w in preds[i].lower().split() if w != "."] for i in ids])
    for k in CM.METRICS:
        assert out[k] == want[k]


def test_cli_errors(tmp_path):
    src, prd, ids = CU.write_cli_case(tmp_path)
    preds = json.load(open(prd))
    base = ["--src_file", src, "--split", "val", "--dataset", "coco", "--metrics_on", "host"]

    def run(p):
        path = os.path.join(tmp_path, "bad.json")
        json.dump(p, open(path, "w"))
        return EC.main(["--predictions", path] + base)
    with pytest.raises(ValueError, match="not an image of the split"):
        run(preds + [{"image_id": 107, "caption": "a dog"}])                  # an image of split train
    with pytest.raises(ValueError, match="not an image of the split"):
        run(preds + [{"image_id": 5, "caption": "a dog"}])
    with pytest.raises(ValueError, match="occurs twice"):
        run(preds + [dict(preds[0])])
    with pytest.raises(ValueError, match="distinct words"):
        run([dict(preds[0], caption=" ".join("w%d" % i for i in range(65535)))] + preds[1:])
    assert run(preds[:3])["images"] == 3                                      # a subset of the split is fine
