"""GPU: python -m vlp_amd.decode_img2txt end to end -- a packed store of 5 images, a 2-layer checkpoint, a generated vocabulary and a
Karpathy-style image list; the captions the command writes must be those of BertForSeq2SeqDecoder called directly, one image at a time."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from oracle import vlp_oracle as O                         # noqa: E402  (checker: parameter init only)
from oracle.make_golden import decode_inputs               # noqa: E402  (pure helper)
from vlp_amd import decode_img2txt as D                    # noqa: E402
from vlp_amd import synthetic as S                         # noqa: E402
from vlp_amd.data import write_packed                      # noqa: E402
from vlp_amd.input_prep import RawRegions                  # noqa: E402
from vlp_amd.modeling import BertConfig                    # noqa: E402

DEV = torch.device("cuda:0")
NV, T, VOCAB = 100, 10, 1024
# 7 images over two splits; the 5 of "test" are in the store (in another order than the list's)
LIST = [("test", 391895), ("val", 522418), ("test", 184613), ("test", 318219), ("val", 554625), ("test", 574769), ("test", 60623)]


def fname(i):
    return "COCO_val2014_%012d.jpg" % i


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("decode_cli"))
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
    # bert directory: config + vocabulary (specials at the vlp_amd.synthetic ids, every third ordinary token a ## piece)
    bert = os.path.join(root, "bert")
    os.makedirs(bert)
    with open(os.path.join(bert, "bert_config.json"), "w") as f:
        f.write(BertConfig(VOCAB, num_hidden_layers=2, type_vocab_size=2).to_json_string())
    special = {S.PAD_ID: "[PAD]", S.UNK_ID: "[UNK]", S.CLS_ID: "[CLS]", S.SEP_ID: "[SEP]", S.MASK_ID: "[MASK]"}
    tokens, n_ord = [], 0
    for i in range(VOCAB):
        if i in special:
            tokens.append(special[i])
        else:
            tokens.append(("##p%d" if n_ord % 3 == 2 else "w%d") % i)
            n_ord += 1
    with open(os.path.join(bert, "vocab.txt"), "w") as f:
        f.write("\n".join(tokens) + "\n")
    p = O.init_params(vocab_size=VOCAB, layers=2, tasks="img2txt", seed=27, std=0.1)
    sd = dict(p)
    sd["cls.predictions.decoder.weight"] = p["bert.embeddings.word_embeddings.weight"]
    ckpt = os.path.join(root, "model.3.bin")
    torch.save(sd, ckpt)
    src = os.path.join(root, "dataset.json")
    with open(src, "w") as f:
        json.dump({"images": [{"split": sp, "filename": fname(i), "filepath": "val2014", "imgid": n} for n, (sp, i) in enumerate(LIST)]}, f)
    row_of = {k: r for r, k in enumerate(keys)}
    regions = {i: (torch.from_numpy(feats[row_of[fname(i)[:-4]]]), torch.from_numpy(boxes[row_of[fname(i)[:-4]]]),
                   torch.from_numpy(cls[row_of[fname(i)[:-4]]].astype(np.float16))) for i in test_ids}
    return dict(root=root, store=store, bert=bert, ckpt=ckpt, src=src, tokens=tokens, test_ids=test_ids, regions=regions)


def argv(su, out, beam):
    return ["--bert_model", su["bert"], "--model_recover_path", su["ckpt"], "--packed_features", su["store"], "--src_file", su["src"], "--split", "test",
            "--dataset", "coco", "--output_file", out, "--batch_size", "2", "--beam_size", str(beam), "--forbid_duplicate_ngrams", "--ngram_size", "2",
            "--min_len", "2", "--max_tgt_length", str(T), "--new_segment_ids", "--fp16", "--enable_butd"]


def expected_caption(ids, tokens):
    """Cut at the first [SEP] / [PAD], then join the ## pieces to the word before them (written out here, independently of the module)."""
    words = []
    for t in ids:
        tok = tokens[t]
        if tok in ("[SEP]", "[PAD]"):
            break
        if tok.startswith("##") and words:
            words[-1] += tok[2:]
        else:
            words.append(tok)
    return " ".join(words)


def direct(su, beam):
    """The model called directly on every image of the split, one image per call."""
    args = D.build_parser().parse_args(argv(su, "unused", beam))
    model = D.build_decoder(args, D.Vocab(os.path.join(su["bert"], "vocab.txt")), torch.load(su["ckpt"], map_location="cpu"), DEV)
    assert model.ngram_blocking == "device" and model.search_beam_size == beam and model.eos_id == S.SEP_ID and model.mask_word_id == S.MASK_ID
    _, _, input_ids, seg, pos, am = [t.to(DEV) for t in decode_inputs(1, T, 0, Nv=NV)]
    caps = []
    for i in su["test_ids"]:
        feat, box, cls = su["regions"][i]
        call = (feat.unsqueeze(0).to(DEV), RawRegions(box.unsqueeze(0).to(DEV), cls.unsqueeze(0).to(DEV)), input_ids, seg, pos, am)
        with torch.no_grad():
            if beam > 1:
                ids = model.beam_search(*call)["pred_seq"][0].tolist()
            else:
                ids = model(*call, task_idx=None, sample_mode="greedy")[0][0].tolist()
        caps.append(expected_caption(ids, su["tokens"]))
    return caps


@pytest.mark.parametrize("beam", [3, 1])
def test_cli_captions_equal_the_model_called_directly(setup, beam):
    su = setup
    out = os.path.join(su["root"], "captions_beam%d.json" % beam)
    res = D.main(argv(su, out, beam))
    with open(out) as f:
        preds = json.load(f)
    assert res == {su["ckpt"]: preds}
    assert [p["image_id"] for p in preds] == su["test_ids"]                       # the split's images, in list order, by the COCO id rule
    assert all(type(p["image_id"]) is int and type(p["caption"]) is str and set(p) == {"image_id", "caption"} for p in preds)
    want = direct(su, beam)
    print("beam %d captions: %s" % (beam, [p["caption"] for p in preds]))
    assert [p["caption"] for p in preds] == want
    assert any(len(c.split()) >= 2 for c in want)                                 # real captions, not five empty strings
    assert len(set(want)) > 1                                                     # the images differ: an order or batching mix-up would show


def test_cli_raises_without_fp16(setup):
    su = setup
    args = [a for a in argv(su, os.path.join(su["root"], "never.json"), 3) if a != "--fp16"]
    with pytest.raises(NotImplementedError, match="--fp16"):
        D.main(args)
    assert not os.path.exists(os.path.join(su["root"], "never.json"))
