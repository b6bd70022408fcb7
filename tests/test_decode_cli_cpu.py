"""CPU: the host-only pieces of vlp_amd.decode_img2txt (flags, image list, vocabulary lookups, detokenisation, decoder inputs)."""
import os

import pytest
import torch

from vlp_amd import decode_img2txt as D
from vlp_amd import synthetic as S

# the reference script's flags and defaults (vlp/decode_img2txt.py:55-104)
REFERENCE_FLAGS = {
    "config_path": None, "bert_model": "bert-base-cased", "model_recover_path": None, "max_position_embeddings": 512, "fp16": False, "amp": False,
    "seed": 123, "do_lower_case": False, "new_segment_ids": False, "batch_size": 4, "beam_size": 1, "length_penalty": 0,
    "forbid_duplicate_ngrams": False, "forbid_ignore_word": None, "min_len": None, "ngram_size": 3, "max_tgt_length": 20,
    "src_file": "/mnt/dat/COCO/annotations/dataset_coco.json", "dataset": "coco", "len_vis_input": 100, "image_root": "/mnt/dat/COCO/images",
    "split": "val", "drop_prob": 0.1, "enable_butd": False,
    "region_bbox_file": "coco_detection_vg_thresh0.2_feat_gvd_checkpoint_trainvaltest.h5",
    "region_det_file_prefix": "feat_cls_1000/coco_detection_vg_100dets_gvd_checkpoint_trainval", "file_valid_jpgs": "",
}


def test_flags_and_defaults_match_the_reference():
    ours = {a.dest: a.default for a in D.build_parser()._actions if a.dest != "help"}
    for name, default in REFERENCE_FLAGS.items():
        assert name in ours, name
        assert ours[name] == default and type(ours[name]) is type(default), (name, ours[name], default)
    assert set(ours) - set(REFERENCE_FLAGS) == {"packed_features", "vocab_file", "output_file", "num_hidden_layers"}


def test_word_pieces_are_merged_as_the_reference_detokenizes():
    assert D.merge_word_pieces(["a", "sur", "##f", "##er", "rides", "##x"]) == ["a", "surfer", "ridesx"]
    assert D.merge_word_pieces(["##lead", "b"]) == ["##lead", "b"]          # a leading piece has nothing to join (reference :39)
    assert D.merge_word_pieces([]) == []


def test_forbid_ignore_word_parsing():
    assert D.parse_forbid_ignore_word("[sep]|.|[Pad]|the") == ["[SEP]", ".", "[PAD]", "the"]
    assert D.parse_forbid_ignore_word("[unclosed") == ["[unclosed"]


def write_vocab(path, n=200):
    toks = ["tok%d" % i for i in range(n)]
    for name, i in (("[PAD]", S.PAD_ID), ("[UNK]", S.UNK_ID), ("[CLS]", S.CLS_ID), ("[SEP]", S.SEP_ID), ("[MASK]", S.MASK_ID)):
        toks[i] = name
    toks[7], toks[8], toks[9] = "sur", "##f", "."
    with open(path, "w", encoding="utf-8") as f:
        f.write("\n".join(toks) + "\n")
    return toks


def test_vocabulary_lookups(tmp_path):
    path = os.path.join(tmp_path, "vocab.txt")
    write_vocab(path)
    v = D.Vocab(path)
    assert len(v) == 200
    assert D.special_ids(v) == (S.CLS_ID, S.UNK_ID, S.SEP_ID, S.MASK_ID, S.PAD_ID)
    assert D.special_ids(None) == (S.CLS_ID, S.UNK_ID, S.SEP_ID, S.MASK_ID, S.PAD_ID)
    assert D.forbid_ignore_set("[sep]|.", v) == {S.SEP_ID, 9}
    assert D.forbid_ignore_set(None, v) is None and D.forbid_ignore_set(None, None) is None
    with pytest.raises(ValueError, match="vocabulary"):
        D.forbid_ignore_set(".", None)
    with pytest.raises(KeyError):
        D.forbid_ignore_set("nosuchword", v)
    # cut at the first [SEP] / [PAD], merge the pieces; without a vocabulary the ids themselves
    assert D.caption_of([7, 8, 9, S.SEP_ID, 7, 0], v, S.SEP_ID, S.PAD_ID) == "surf ."
    assert D.caption_of([7, S.PAD_ID, 8], v, S.SEP_ID, S.PAD_ID) == "sur"
    assert D.caption_of([7, 8, 9, S.SEP_ID, 7], None, S.SEP_ID, S.PAD_ID) == "7 8 9"
    assert D.caption_of([S.SEP_ID], v, S.SEP_ID, S.PAD_ID) == ""


IMAGES = [
    {"split": "val", "filename": "COCO_val2014_000000000042.jpg", "filepath": "val2014", "imgid": 900},
    {"split": "test", "filename": "COCO_val2014_000000000073.jpg", "filepath": "val2014", "imgid": 901},
    {"split": "val", "filename": "COCO_val2014_000000581929.jpg", "filepath": "val2014", "imgid": 902},
]


def test_image_list_filter_and_image_id_rules():
    assert D.select_images(IMAGES, "val", "coco") == [(42, "COCO_val2014_000000000042"), (581929, "COCO_val2014_000000581929")]
    assert D.select_images(IMAGES, "test", "coco") == [(73, "COCO_val2014_000000000073")]
    # the valid-jpg list only filters datasets other than coco / flickr30k (reference :191-194)
    assert len(D.select_images(IMAGES, "val", "coco", valid_jpgs={"COCO_val2014_000000000042.jpg"})) == 2
    assert D.select_images(IMAGES, "val", "cc", valid_jpgs={"COCO_val2014_000000581929.jpg"}) == [(902, "COCO_val2014_000000581929")]
    assert D.select_images(IMAGES, "val", "cc") == [(900, "COCO_val2014_000000000042"), (902, "COCO_val2014_000000581929")]
    flickr = [{"split": "test", "filename": "1007129816.jpg"}, {"split": "train", "filename": "12.jpg"}]
    assert D.select_images(flickr, "test", "flickr30k") == [(1007129816, "1007129816")]
    with pytest.raises(ValueError):
        D.select_images(IMAGES, "val", "nocaps")


def test_output_path_rules():
    args = D.build_parser().parse_args(["--split", "test"])
    assert D.output_path(args, "/x/model.30.bin", 1) == "/x/model.30-test-captions.json"
    args.output_file = "/y/out.json"
    assert D.output_path(args, "/x/model.30.bin", 1) == "/y/out.json"
    assert D.output_path(args, "/x/model.30.bin", 2) == "/y/out.model.30.json"


@pytest.mark.parametrize("new_segment_ids", [True, False])
def test_decoder_inputs_equal_the_loader_restatement(new_segment_ids):
    """Against oracle.make_golden.decode_inputs (Preprocess4Seq2seqDecoder's output as the decoder fixtures were generated with)."""
    from oracle.make_golden import decode_inputs
    B, T, Nv = 3, 7, 100
    _, _, ids, seg, pos, am = decode_inputs(B, T, 1, Nv=Nv)
    got = D.decoder_inputs(B, Nv, T, new_segment_ids, S.CLS_ID, S.UNK_ID, S.SEP_ID, torch.device("cpu"))
    if not new_segment_ids:
        seg = seg - 4                                                 # segments 0 | 1 instead of 4 | 5 (seq2seq_loader.py:404-409)
    for g, w in zip(got, (ids, seg, pos, am)):
        assert g.dtype == torch.long and g.is_contiguous() and torch.equal(g, w)


def test_main_needs_fp16_and_a_packed_store(tmp_path):
    with pytest.raises(NotImplementedError, match="--fp16"):
        D.main(["--enable_butd", "--packed_features", str(tmp_path), "--model_recover_path", "x"])
    with pytest.raises(NotImplementedError, match="--amp only engages"):
        D.main(["--enable_butd", "--amp", "--packed_features", str(tmp_path), "--model_recover_path", "x"])
    with pytest.raises(NotImplementedError, match="--packed_features"):
        D.main(["--enable_butd", "--fp16", "--model_recover_path", "x"])
