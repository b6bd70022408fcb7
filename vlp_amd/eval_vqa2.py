"""VQA 2.0 prediction from a fine-tuned checkpoint: the counterpart of the reference's vlp/eval_vqa2.py on packed region features.

    python -m vlp_amd.eval_vqa2 --bert_model DIR --model_recover_path 'out/model.*.bin' --packed_features STORE \\
        --token_file vqa_val.json --answer_vocab_file answers_vqa.txt --split val --fp16 --enable_butd --new_segment_ids --batch_size 64

Every flag of the reference script keeps its name and default (the flags it shares with decoding and never reads -- --beam_size,
--length_penalty, --forbid_duplicate_ngrams, --forbid_ignore_word, --min_len, --ngram_size -- are accepted as well).  What differs:
  * there is no tokenizer: the questions come pre-tokenised from --token_file, a json list of [image id, question token ids, answer ids,
    question id] (vlp_amd.data.vqa_examples_from_imdb converts the reference's imdb array, --src_file there); --src_file is not read;
  * region features come from a vlp_amd.data packed store (--packed_features) and go to the model as stored (fp16 features + RawRegions);
  * the inputs of Preprocess4Seq2seq(0, 0, ..., mode="bi", always_truncate_tail=True, max_len_b=max_tgt_length) (eval_vqa2.py:138-144) are
    built by TextPreprocessor(mode="bi") with a MaskSpec in place of the [L, L] mask, so the forward is padding-free;
  * the answer is chosen on the device (BertForPreTrainingLossMask.answer: vlp_vqa_answer_rows) and written as the line of
    --answer_vocab_file with that index (one answer per line, the reference's answers_vqa.txt); without the file, as the index itself;
  * the predictions [{"question_id", "answer"}, ...] (input order) go to --output_file, or next to the checkpoint;
  * the reference then starts Pythia's evaluation script on the results file.  Pythia is not part of this project.  When the examples carry
    answers and --split is not test2015, this script logs and returns the SOFT-SCORE ACCURACY instead: the mean over the questions of the score
    the question's human answers give the predicted answer (SparseAnswers.answer_scores), in percent.  That is Pythia's training-time
    metric over the answer vocabulary; it is NOT the official evaluator's number, which normalises the answer strings first.
--do_lower_case, --src_file, --ref_file, --image_root, --region_bbox_file, --region_det_file_prefix, --output_dir, --file_valid_jpgs, --dataset and
--seed are accepted for the reference's command lines; nothing here depends on them (no tokenizer, no h5 files, no random draw: max_pred = 0).
A short last batch is filled up with its last question (and the extra rows dropped), so every batch runs the same launches.
"""
import argparse
import glob
import json
import logging
import os

import torch

from . import synthetic
from .data import PackedRegionStore, TextPreprocessor, examples_have_answers, FEAT_DIM, BOX_DIM
from .decode_img2txt import require_fp16
from .input_prep import MaskSpec, RawRegions, SparseAnswers, N_CLS, N_ANSWER_SLOTS
from .modeling import BertForPreTrainingLossMask, load_checkpoint_state
from .run_img2txt_dist import KNOWN_VOCABS, model_config

logger = logging.getLogger(__name__)

# the reference script's command line, flag for flag (vlp/eval_vqa2.py:57-109): (name, type, default); its store_true switches follow
_REFERENCE_OPTIONS = (
    ("bert_model", str, "bert-base-cased"), ("model_recover_path", str, None), ("seed", int, 123), ("batch_size", int, 4), ("beam_size", int, 1),
    ("length_penalty", float, 0), ("forbid_ignore_word", str, None), ("min_len", int, None), ("ngram_size", int, 3), ("max_tgt_length", int, 20),
    ("src_file", str, "/mnt/dat/COCO/annotations/dataset_coco.json"), ("ref_file", str, "pythia/data/v2_mscoco_val2014_annotations.json"),
    ("dataset", str, "coco"), ("len_vis_input", int, 100), ("image_root", str, "/mnt/dat/COCO/images"), ("split", str, "val"),
    ("drop_prob", float, 0.1), ("region_bbox_file", str, "coco_detection_vg_thresh0.2_feat_gvd_checkpoint_trainvaltest.h5"),
    ("region_det_file_prefix", str, "feat_cls_1000/coco_detection_vg_100dets_gvd_checkpoint_trainval"), ("output_dir", str, "tmp"),
    ("file_valid_jpgs", str, ""))
_REFERENCE_SWITCHES = ("fp16", "amp", "do_lower_case", "new_segment_ids", "forbid_duplicate_ngrams", "enable_butd")


def build_parser():
    p = argparse.ArgumentParser(description="Answer the questions of one VQA 2.0 split from a fine-tuned checkpoint.")
    for name, kind, default in _REFERENCE_OPTIONS:
        p.add_argument("--" + name, type=kind, default=default)
    for name in _REFERENCE_SWITCHES:
        p.add_argument("--" + name, action="store_true")
    p.add_argument("--packed_features", default="", help="directory of a vlp_amd.data packed region store (write_packed / pack_from_h5); required")
    p.add_argument("--token_file", default="", help="json list of [image id, [question token ids], [answer ids], question id] "
                                                     "(vlp_amd.data.vqa_examples_from_imdb); required: there is no tokenizer")
    p.add_argument("--answer_vocab_file", default=None, help="the answer vocabulary, one answer per line (line number = index); without it the "
                                                             "answers are written as indices")
    p.add_argument("--output_file", default=None, help="where the predictions go (default: next to the checkpoint, <checkpoint>-<split>-vqa2.json)")
    p.add_argument("--config_path", default=None, type=str)
    p.add_argument("--num_hidden_layers", type=int, default=None, help="override the config's depth (plumbing tests)")
    return p


# ---- host-only pieces --------------------------------------------------------------------------------------------------
def load_answer_vocab(path):
    with open(path, "r", encoding="utf-8") as f:
        words = [line.rstrip("\n") for line in f]
    while words and words[-1] == "":
        words.pop()
    return words


def load_questions(path):
    """--token_file -> [(image id, question token ids, answer ids, question id)]; a caption file (no answers, no question ids) is refused."""
    with open(path) as f:
        examples = [tuple(e) for e in json.load(f)]
    if not examples:
        raise ValueError("--token_file %s holds no examples" % path)
    if not examples_have_answers(examples):
        from .data import VQA_EXAMPLE_FORMAT
        raise ValueError("--token_file %s holds caption examples: %s" % (path, VQA_EXAMPLE_FORMAT))
    return examples


def question_preprocessor(args):
    """Preprocess4Seq2seq(0, 0, ..., mode='bi', truncate_config={max_len_b: max_tgt_length, trunc_seg: 'b', always_truncate_tail: True})
    (eval_vqa2.py:138-144): nothing is masked (max_pred = 0), so it draws nothing."""
    return TextPreprocessor(max_pred=0, mask_prob=0, vocab_size=KNOWN_VOCABS.get(args.bert_model, 28996), cls_id=synthetic.CLS_ID,
                            sep_id=synthetic.SEP_ID, mask_id=synthetic.MASK_ID, unk_id=synthetic.UNK_ID,
                            max_len=args.max_tgt_length + args.len_vis_input + 3, max_len_b=args.max_tgt_length, mode="bi",
                            len_vis_input=args.len_vis_input, new_segment_ids=args.new_segment_ids, trunc_seg="b", always_truncate_tail=True)


def output_path(args, ckpt, n_ckpts):
    if not args.output_file:
        return "%s-%s-vqa2.json" % (os.path.splitext(ckpt)[0], args.split)
    if n_ckpts == 1:
        return args.output_file
    root, ext = os.path.splitext(args.output_file)
    return "%s.%s%s" % (root, os.path.splitext(os.path.basename(ckpt))[0], ext)


def check_args(args):
    require_fp16(args)
    if args.enable_butd:
        assert args.len_vis_input == 100
    if not args.packed_features:
        raise NotImplementedError("give --packed_features DIR (vlp_amd.data; the reference's h5 files are converted once with pack_from_h5)")
    if not args.token_file:
        raise NotImplementedError("give --token_file FILE: vlp_amd has no tokenizer, the questions of --src_file are tokenised once with "
                                  "vlp_amd.data.vqa_examples_from_imdb")
    if not args.model_recover_path:
        raise ValueError("--model_recover_path is required")
    args.max_position_embeddings = 512                  # eval_vqa2.py:165
    args.label_smoothing = 0


# ---- device side -------------------------------------------------------------------------------------------------------
def build_model(args, state, device):
    config = model_config(args)
    model = BertForPreTrainingLossMask(config, num_labels=2, enable_butd=args.enable_butd, len_vis_input=args.len_vis_input, tasks="vqa2",
                                       allow_random_fc7=True)             # (every weight comes from the checkpoint, vis_embed.0 included)
    load_checkpoint_state(model, state)
    model.half()
    model.to(device)
    return model.eval()


def answer_questions(model, store, examples, args, device, with_scores):
    """(answer indices, scores or None) of `examples`, in order: one model.answer() per batch of --batch_size questions."""
    Nv, bs = args.len_vis_input, args.batch_size
    if store.nv != Nv:
        raise RuntimeError("the packed store holds %d regions per image, --len_vis_input is %d" % (store.nv, Nv))
    proc = question_preprocessor(args)
    L = proc.max_len
    feat = torch.empty(bs, Nv, FEAT_DIM, dtype=torch.float16).pin_memory()
    cls = torch.empty(bs, Nv, N_CLS, dtype=torch.float16).pin_memory()
    bbox = torch.empty(bs, Nv, BOX_DIM, dtype=torch.float32).pin_memory()
    text = torch.empty(2, bs, L, dtype=torch.long).pin_memory()
    a_idx = torch.empty(bs, N_ANSWER_SLOTS, dtype=torch.int32).pin_memory()
    a_score = torch.empty(bs, N_ANSWER_SLOTS, dtype=torch.float32).pin_memory()
    ids_out, scores_out = [], []
    with torch.no_grad():
        for i in range(0, len(examples), bs):
            chunk = list(examples[i:i + bs])
            n = len(chunk)
            chunk = chunk + [chunk[-1]] * (bs - n)                  # a short last batch runs at the full size
            store.gather(store.rows([e[0] for e in chunk]), feat.numpy(), cls.numpy(), bbox.numpy())
            toks = [proc(e[1]) for e in chunk]
            text.numpy()[0] = [t["input_ids"] for t in toks]
            text.numpy()[1] = [t["segment_ids"] for t in toks]
            spec = MaskSpec.from_lengths([t["len_a"] for t in toks], [t["len_b"] for t in toks], False, device=device)
            answers = None
            if with_scores:
                answers = SparseAnswers.from_answer_ids([e[2] for e in chunk], out=(a_idx.numpy(), a_score.numpy())).to(device, non_blocking=True)
            text_d = text.to(device, non_blocking=True)
            regions = RawRegions(bbox.to(device, non_blocking=True), cls.to(device, non_blocking=True))
            idx, _, score = model.answer(feat.to(device, non_blocking=True), regions, text_d[0], text_d[1], spec, answers=answers)
            ids_out.extend(idx.tolist()[:n])                        # synchronises: the pinned buffers are free again
            if with_scores:
                scores_out.extend(score.tolist()[:n])
    return ids_out, (scores_out if with_scores else None)


def main(argv=None):
    """Returns {checkpoint: (predictions, soft-score accuracy in percent or None)}."""
    args = build_parser().parse_args(argv)
    check_args(args)
    if not torch.cuda.is_available():
        raise RuntimeError("vlp_amd: the model runs on the HIP engine only; there is no CPU path")
    device = torch.device("cuda")
    examples = load_questions(args.token_file)
    words = load_answer_vocab(args.answer_vocab_file) if args.answer_vocab_file else None
    with_scores = args.split != "test2015" and any(len(e[2]) > 0 for e in examples)
    store = PackedRegionStore(args.packed_features)

    ckpts = sorted(glob.glob(args.model_recover_path.strip()))
    if not ckpts:
        raise FileNotFoundError("--model_recover_path %r matches no file" % (args.model_recover_path,))
    results = {}
    for ckpt in ckpts:
        logger.info("***** Recover model: %s *****", ckpt)
        model = build_model(args, torch.load(ckpt, map_location="cpu"), device)
        ids, scores = answer_questions(model, store, examples, args, device, with_scores)
        predictions = [{"question_id": e[3], "answer": (words[i] if words is not None else i)} for e, i in zip(examples, ids)]
        out = output_path(args, ckpt, len(ckpts))
        with open(out, "w") as f:
            json.dump(predictions, f)
        logger.info("wrote %d answers to %s", len(predictions), out)
        accuracy = None
        if scores is not None:
            accuracy = 100.0 * sum(scores) / len(scores)
            logger.info("soft-score accuracy over the answer vocabulary (not the official evaluator's): %.2f", accuracy)
        else:
            logger.info("no accuracy: %s", "the test set has no public answers; submit %s to the VQA 2.0 server" % out
                        if args.split == "test2015" else "the examples carry no answers")
        results[ckpt] = (predictions, accuracy)
        del model
    return results


if __name__ == "__main__":
    logging.basicConfig(format="%(asctime)s - %(levelname)s - %(name)s -   %(message)s", datefmt="%m/%d/%Y %H:%M:%S", level=logging.INFO)
    main()
