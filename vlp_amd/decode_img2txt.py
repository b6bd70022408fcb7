"""Caption decoding from a fine-tuned checkpoint: the counterpart of the reference's vlp/decode_img2txt.py on packed region features.

    python -m vlp_amd.decode_img2txt --bert_model DIR --model_recover_path 'out/model.*.bin' --packed_features STORE \\
        --src_file dataset_coco.json --split val --fp16 --enable_butd --new_segment_ids --beam_size 3 --forbid_duplicate_ngrams

Every flag of the reference script keeps its name and default.  What differs:
  * region features come from a vlp_amd.data packed store (--packed_features, keyed by the file name's stem) and go to the model as stored:
    fp16 features plus RawRegions (boxes, class probabilities); vlp_vis_pe_prep encodes them on the device (seq2seq_loader.py:459-470);
  * the decoder inputs of Preprocess4Seq2seqDecoder (seq2seq_loader.py:390-429: [CLS] [UNK]*Nv [SEP], segments, positions, the prefix-visible /
    target-causal mask) are built on the device, once per batch size;
  * there is no tokenizer: the vocabulary file only maps the special tokens and --forbid_ignore_word to ids and the decoded ids back to word
    pieces.  Without one the ids of vlp_amd.synthetic are used and captions are written as space-joined token ids;
  * the predictions [{"image_id", "caption"}, ...] (input order; the list the reference hands to language_eval) are written to --output_file;
    python -m vlp_amd.eval_captions scores them (BLEU-1..4, ROUGE-L, CIDEr; no Java).
--do_lower_case, --image_root, --region_bbox_file and --region_det_file_prefix are accepted for the reference's command lines and not used: there is
no tokenizer, and the features come from the packed store.
A short last batch is filled up with its last image (and the extra rows dropped), so every batch runs the same launches.

  --n_best N (1..--beam_size; default 1: the tool as above, byte for byte) keeps the N best finished hypotheses of every image's beam search,
      ranked and back-tracked on the device (vlp_beam_nbest; vlp_amd.nbest.beam_nbest_host is the rule).  Rank 0 is the caption written without the flag
  --nbest_file PATH receives every hypothesis, ordered by image and rank (rank 0 always; the others unless they went on after their [SEP]):
      {"image_id": ..., "rank": n, "caption": "...", "logprob": cumulative log-probability, "value": logprob + length_penalty * length}
  --select {none,consensus,logprob}, --consensus_df PATH and --samples_file (here an alias of --nbest_file) are vlp_amd.sample_img2txt's flags,
      applied to the hypotheses of the beam instead of samples: none writes rank 0; logprob the hypothesis with the largest logprob; consensus
      (2 <= N <= 16) the one with the largest CIDEr-D against the image's other hypotheses, scored on the device.  With a selection
      --output_file receives {"image_id", "caption", "rank", "logprob", "utility"} per image, which python -m vlp_amd.eval_captions reads as it stands.
  --beam_groups G (1..--beam_size, dividing it; default 1: the tool as above, byte for byte) with --diversity_penalty L (finite, >= 0) runs a
      diverse beam search (vlp_amd.diverse; vlp_beam_select_groups on the device): the beams in G groups, a word penalised by L for every
      earlier group that chose it in the same step.  logprob / value stay unpenalised, so --n_best, --nbest_file and --select work on the
      diverse beam unchanged -- and have hypotheses that differ to choose from.
  --constraints_file PATH (default: none, the tool as above, byte for byte) runs a constrained beam search (vlp_amd.constrained;
      vlp_logsoftmax_topk_want and vlp_beam_select_constrained on the device): PATH is a json object {image id: [phrase, ...]}, a phrase a
      list of word-piece ids or a string whose words are looked up in the vocabulary (--do_lower_case is honoured; a missing word is split
      by the greedy longest-match-first WordPiece rule with ## continuations).  At most 8 phrases of at most 8 pieces per image; a phrase
      that needs [UNK] or names a special token is an error, as are --beam_groups > 1 and --beam_size < 2.  Images without an entry are
      searched unconstrained.  Every record of --output_file (and of --nbest_file) gains "constraints" (the image's phrases as id lists) and
      "met" (one boolean per phrase); python -m vlp_amd.eval_captions reads the file as it stands.
"""
import argparse
import glob
import json
import logging
import os
import random

import numpy as np
import torch

from . import synthetic
from .data import PackedRegionStore, FEAT_DIM, BOX_DIM
from .input_prep import RawRegions, N_CLS
from .modeling import BertForSeq2SeqDecoder, load_checkpoint_state
from .run_img2txt_dist import model_config

logger = logging.getLogger(__name__)


# the reference script's command line, flag for flag: (name, type, default); its store_true switches follow
_REFERENCE_OPTIONS = (
    ("config_path", str, None), ("bert_model", str, "bert-base-cased"), ("model_recover_path", str, None), ("max_position_embeddings", int, 512),
    ("seed", int, 123), ("batch_size", int, 4), ("beam_size", int, 1), ("length_penalty", float, 0), ("forbid_ignore_word", str, None),
    ("min_len", int, None), ("ngram_size", int, 3), ("max_tgt_length", int, 20), ("src_file", str, "/mnt/dat/COCO/annotations/dataset_coco.json"),
    ("dataset", str, "coco"), ("len_vis_input", int, 100), ("image_root", str, "/mnt/dat/COCO/images"), ("split", str, "val"),
    ("drop_prob", float, 0.1), ("region_bbox_file", str, "coco_detection_vg_thresh0.2_feat_gvd_checkpoint_trainvaltest.h5"),
    ("region_det_file_prefix", str, "feat_cls_1000/coco_detection_vg_100dets_gvd_checkpoint_trainval"), ("file_valid_jpgs", str, ""))
_REFERENCE_SWITCHES = ("fp16", "amp", "do_lower_case", "new_segment_ids", "forbid_duplicate_ngrams", "enable_butd")


def build_parser():
    p = argparse.ArgumentParser(description="Write captions for the images of one split from a fine-tuned checkpoint.")
    for name, kind, default in _REFERENCE_OPTIONS:
        p.add_argument("--" + name, type=kind, default=default)
    for name in _REFERENCE_SWITCHES:
        p.add_argument("--" + name, action="store_true")
    p.add_argument("--packed_features", default="", help="directory of a vlp_amd.data packed region store (write_packed / pack_from_h5); required")
    p.add_argument("--vocab_file", default=None, help="WordPiece vocabulary, one token per line (default: <bert_model>/vocab.txt when --bert_model is a "
                                                      "directory); without one, captions are written as token ids")
    p.add_argument("--output_file", default=None, help="where the predictions go (default: next to the checkpoint, <checkpoint>-<split>-captions.json)")
    p.add_argument("--num_hidden_layers", type=int, default=None, help="override the config's depth (plumbing tests)")
    return p


MAX_CONSENSUS = 16          # vlp_amd.consensus: a consensus is taken among 2..16 hypotheses of an image


def parse_args(argv=None):
    """The parsed command line of this tool, or the parser's error exit: build_parser()'s flags, the n-best list and the selection flags of
    vlp_amd.sample_img2txt (here they choose among the hypotheses of the beam instead of samples)."""
    from .sample_img2txt import add_selection_flags
    p = build_parser()
    p.add_argument("--n_best", type=int, default=1,
                   help="keep the N best finished hypotheses of every image's beam search, 1..--beam_size (default 1: the best one only)")
    p.add_argument("--nbest_file", default=None, metavar="PATH",
                   help="with --n_best >= 2: write every hypothesis here as {image_id, rank, caption, logprob, value} (--samples_file is an alias)")
    p.add_argument("--beam_groups", type=int, default=1, metavar="G",
                   help="diverse beam search: split the --beam_size beams into G groups, 1..--beam_size and dividing it (default 1: the plain search)")
    p.add_argument("--diversity_penalty", type=float, default=0.0, metavar="L",
                   help="with --beam_groups >= 2: subtract L from a word's score for every earlier group that chose it in the same step (default 0)")
    p.add_argument("--constraints_file", default=None, metavar="PATH",
                   help="constrained beam search: a json object {image id: [phrase, ...]} of phrases the caption must mention; a phrase is a list "
                        "of word-piece ids or a string (needs a vocabulary); at most 8 phrases of at most 8 pieces per image")
    add_selection_flags(p)
    a = p.parse_args(argv)
    a.constraints = None
    if a.constraints_file:
        if a.beam_size < 2:
            p.error("--constraints_file steers a beam search: it needs --beam_size >= 2 (got %d)" % a.beam_size)
        if a.beam_groups > 1:
            p.error("--constraints_file and --beam_groups %d (diverse beam search) exclude each other" % a.beam_groups)
        try:
            path = vocab_path(a)
            a.constraints = load_constraints(a.constraints_file, Vocab(path) if path else None, a.do_lower_case)
        except (OSError, ValueError) as e:
            p.error("--constraints_file %s: %s" % (a.constraints_file, e))
    if not (1 <= a.beam_groups <= max(a.beam_size, 1)):
        p.error("--beam_groups must be in 1..--beam_size = 1..%d (got %d)" % (max(a.beam_size, 1), a.beam_groups))
    if a.beam_size % a.beam_groups != 0:
        p.error("--beam_groups %d must divide --beam_size %d: the groups have equal size" % (a.beam_groups, a.beam_size))
    if not (a.diversity_penalty == a.diversity_penalty and 0.0 <= a.diversity_penalty < float("inf")):
        p.error("--diversity_penalty must be finite and >= 0 (got %r)" % (a.diversity_penalty,))
    if a.diversity_penalty != 0.0 and a.beam_groups == 1:
        p.error("--diversity_penalty %r penalises the words of earlier groups: it needs --beam_groups >= 2" % (a.diversity_penalty,))
    if a.n_best > 1 and a.beam_size < 2:
        p.error("--n_best %d lists the hypotheses of a beam search: it needs --beam_size >= 2 (got %d)" % (a.n_best, a.beam_size))
    if not (1 <= a.n_best <= max(a.beam_size, 1)):
        p.error("--n_best must be in 1..--beam_size = 1..%d (got %d)" % (max(a.beam_size, 1), a.n_best))
    if a.select != "none" and a.n_best < 2:
        p.error("--select %s chooses among the hypotheses of an image: it needs --n_best >= 2 (got %d)" % (a.select, a.n_best))
    if a.select == "consensus" and not a.consensus_df:
        p.error("--select consensus needs --consensus_df PATH (a table written by python -m vlp_amd.cider_df)")
    if a.select != "consensus" and a.consensus_df:
        p.error("--consensus_df %s needs --select consensus (it holds the document frequencies of the consensus score)" % a.consensus_df)
    if a.select == "consensus" and a.n_best > MAX_CONSENSUS:
        p.error("--select consensus scores 2..%d hypotheses of an image against each other (got --n_best %d)" % (MAX_CONSENSUS, a.n_best))
    if a.samples_file and a.nbest_file and a.samples_file != a.nbest_file:
        p.error("--samples_file is an alias of --nbest_file here: give one of them (got %s and %s)" % (a.samples_file, a.nbest_file))
    a.nbest_file = a.nbest_file or a.samples_file
    if a.nbest_file and a.n_best < 2:
        p.error("--nbest_file %s holds the hypotheses of an n-best list: it needs --n_best >= 2 (got %d)" % (a.nbest_file, a.n_best))
    return a


# ---- host-only pieces --------------------------------------------------------------------------------------------------
def merge_word_pieces(pieces):
    """WordPiece continuation pieces ('##ing') are glued onto the word in front of them; one that opens the caption stays as it is."""
    words = []
    for piece in pieces:
        if words and piece.startswith("##"):
            words[-1] += piece[2:]
        else:
            words.append(piece)
    return words


def parse_forbid_ignore_word(text):
    """decode_img2txt.py:149-155: '|'-separated words; a bracketed word ([sep]) names a special token and is upper-cased."""
    return [w.upper() if w.startswith("[") and w.endswith("]") else w for w in text.split("|")]


class Vocab(object):
    """The id <-> word-piece table of a BERT vocab.txt (one token per line, id = line number)."""

    def __init__(self, path):
        with open(path, "r", encoding="utf-8") as f:
            self.tokens = [line.rstrip("\n") for line in f]
        while self.tokens and self.tokens[-1] == "":
            self.tokens.pop()
        self.ids = {}
        for i, t in enumerate(self.tokens):
            self.ids.setdefault(t, i)

    def __len__(self):
        return len(self.tokens)

    def to_ids(self, tokens):
        missing = [t for t in tokens if t not in self.ids]
        if missing:
            raise KeyError("not in the vocabulary: %s" % ", ".join(missing))
        return [self.ids[t] for t in tokens]


def vocab_path(args):
    """--vocab_file, else <bert_model>/vocab.txt when --bert_model is a directory that has one, else None."""
    if args.vocab_file is None and os.path.isdir(args.bert_model) and os.path.exists(os.path.join(args.bert_model, "vocab.txt")):
        return os.path.join(args.bert_model, "vocab.txt")
    return args.vocab_file


def word_pieces(word, vocab):
    """The greedy longest-match-first WordPiece split of one word (continuations carry ##) as ids, or None when it cannot be built."""
    out, start = [], 0
    while start < len(word):
        end = len(word)
        while end > start:
            piece = ("##" if start else "") + word[start:end]
            if piece in vocab.ids:
                break
            end -= 1
        if end == start:
            return None
        out.append(vocab.ids[piece])
        start = end
    return out


def phrase_ids(phrase, vocab, do_lower_case=False):
    """One phrase of a constraints file as word-piece ids: a list of ids as it is, a string word by word (a word of the vocabulary is its id,
    any other is split by word_pieces).  ValueError for a phrase that is empty, needs [UNK] or contains a special token."""
    special = special_ids(vocab)
    if isinstance(phrase, str):
        if vocab is None:
            raise ValueError("the phrase %r is text: it needs a vocabulary (--vocab_file, or a --bert_model directory with vocab.txt)" % (phrase,))
        ids = []
        for word in (phrase.lower() if do_lower_case else phrase).split():
            if word.upper() in ("[CLS]", "[UNK]", "[SEP]", "[MASK]", "[PAD]"):
                raise ValueError("the phrase %r contains the special token %s" % (phrase, word.upper()))
            pieces = [vocab.ids[word]] if word in vocab.ids else word_pieces(word, vocab)
            if pieces is None:
                raise ValueError("the phrase %r cannot be built from the vocabulary without [UNK] (word %r)" % (phrase, word))
            ids.extend(pieces)
    elif isinstance(phrase, list) and all(isinstance(t, int) and not isinstance(t, bool) for t in phrase):
        ids = list(phrase)
        if any(t < 0 or (vocab is not None and t >= len(vocab)) for t in ids):
            raise ValueError("the phrase %r holds an id outside the vocabulary" % (phrase,))
    else:
        raise ValueError("a phrase is a string or a list of word-piece ids (got %r)" % (phrase,))
    if not ids:
        raise ValueError("the phrase %r is empty" % (phrase,))
    if any(t in special for t in ids):
        raise ValueError("the phrase %r contains a special token ([CLS], [UNK], [SEP], [MASK] or [PAD])" % (phrase,))
    return ids


def load_constraints(path, vocab, do_lower_case=False):
    """A constraints file -> {image id as a string: [id list, ...]}; ValueError names what is wrong with it."""
    from .constrained import MAX_CONS, MAX_LEN
    with open(path, "r", encoding="utf-8") as f:
        raw = json.load(f)
    if not isinstance(raw, dict) or not all(isinstance(v, list) for v in raw.values()):
        raise ValueError("expected a json object that maps an image id to a list of phrases")
    out = {}
    for imgid, phrases in raw.items():
        ids = [phrase_ids(ph, vocab, do_lower_case) for ph in phrases]
        if len(ids) > MAX_CONS:
            raise ValueError("image %s has %d phrases, at most %d are searched for" % (imgid, len(ids), MAX_CONS))
        for ph, t in zip(phrases, ids):
            if len(t) > MAX_LEN:
                raise ValueError("the phrase %r of image %s is %d word pieces long, at most %d" % (ph, imgid, len(t), MAX_LEN))
        out[str(imgid)] = ids
    return out


def constraint_shape(constraints):
    """(C, Lc) of a whole run: one shape for every batch, so that the token steps are captured once."""
    return (max([len(p) for p in constraints.values()] + [1]), max([len(t) for p in constraints.values() for t in p] + [1]))


def met_list(mask, phrases):
    return [bool((int(mask) >> c) & 1) for c in range(len(phrases))]


def special_ids(vocab):
    """(cls, unk, sep, mask, pad) ids: from the vocabulary, else the ids of vlp_amd.synthetic (those of the BERT cased vocabularies)."""
    if vocab is None:
        return synthetic.CLS_ID, synthetic.UNK_ID, synthetic.SEP_ID, synthetic.MASK_ID, synthetic.PAD_ID
    return tuple(vocab.to_ids(["[CLS]", "[UNK]", "[SEP]", "[MASK]", "[PAD]"]))


def forbid_ignore_set(text, vocab):
    if not text:
        return None
    if vocab is None:
        raise ValueError("--forbid_ignore_word names tokens: it needs a vocabulary (--vocab_file, or a --bert_model directory with vocab.txt)")
    return set(vocab.to_ids(parse_forbid_ignore_word(text)))


def select_images(img_dat, split, dataset, valid_jpgs=None):
    """decode_img2txt.py:189-206: the images of `split` in file order -> [(image_id, store key)]; the store key is the file name's stem.
    valid_jpgs only filters datasets other than coco / flickr30k, as in the reference."""
    if dataset not in ("coco", "cc", "flickr30k"):
        raise ValueError("--dataset must be coco, cc or flickr30k (got %r)" % (dataset,))
    if dataset in ("coco", "flickr30k"):
        valid_jpgs = None
    out = []
    for src in img_dat:
        if src["split"] == split and (valid_jpgs is None or src["filename"] in valid_jpgs):
            name = src["filename"]
            if dataset == "coco":
                imgid = int(name.split("_")[2][:-4])
            elif dataset == "cc":
                imgid = int(src["imgid"])
            else:
                imgid = int(name.split(".")[0])
            out.append((imgid, os.path.splitext(os.path.basename(name))[0]))
    return out


def caption_of(w_ids, vocab, sep_id, pad_id):
    """decode_img2txt.py:250-257: cut at the first [SEP] / [PAD], merge the word pieces; without a vocabulary the ids themselves."""
    kept = []
    for t in w_ids:
        if t in (sep_id, pad_id):
            break
        kept.append(int(t))
    if vocab is None:
        return " ".join(str(t) for t in kept)
    return " ".join(merge_word_pieces([vocab.tokens[t] if 0 <= t < len(vocab) else "[UNK]" for t in kept]))


def output_path(args, ckpt, n_ckpts):
    if not args.output_file:
        return "%s-%s-captions.json" % (os.path.splitext(ckpt)[0], args.split)
    if n_ckpts == 1:
        return args.output_file
    root, ext = os.path.splitext(args.output_file)
    return "%s.%s%s" % (root, os.path.splitext(os.path.basename(ckpt))[0], ext)


# ---- device side -------------------------------------------------------------------------------------------------------
def decoder_inputs(B, Nv, max_tgt_length, new_segment_ids, cls_id, unk_id, sep_id, device):
    """Preprocess4Seq2seqDecoder.__call__ (seq2seq_loader.py:390-429) for B images with max_a_len = Nv, built on the device:
    input_ids [B, Nv+2], token_type_ids / position_ids [B, L], input_mask [B, L, L] with L = Nv + 2 + max_tgt_length."""
    in_len, L = Nv + 2, Nv + 2 + max_tgt_length
    input_ids = torch.full((B, in_len), unk_id, dtype=torch.long, device=device)
    input_ids[:, 0] = cls_id
    input_ids[:, in_len - 1] = sep_id
    seg = torch.full((B, L), 5 if new_segment_ids else 1, dtype=torch.long, device=device)
    seg[:, :in_len] = 4 if new_segment_ids else 0
    pos = torch.arange(L, dtype=torch.long, device=device).unsqueeze(0).expand(B, L).contiguous()
    mask = torch.zeros(L, L, dtype=torch.long, device=device)
    mask[:, :in_len] = 1
    mask[in_len:, in_len:] = torch.tril(torch.ones(max_tgt_length, max_tgt_length, dtype=torch.long, device=device))
    return input_ids, seg, pos, mask.unsqueeze(0).expand(B, L, L).contiguous()


def require_fp16(args):
    if not args.fp16:
        raise NotImplementedError(
            "vlp_amd implements the reference's --fp16 path (fp16 storage, fp32 accumulate) and has no fp32 compute path.  This command line has "
            "no --fp16%s.  Add --fp16." % (": --amp only engages together with --fp16 (decode_img2txt.py:138)" if args.amp else ""))


def build_decoder(args, vocab, state, device):
    require_fp16(args)
    config = model_config(args)
    cls_id, unk_id, sep_id, mask_id, pad_id = special_ids(vocab)
    model = BertForSeq2SeqDecoder(config, mask_word_id=mask_id, num_labels=2, search_beam_size=args.beam_size, length_penalty=args.length_penalty,
                                  eos_id=sep_id, forbid_duplicate_ngrams=args.forbid_duplicate_ngrams,
                                  forbid_ignore_set=forbid_ignore_set(args.forbid_ignore_word, vocab), ngram_size=args.ngram_size, min_len=args.min_len,
                                  enable_butd=args.enable_butd, len_vis_input=args.len_vis_input, n_best=getattr(args, "n_best", 1),
                                  beam_groups=getattr(args, "beam_groups", 1), diversity_penalty=getattr(args, "diversity_penalty", 0.0))
    load_checkpoint_state(model, state)
    model.half()
    model.to(device)
    return model.eval()


def decode_images(model, store, keys, args, vocab, device, constraints=None):
    """Captions of the store rows `keys`, in order.  constraints: per key the image's phrases as id lists (an empty list: none); the
    result is then a list of (caption, met mask)."""
    cls_id, unk_id, sep_id, mask_id, pad_id = special_ids(vocab)
    Nv, bs = args.len_vis_input, args.batch_size
    if store.nv != Nv:
        raise RuntimeError("the packed store holds %d regions per image, --len_vis_input is %d" % (store.nv, Nv))
    feat = torch.empty(bs, Nv, FEAT_DIM, dtype=torch.float16).pin_memory()
    cls = torch.empty(bs, Nv, N_CLS, dtype=torch.float16).pin_memory()
    bbox = torch.empty(bs, Nv, BOX_DIM, dtype=torch.float32).pin_memory()
    input_ids, seg, pos, mask = decoder_inputs(bs, Nv, args.max_tgt_length, args.new_segment_ids, cls_id, unk_id, sep_id, device)
    rows = store.rows(keys)
    captions = []
    with torch.no_grad():
        for i in range(0, len(rows), bs):
            chunk = rows[i:i + bs]
            n = len(chunk)
            chunk = chunk + [chunk[-1]] * (bs - n)                  # a short last batch runs at the full size
            store.gather(chunk, feat.numpy(), cls.numpy(), bbox.numpy())
            img = feat.to(device, non_blocking=True)
            regions = RawRegions(bbox.to(device, non_blocking=True), cls.to(device, non_blocking=True))
            out = model(img, regions, input_ids, seg, pos, mask, task_idx=None, **_batch_constraints(constraints, i, n, bs))
            ids = (out["pred_seq"] if args.beam_size > 1 else out[0]).tolist()       # synchronises: the pinned buffers are free again
            if constraints is None:
                captions.extend(caption_of(w, vocab, sep_id, pad_id) for w in ids[:n])
            else:
                captions.extend(zip((caption_of(w, vocab, sep_id, pad_id) for w in ids[:n]), out["pred_met"].tolist()[:n]))
    return captions


_shape_of_run = {}


def _run_shape(constraints):
    """constraint_shape of a run's per-image list, computed once per list."""
    if _shape_of_run.get("id") != id(constraints):
        _shape_of_run.update(id=id(constraints), shape=constraint_shape({k: p for k, p in enumerate(constraints)}))
    return _shape_of_run["shape"]


def _batch_constraints(constraints, i, n, bs):
    """The model's constraints= keyword for the batch of images i .. i+n-1 (filled up to bs with its last image), at the run's one (C, Lc)."""
    if constraints is None:
        return {}
    from .constrained import pack_constraints
    C, Lc = _run_shape(constraints)
    part = constraints[i:i + n]
    return {"constraints": pack_constraints(part + [part[-1]] * (bs - n), bs, C, Lc)}


def decode_images_nbest(model, store, keys, args, vocab, device, df=None, constraints=None):
    """--n_best N >= 2: per store row of `keys`, in order, (hypotheses, pick).  hypotheses: N dicts {rank, caption, logprob, value, ok[,
    utility]} from the ranked list of the image's beam search (vlp_beam_nbest; nothing but the final read goes to the host); pick: the rank
    --select keeps -- none: 0; logprob: the ok hypothesis with the largest logprob; consensus (df: the table): the hypothesis with the
    largest CIDEr-D against the image's other hypotheses, scored on the device, the rows of rank > 0 that are not ok emptied first.
    Ties go to the lowest rank.  constraints: as decode_images takes them; every hypothesis then also carries its met mask, "met"."""
    from . import consensus as CS
    from .scst import clean_captions
    cls_id, unk_id, sep_id, mask_id, pad_id = special_ids(vocab)
    Nv, bs, N = args.len_vis_input, args.batch_size, args.n_best
    if store.nv != Nv:
        raise RuntimeError("the packed store holds %d regions per image, --len_vis_input is %d" % (store.nv, Nv))
    feat = torch.empty(bs, Nv, FEAT_DIM, dtype=torch.float16).pin_memory()
    cls = torch.empty(bs, Nv, N_CLS, dtype=torch.float16).pin_memory()
    bbox = torch.empty(bs, Nv, BOX_DIM, dtype=torch.float32).pin_memory()
    input_ids, seg, pos, mask = decoder_inputs(bs, Nv, args.max_tgt_length, args.new_segment_ids, cls_id, unk_id, sep_id, device)
    rows = store.rows(keys)
    out = []
    with torch.no_grad():
        for i in range(0, len(rows), bs):
            chunk = rows[i:i + bs]
            n = len(chunk)
            chunk = chunk + [chunk[-1]] * (bs - n)                  # a short last batch runs at the full size
            store.gather(chunk, feat.numpy(), cls.numpy(), bbox.numpy())
            img = feat.to(device, non_blocking=True)
            regions = RawRegions(bbox.to(device, non_blocking=True), cls.to(device, non_blocking=True))
            tr = model(img, regions, input_ids, seg, pos, mask, task_idx=None, **_batch_constraints(constraints, i, n, bs))
            if args.select == "consensus":                          # launched before the read below: no synchronisation of its own
                ok_nb = tr["nbest_ok"].transpose(0, 1).reshape(N * bs).bool()          # sample-major again: rank k of image b = row k*bs + b
                ok_nb[:bs] = True                                   # rank 0 stays as it is
                ids_nb = tr["nbest_seq"].transpose(0, 1).reshape(N * bs, -1)[:, :args.max_tgt_length]
                ids_nb = clean_captions(ids_nb, sep_id, pad_id).masked_fill_(~ok_nb.unsqueeze(1), 0)
                pick, utility = CS.consensus_select_device(ids_nb, N, df)
                pick, utility = pick.tolist(), utility.view(N, bs).tolist()
            ids, logp, val, ok = tr["nbest_seq"].tolist(), tr["nbest_score"].tolist(), tr["nbest_value"].tolist(), tr["nbest_ok"].tolist()
            for b in range(n):                                      # (the rows that pad a short last batch are dropped, their picks too)
                hyps = [{"rank": k, "caption": caption_of(ids[b][k], vocab, sep_id, pad_id), "logprob": logp[b][k], "value": val[b][k],
                         "ok": bool(ok[b][k])} for k in range(N)]
                if constraints is not None:
                    for k, m in enumerate(tr["nbest_met"][b].tolist()):
                        hyps[k]["met"] = m
                k_sel = 0
                if args.select == "consensus":
                    k_sel = pick[b]
                    for k in range(N):
                        hyps[k]["utility"] = utility[k][b]
                elif args.select == "logprob":
                    k_sel = int(CS.first_max([h["logprob"] if h["ok"] else -float("inf") for h in hyps], N)[0])
                out.append((hyps, k_sel))
    return out


def nbest_path(args, ckpt, n_ckpts):
    """--nbest_file, with the checkpoint's name in it when there are several (as output_path does for --output_file)."""
    if n_ckpts == 1:
        return args.nbest_file
    root, ext = os.path.splitext(args.nbest_file)
    return "%s.%s%s" % (root, os.path.splitext(os.path.basename(ckpt))[0], ext)


def _finite(x):
    """json has no -inf: the logprob / value of an empty hypothesis are written as null."""
    return x if x == x and abs(x) != float("inf") else None


def main(argv=None):
    args = parse_args(argv)
    require_fp16(args)
    if args.enable_butd:
        assert args.len_vis_input == 100
    if not args.packed_features:
        raise NotImplementedError("give --packed_features DIR (vlp_amd.data; the reference's h5 files are converted once with pack_from_h5)")
    if not args.model_recover_path:
        raise ValueError("--model_recover_path is required")
    if not torch.cuda.is_available():
        raise RuntimeError("vlp_amd: the decoder runs on the HIP engine only; there is no CPU path")
    device = torch.device("cuda")
    random.seed(args.seed)
    np.random.seed(args.seed)
    torch.manual_seed(args.seed)
    torch.cuda.manual_seed_all(args.seed)

    vocab_file = vocab_path(args)
    vocab = Vocab(vocab_file) if vocab_file else None

    with open(args.src_file, "r", encoding="utf-8") as f:
        img_dat = json.load(f)["images"]
    valid_jpgs = None
    if args.file_valid_jpgs != "" and args.dataset not in ("coco", "flickr30k"):
        with open(args.file_valid_jpgs) as f:
            valid_jpgs = set(json.load(f))
    images = select_images(img_dat, args.split, args.dataset, valid_jpgs)
    store = PackedRegionStore(args.packed_features)
    df = None
    if args.select == "consensus":
        from .sample_img2txt import consensus_doc_freq
        df = consensus_doc_freq(args.consensus_df, args.max_tgt_length, special_ids(vocab)[2])
        logger.info("--consensus_df %s: %d n-grams over %d images", args.consensus_df, len(df), df.n_docs)

    cons = None          # --constraints_file: per image, in order, its phrases as id lists (none for an image without an entry)
    if args.constraints is not None:
        cons = [args.constraints.get(str(imgid), []) for imgid, _ in images]

    def with_met(records, masks):
        if cons is None:
            return records
        return [dict(r, constraints=ph, met=met_list(m, ph)) for r, ph, m in zip(records, cons, masks)]

    ckpts = sorted(glob.glob(args.model_recover_path.strip()))
    if not ckpts:
        raise FileNotFoundError("--model_recover_path %r matches no file" % (args.model_recover_path,))
    results = {}
    for ckpt in ckpts:
        logger.info("***** Recover model: %s *****", ckpt)
        model = build_decoder(args, vocab, torch.load(ckpt, map_location="cpu"), device)
        if args.n_best > 1:
            ranked = decode_images_nbest(model, store, [key for _, key in images], args, vocab, device, df=df, constraints=cons)
            if args.nbest_file:          # every hypothesis that is one: rank 0 always, the others when ok
                with open(nbest_path(args, ckpt, len(ckpts)), "w") as f:
                    json.dump([dict({"image_id": imgid, "rank": h["rank"], "caption": h["caption"], "logprob": _finite(h["logprob"]),
                                     "value": _finite(h["value"])}, **dict(({"utility": h["utility"]} if "utility" in h else {}),
                                                                           **({"constraints": cons[n], "met": met_list(h["met"], cons[n])}
                                                                              if cons is not None else {})))
                               for n, ((imgid, _), (hyps, _)) in enumerate(zip(images, ranked)) for h in hyps if h["ok"] or h["rank"] == 0], f)
            if args.select == "none":
                predictions = [{"image_id": imgid, "caption": hyps[0]["caption"]} for (imgid, _), (hyps, _) in zip(images, ranked)]
            else:
                predictions = [{"image_id": imgid, "caption": hyps[k]["caption"], "rank": k, "logprob": _finite(hyps[k]["logprob"]),
                                "utility": hyps[k].get("utility")} for (imgid, _), (hyps, k) in zip(images, ranked)]
            predictions = with_met(predictions, [hyps[k].get("met", 0) if args.select != "none" else hyps[0].get("met", 0) for hyps, k in ranked])
        else:
            captions = decode_images(model, store, [key for _, key in images], args, vocab, device, constraints=cons)
            if cons is not None:
                captions, masks = [c for c, _ in captions], [m for _, m in captions]
            predictions = with_met([{"image_id": imgid, "caption": cap} for (imgid, _), cap in zip(images, captions)], masks if cons is not None else None)
        out = output_path(args, ckpt, len(ckpts))
        with open(out, "w") as f:
            json.dump(predictions, f)
        logger.info("wrote %d captions to %s", len(predictions), out)
        results[ckpt] = predictions
        del model
    return results


if __name__ == "__main__":
    logging.basicConfig(format="%(asctime)s - %(levelname)s - %(name)s -   %(message)s", datefmt="%m/%d/%Y %H:%M:%S", level=logging.INFO)
    main()
