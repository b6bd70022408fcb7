"""Score given captions under a fine-tuned checkpoint: held-out log-likelihood and perplexity, token-level top-1 / top-5 accuracy and
entropy, and the model's choice among several captions of an image.

    python -m vlp_amd.score_img2txt --bert_model DIR --model_recover_path out/model.30.bin --packed_features STORE --token_file val_tokens.json \\
        --fp16 --enable_butd --new_segment_ids --batch_size 64 --output_file scores.json --summary_file summary.json

The model and data flags are vlp_amd.decode_img2txt's.  The captions come pre-tokenised from --token_file, the training entry's format: a json
list of [store key, [caption token ids]].  Every example is one row of a batch: its image's regions, the caption teacher-forced behind them,
all positions scored by one forward (BertForSeq2SeqDecoder.score; vlp_amd.caption_score has the counting rule: a caption of n tokens is
scored over its tokens and the closing [SEP], one of --max_tgt_length tokens or more is cut and flagged).  A short last batch is filled up
with its last row (and the extra rows dropped), so every batch runs the same launches.

  --src_file F --split S (both or neither) keep the examples whose key is an image of the split and give the records the integer image id
      vlp_amd.decode_img2txt writes; without them every example is scored and its key is the id.
  --output_file receives one record per caption, in input order:
      {"image_id", "index" (the caption's number within its image), "tokens" (counted positions), "truncated", "logprob" (their sum), "ppl"
       (exp(-logprob / tokens)), "top1" / "top5" (how many of them the model ranked first / among its first five), "entropy" (the mean
       entropy of the model's distribution over them), "caption" (decode_img2txt's caption_of: cut at [SEP], word pieces merged)}
  --summary_file receives (and the log shows) {"captions", "tokens", "logprob", "ppl", "top1", "top5", "entropy"} over all of them: ppl =
      exp(-sum logprob / sum tokens), top1 / top5 the shares of all counted positions.  Sums are taken on the host in fp64.
  --select likelihood [--length_norm {none,mean}] writes one {"image_id", "caption", "index", "logprob"} record per image to --output_file
      instead, which python -m vlp_amd.eval_captions reads as it stands: the caption with the largest log-probability (none) or the
      largest log-probability per counted token (mean), ties to the lowest index; --samples_file then receives the per-caption records.
"""
import glob
import json
import logging
import os

import torch

from . import caption_score as CS
from . import decode_img2txt as D
from .data import PackedRegionStore, FEAT_DIM, BOX_DIM, examples_have_answers
from .input_prep import RawRegions, N_CLS
from .run_img2txt_dist import read_examples

logger = logging.getLogger(__name__)


def parse_args(argv=None):
    """The parsed command line, or the parser's error exit."""
    p = D.build_parser()
    p.description = "Score given captions under a fine-tuned checkpoint."
    p.set_defaults(src_file=None, split=None)
    p.add_argument("--token_file", default="", help="json list of [store key, [caption token ids]] (the training entry's format); required")
    p.add_argument("--summary_file", default=None, metavar="PATH", help="write the corpus figures {captions, tokens, logprob, ppl, top1, top5, entropy} here")
    p.add_argument("--select", choices=("none", "likelihood"), default="none",
                   help="'likelihood': write one caption per image, the most probable of those given (default none: every caption's record)")
    p.add_argument("--length_norm", choices=("none", "mean"), default=None,
                   help="with --select likelihood: compare total log-probabilities (none, the default) or log-probabilities per counted token (mean)")
    p.add_argument("--samples_file", default=None, metavar="PATH", help="with --select likelihood: write the per-caption records here")
    a = p.parse_args(argv)
    if not a.fp16:
        p.error("vlp_amd implements the --fp16 path only (fp16 storage, fp32 accumulate): add --fp16")
    if not a.packed_features:
        p.error("--packed_features DIR is required (a vlp_amd.data packed region store; the reference's h5 files are converted once with pack_from_h5)")
    if not a.token_file:
        p.error("--token_file FILE is required: the captions to score, a json list of [store key, [caption token ids]]")
    if not a.model_recover_path:
        p.error("--model_recover_path is required")
    if a.length_norm is not None and a.select == "none":
        p.error("--length_norm %s says how --select likelihood compares captions: it needs --select likelihood" % a.length_norm)
    if a.samples_file and a.select == "none":
        p.error("--samples_file %s receives the per-caption records next to a selection: it needs --select likelihood (without one they go to "
                "--output_file)" % a.samples_file)
    if bool(a.src_file) != bool(a.split):
        p.error("--src_file and --split go together: the image list and the split of it whose captions are scored")
    a.length_norm = a.length_norm or "none"
    return a


def load_captions(args):
    """--token_file (and --src_file / --split) -> [(image id, store key, token ids)] in input order; a VQA file is refused."""
    examples = read_examples(args.token_file)
    if not examples:
        raise ValueError("--token_file %s holds no examples" % args.token_file)
    if examples_have_answers(examples):
        raise ValueError("--token_file %s holds VQA examples (questions with answers); captions are scored from [store key, [caption token ids]]"
                         % args.token_file)
    images = None
    if args.src_file:
        with open(args.src_file, "r", encoding="utf-8") as f:
            images = D.select_images(json.load(f)["images"], args.split, args.dataset)
    return CS.filter_examples(examples, images)


def score_captions(model, store, captions, args, vocab, device):
    """The per-caption records of `captions` [(image id, store key, token ids)], in order."""
    cls_id, unk_id, sep_id, mask_id, pad_id = D.special_ids(vocab)
    Nv, bs, T = args.len_vis_input, args.batch_size, args.max_tgt_length
    if store.nv != Nv:
        raise RuntimeError("the packed store holds %d regions per image, --len_vis_input is %d" % (store.nv, Nv))
    missing = [key for _, key, _ in captions if str(key) not in store.row_of]
    if missing:
        raise KeyError("--token_file %s: key %r is not in the packed store %s (%d examples in all)" % (args.token_file, missing[0],
                                                                                                    args.packed_features, len(missing)))
    feat = torch.empty(bs, Nv, FEAT_DIM, dtype=torch.float16).pin_memory()
    cls = torch.empty(bs, Nv, N_CLS, dtype=torch.float16).pin_memory()
    bbox = torch.empty(bs, Nv, BOX_DIM, dtype=torch.float32).pin_memory()
    input_ids, seg, pos, mask = D.decoder_inputs(bs, Nv, T, args.new_segment_ids, cls_id, unk_id, sep_id, device)
    rows = store.rows([key for _, key, _ in captions])
    index = CS.caption_indices([imgid for imgid, _, _ in captions])
    records = []
    with torch.no_grad():
        for i in range(0, len(rows), bs):
            chunk, toks = rows[i:i + bs], [t for _, _, t in captions[i:i + bs]]
            n = len(chunk)
            chunk, toks = chunk + [chunk[-1]] * (bs - n), toks + [toks[-1]] * (bs - n)      # a short last batch runs at the full size
            store.gather(chunk, feat.numpy(), cls.numpy(), bbox.numpy())
            img = feat.to(device, non_blocking=True)
            regions = RawRegions(bbox.to(device, non_blocking=True), cls.to(device, non_blocking=True))
            logp, ent, rank, _, counted = (t.cpu().numpy() for t in model.score(img, regions, input_ids, seg, pos, mask, toks))
            for b in range(n):                                      # (the .cpu() above synchronised: the pinned buffers are free again)
                imgid, _, t = captions[i + b]
                rec = {"image_id": imgid, "index": index[i + b], "truncated": bool(CS.is_truncated(len(t), T))}
                rec.update(CS.caption_record(logp[b], ent[b], rank[b], counted[b]))
                rec["caption"] = D.caption_of(t[:T], vocab, sep_id, pad_id)
                records.append(rec)
    return records


def _path(path, ckpt, n_ckpts):
    """A file name with the checkpoint's name in it when there are several (decode_img2txt.output_path's rule)."""
    if n_ckpts == 1 or not path:
        return path
    root, ext = os.path.splitext(path)
    return "%s.%s%s" % (root, os.path.splitext(os.path.basename(ckpt))[0], ext)


def main(argv=None):
    args = parse_args(argv)
    if args.enable_butd:
        assert args.len_vis_input == 100
    if not torch.cuda.is_available():
        raise RuntimeError("vlp_amd: the decoder runs on the HIP engine only; there is no CPU path")
    device = torch.device("cuda")
    vocab_file = args.vocab_file
    if vocab_file is None and os.path.isdir(args.bert_model) and os.path.exists(os.path.join(args.bert_model, "vocab.txt")):
        vocab_file = os.path.join(args.bert_model, "vocab.txt")
    vocab = D.Vocab(vocab_file) if vocab_file else None
    captions = load_captions(args)
    store = PackedRegionStore(args.packed_features)
    ckpts = sorted(glob.glob(args.model_recover_path.strip()))
    if not ckpts:
        raise FileNotFoundError("--model_recover_path %r matches no file" % (args.model_recover_path,))
    results = {}
    for ckpt in ckpts:
        logger.info("***** Recover model: %s *****", ckpt)
        model = D.build_decoder(args, vocab, torch.load(ckpt, map_location="cpu"), device)
        records = score_captions(model, store, captions, args, vocab, device)
        summary = CS.summarize(records)
        logger.info("%s: %s", ckpt, json.dumps(summary, sort_keys=True))
        out = D.output_path(args, ckpt, len(ckpts)) if args.output_file else "%s-scores.json" % os.path.splitext(ckpt)[0]
        written = records
        if args.select == "likelihood":
            written = CS.select_likelihood(records, args.length_norm)
            if args.samples_file:
                with open(_path(args.samples_file, ckpt, len(ckpts)), "w") as f:
                    json.dump(records, f)
        with open(out, "w") as f:
            json.dump(written, f)
        if args.summary_file:
            with open(_path(args.summary_file, ckpt, len(ckpts)), "w") as f:
                json.dump(summary, f)
        logger.info("wrote %d records to %s", len(written), out)
        results[ckpt] = {"records": records, "summary": summary, "written": written}
        del model
    return results


if __name__ == "__main__":
    logging.basicConfig(format="%(asctime)s - %(levelname)s - %(name)s -   %(message)s", datefmt="%m/%d/%Y %H:%M:%S", level=logging.INFO)
    main()
