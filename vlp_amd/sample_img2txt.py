"""Sampled captions from a fine-tuned checkpoint: temperature, top-k and nucleus (top-p) sampling, several captions per image.

    python -m vlp_amd.sample_img2txt --bert_model DIR --model_recover_path 'out/model.*.bin' --packed_features STORE \\
        --src_file dataset_coco.json --split val --fp16 --enable_butd --new_segment_ids \\
        --temperature 0.8 --top_k 50 --top_p 0.9 --num_samples 5 --seed 7

The command line is vlp_amd.decode_img2txt's (same store, vocabulary, image list and checkpoint handling, imported from there) plus
  --temperature T   logits are divided by T before the softmax (default 1)
  --top_k K         only the K largest logits of a step can be drawn, ties at the K-th included (default 0: all)
  --top_p P         then only the smallest set of largest logits whose probability reaches P (default 1: all)
  --num_samples N   captions per image, 1..16 (default 1); batch_size * num_samples sequences are decoded together, at most 1024
Every token is drawn on the device (vlp_sample_rows_filtered; with the defaults, the unfiltered sampler).  --seed selects the draws: the same
seed writes the same file.  Beam search and n-gram blocking are decode_img2txt's business: --beam_size > 1 and --forbid_duplicate_ngrams are refused.

--output_file (default <checkpoint>-<split>-samples.json) receives one record per (image, sample), ordered by image (input order), then sample:
    {"image_id": ..., "sample": k, "caption": "...", "logprob": sum of the log-probabilities of the drawn tokens up to and including the first [SEP]}
the log-probabilities being those of the distribution drawn from (tempered, truncated, renormalised).

  --select {none,consensus,logprob}   turn the N samples of an image into ONE caption (needs --num_samples >= 2; default none: the above)
      consensus   the sample that agrees most with the image's other samples: the largest CIDEr-D against them as references, scored on the
                  device (vlp_amd.consensus, vlp_cider_d_consensus) with the document frequencies of --consensus_df PATH, a table written
                  by `python -m vlp_amd.cider_df` for this --max_tgt_length and vocabulary.  No references are needed
      logprob     the sample with the largest "logprob"
  Ties go to the lowest sample index.  --output_file (default <checkpoint>-<split>-selected.json) then receives one record per image in input
  order, which `python -m vlp_amd.eval_captions` reads as it stands:
      {"image_id": ..., "caption": "...", "sample": k, "logprob": ..., "utility": CIDEr-D against the other samples, null for logprob}
  --samples_file PATH additionally receives all samples in the record format above, plus "utility" under consensus.
"""
import glob
import json
import logging
import os

import torch

from . import decode_img2txt as D
from .data import PackedRegionStore, FEAT_DIM, BOX_DIM
from .input_prep import RawRegions, N_CLS

logger = logging.getLogger(__name__)

MAX_SAMPLES = 16            # Engine.decode_sample_group: 1..16 samples per image,
MAX_SEQUENCES = 1024        # at most 1024 sequences per call
SELECTIONS = ("none", "consensus", "logprob")


def build_parser():
    p = D.build_parser()
    p.description = "Write sampled captions (temperature / top-k / top-p) for the images of one split from a fine-tuned checkpoint."
    p.add_argument("--temperature", type=float, default=1.0, help="divide the logits by this before the softmax (> 0)")
    p.add_argument("--top_k", type=int, default=0, help="draw among the K largest logits only, ties included (0: all)")
    p.add_argument("--top_p", type=float, default=1.0, help="draw among the smallest set of largest logits whose probability reaches P, 0 < P <= 1 (1: all)")
    p.add_argument("--num_samples", type=int, default=1, help="captions per image, 1..%d" % MAX_SAMPLES)
    return p


def add_selection_flags(p):
    """The flags that turn the samples of an image into one caption, on top of build_parser()'s (the sampling controls alone)."""
    p.add_argument("--select", choices=SELECTIONS, default="none",
                   help="write one caption per image: 'consensus' keeps the sample with the largest CIDEr-D against the image's other samples "
                        "(scored on the device, needs --consensus_df), 'logprob' the most probable sample; needs --num_samples >= 2 (default none: "
                        "every sample is written)")
    p.add_argument("--consensus_df", default=None, metavar="PATH",
                   help="--select consensus: the document-frequency table, written by `python -m vlp_amd.cider_df` with --max_len_b equal to "
                        "--max_tgt_length")
    p.add_argument("--samples_file", default=None, metavar="PATH", help="with --select: also write all samples here (with their utility under consensus)")
    return p


def parse_args(argv=None):
    """The parsed command line, or the parser's error exit: ranges, the options that belong to decode_img2txt, the decoder's sequence limit."""
    p = add_selection_flags(build_parser())
    a = p.parse_args(argv)
    if not (0.0 < a.temperature < float("inf")):
        p.error("--temperature must be finite and > 0 (got %r)" % a.temperature)
    if a.top_k < 0 or a.top_k >= 1 << 31:
        p.error("--top_k must be >= 0 (got %d)" % a.top_k)
    if not (0.0 < a.top_p <= 1.0):
        p.error("--top_p must be in (0, 1] (got %r)" % a.top_p)
    if not (1 <= a.num_samples <= MAX_SAMPLES):
        p.error("--num_samples must be in 1..%d (got %d)" % (MAX_SAMPLES, a.num_samples))
    if a.beam_size > 1:
        p.error("--beam_size %d: this tool samples; beam search is python -m vlp_amd.decode_img2txt" % a.beam_size)
    if a.forbid_duplicate_ngrams:
        p.error("--forbid_duplicate_ngrams blocks n-grams in a beam search (python -m vlp_amd.decode_img2txt); sampled captions are not blocked")
    if a.batch_size < 1 or a.batch_size * a.num_samples > MAX_SEQUENCES:
        p.error("--batch_size %d x --num_samples %d = %d sequences per decode; the sampled decode takes 1..%d: lower --batch_size"
                % (a.batch_size, a.num_samples, a.batch_size * a.num_samples, MAX_SEQUENCES))
    if a.select != "none" and a.num_samples < 2:
        p.error("--select %s chooses among the samples of an image: it needs --num_samples >= 2 (got %d)" % (a.select, a.num_samples))
    if a.select == "consensus" and not a.consensus_df:
        p.error("--select consensus needs --consensus_df PATH (a table written by python -m vlp_amd.cider_df)")
    if a.select != "consensus" and a.consensus_df:
        p.error("--consensus_df %s needs --select consensus (it holds the document frequencies of the consensus score)" % a.consensus_df)
    if a.select == "none" and a.samples_file:
        p.error("--samples_file %s needs --select (without a selection --output_file holds the samples)" % a.samples_file)
    return a


def consensus_doc_freq(path, max_tgt_length, sep_id):
    """--consensus_df: a saved table, refused when it was built for another caption format than this run's."""
    from .scst import DocFreq
    if not os.path.isfile(path):
        raise ValueError("--consensus_df: the path of a saved table; there is no file %s" % path)
    table = DocFreq.load(path)
    if (table.max_len_b, table.sep_id) != (max_tgt_length, sep_id):
        raise ValueError("--consensus_df %s was built for --max_len_b %s and [SEP] id %s; this run has --max_tgt_length %d and [SEP] id %d: rebuild it "
                         "with python -m vlp_amd.cider_df" % (path, table.max_len_b, table.sep_id, max_tgt_length, sep_id))
    return table


def sequence_logprob(ids, logps, sep_id):
    """Sum of the step log-probabilities up to and including the first [SEP] (all steps when there is none)."""
    n = ids.index(sep_id) + 1 if sep_id in ids else len(ids)
    return float(sum(logps[:n]))


def sample_images(model, store, keys, args, vocab, device, df=None, picked=None):
    """[(caption, logprob)] * num_samples for each of the store rows `keys`, in order.  With --select, `picked` (a list) receives per image
    (k, utilities): the selected sample and, under consensus (df: the table), the num_samples utilities, else None."""
    from . import consensus as CS
    from .scst import clean_captions
    select = getattr(args, "select", "none")
    cls_id, unk_id, sep_id, mask_id, pad_id = D.special_ids(vocab)
    Nv, bs, Ks = args.len_vis_input, args.batch_size, args.num_samples
    if store.nv != Nv:
        raise RuntimeError("the packed store holds %d regions per image, --len_vis_input is %d" % (store.nv, Nv))
    feat = torch.empty(bs, Nv, FEAT_DIM, dtype=torch.float16).pin_memory()
    cls = torch.empty(bs, Nv, N_CLS, dtype=torch.float16).pin_memory()
    bbox = torch.empty(bs, Nv, BOX_DIM, dtype=torch.float32).pin_memory()
    input_ids, seg, pos, mask = D.decoder_inputs(bs, Nv, args.max_tgt_length, args.new_segment_ids, cls_id, unk_id, sep_id, device)
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
            ids, logp = model(img, regions, input_ids, seg, pos, mask, task_idx=None, sample_mode="sample", n_samples=Ks,
                              temperature=args.temperature, top_k=args.top_k, top_p=args.top_p)
            if select == "consensus":                               # launched before the read below: no synchronisation of its own
                pick, utility = CS.consensus_select_device(clean_captions(ids, sep_id, pad_id), Ks, df)
            ids, logp = ids.view(Ks, bs, -1).tolist(), logp.view(Ks, bs, -1).tolist()      # sample-major; synchronises: the pinned buffers are free again
            if select == "consensus":
                pick, utility = pick.tolist(), utility.view(Ks, bs).tolist()
            for b in range(n):                                      # (the rows that pad a short last batch are dropped, their picks too)
                out.append([(D.caption_of(ids[k][b], vocab, sep_id, pad_id), sequence_logprob(ids[k][b], logp[k][b], sep_id)) for k in range(Ks)])
                if select == "consensus":
                    picked.append((pick[b], [utility[k][b] for k in range(Ks)]))
                elif select == "logprob":
                    picked.append((int(CS.select_by_logprob([lp for _, lp in out[-1]], Ks)[0]), None))
    return out


def output_path(args, ckpt, n_ckpts):
    if not args.output_file:
        return "%s-%s-%s.json" % (os.path.splitext(ckpt)[0], args.split, "samples" if args.select == "none" else "selected")
    return D.output_path(args, ckpt, n_ckpts)


def samples_path(args, ckpt, n_ckpts):
    """--samples_file, with the checkpoint's name in it when there are several (as D.output_path does for --output_file)."""
    if n_ckpts == 1:
        return args.samples_file
    root, ext = os.path.splitext(args.samples_file)
    return "%s.%s%s" % (root, os.path.splitext(os.path.basename(ckpt))[0], ext)


def main(argv=None):
    args = parse_args(argv)
    D.require_fp16(args)
    if args.enable_butd:
        assert args.len_vis_input == 100
    if not args.packed_features:
        raise NotImplementedError("give --packed_features DIR (vlp_amd.data; the reference's h5 files are converted once with pack_from_h5)")
    if not args.model_recover_path:
        raise ValueError("--model_recover_path is required")
    if not torch.cuda.is_available():
        raise RuntimeError("vlp_amd: the decoder runs on the HIP engine only; there is no CPU path")
    device = torch.device("cuda")

    vocab_file = args.vocab_file
    if vocab_file is None and os.path.isdir(args.bert_model) and os.path.exists(os.path.join(args.bert_model, "vocab.txt")):
        vocab_file = os.path.join(args.bert_model, "vocab.txt")
    vocab = D.Vocab(vocab_file) if vocab_file else None

    with open(args.src_file, "r", encoding="utf-8") as f:
        img_dat = json.load(f)["images"]
    valid_jpgs = None
    if args.file_valid_jpgs != "" and args.dataset not in ("coco", "flickr30k"):
        with open(args.file_valid_jpgs) as f:
            valid_jpgs = set(json.load(f))
    images = D.select_images(img_dat, args.split, args.dataset, valid_jpgs)
    store = PackedRegionStore(args.packed_features)
    df = None
    if args.select == "consensus":
        df = consensus_doc_freq(args.consensus_df, args.max_tgt_length, D.special_ids(vocab)[2])
        logger.info("--consensus_df %s: %d n-grams over %d images", args.consensus_df, len(df), df.n_docs)

    ckpts = sorted(glob.glob(args.model_recover_path.strip()))
    if not ckpts:
        raise FileNotFoundError("--model_recover_path %r matches no file" % (args.model_recover_path,))
    results = {}
    for ckpt in ckpts:
        logger.info("***** Recover model: %s *****", ckpt)
        model = D.build_decoder(args, vocab, torch.load(ckpt, map_location="cpu"), device)
        model.engine.base_seed, model.engine.step_seed = int(args.seed), 0          # the draws are a function of --seed alone
        picked = []
        drawn = sample_images(model, store, [key for _, key in images], args, vocab, device, df=df, picked=picked)
        records = [{"image_id": imgid, "sample": k, "caption": cap, "logprob": lp}
                   for (imgid, _), samples in zip(images, drawn) for k, (cap, lp) in enumerate(samples)]
        out = output_path(args, ckpt, len(ckpts))
        if args.select != "none":
            Ks = args.num_samples
            if args.select == "consensus":
                for i, (_, utilities) in enumerate(picked):
                    for k in range(Ks):
                        records[i * Ks + k]["utility"] = utilities[k]
            if args.samples_file:
                with open(samples_path(args, ckpt, len(ckpts)), "w") as f:
                    json.dump(records, f)
            samples = records
            records = [{"image_id": samples[i * Ks + k]["image_id"], "caption": samples[i * Ks + k]["caption"], "sample": k,
                        "logprob": samples[i * Ks + k]["logprob"], "utility": samples[i * Ks + k].get("utility")} for i, (k, _) in enumerate(picked)]
        with open(out, "w") as f:
            json.dump(records, f)
        logger.info("wrote %d %s captions of %d images to %s", len(records), "sampled" if args.select == "none" else "selected", len(images), out)
        results[ckpt] = records
        del model
    return results


if __name__ == "__main__":
    logging.basicConfig(format="%(asctime)s - %(levelname)s - %(name)s -   %(message)s", datefmt="%m/%d/%Y %H:%M:%S", level=logging.INFO)
    main()
