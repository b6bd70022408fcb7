"""Score a predictions file: corpus BLEU-1..4, ROUGE-L and CIDEr of the captions python -m vlp_amd.decode_img2txt wrote.

    python -m vlp_amd.eval_captions --predictions out/model.30-val-captions.json --src_file dataset_coco.json --split val --dataset coco

  * references: `sentences[].tokens` of the split's images in --src_file (Karpathy's lower-cased, punctuation-free tokens); the images are
    selected like the decoder selects them (decode_img2txt.select_images);
  * a predicted caption is lower-cased and split on whitespace, and the tokens of coco-caption's punctuation list are dropped
    (caption_metrics.tokenize_caption);
  * every prediction must name an image of the split, no image id may occur twice; scoring and document frequencies cover the predicted
    images only, as COCOEvalCap does;
  * --metrics_on device (the default) scores with the vlp_caption_eval kernels, an image that does not fit them (a string of more than 64
    words, more than 8 references) on the host against the same table: "scored_on_host" counts those images, whatever --metrics_on says;
    --metrics_on host scores every image on the host and needs no GPU;
  * prints and writes (--output_file) {"Bleu_1".."Bleu_4", "ROUGE_L", "CIDEr", "images", "scored_on_host"}; --per_image_file gets
    [{"image_id", "bleu_stats", "ROUGE_L", "CIDEr"}, ...] in the order of the predictions.

Departure from the reference's language_eval: the Java pipeline runs PTBTokenizer over the raw captions of both sides.  Given the same tokens
the three metrics are coco-caption's (vlp_amd/caption_metrics.py says how they are defined); the tokenisation here is the rule above, so
figures can differ from the Java pipeline's.  Nobody has measured by how much.  METEOR and SPICE are out of scope.
"""
import argparse
import json
import sys

from .caption_metrics import METRICS, CaptionMetrics, tokenize_caption


def build_parser():
    p = argparse.ArgumentParser(description="BLEU-1..4, ROUGE-L and CIDEr of a predictions file against the references of one split.")
    p.add_argument("--predictions", required=True, help='[{"image_id", "caption"}, ...] as decode_img2txt writes it')
    p.add_argument("--src_file", required=True, help="the dataset's Karpathy-split json (dataset_coco.json)")
    p.add_argument("--split", default="val")
    p.add_argument("--dataset", default="coco")
    p.add_argument("--metrics_on", default="device", choices=("device", "host"))
    p.add_argument("--output_file", default=None, help="where the corpus values go (json)")
    p.add_argument("--per_image_file", default=None, help="where the per-image values go (json)")
    return p


def references_of(src_file, split, dataset):
    """{image_id: [word lists]} of the split's images, from sentences[].tokens."""
    from .decode_img2txt import select_images
    with open(src_file, "r", encoding="utf-8") as f:
        img_dat = json.load(f)["images"]
    in_split = [src for src in img_dat if src["split"] == split]
    ids = select_images(in_split, split, dataset)
    refs = {}
    for (image_id, _), src in zip(ids, in_split):
        if image_id in refs:
            raise ValueError("%s: image id %d occurs twice in split %r" % (src_file, image_id, split))
        refs[image_id] = [[str(w) for w in s["tokens"]] for s in src["sentences"]]
    return refs


def load_predictions(path, refs):
    with open(path, "r", encoding="utf-8") as f:
        preds = json.load(f)
    ids, hyps = [], []
    seen = set()
    for p in preds:
        image_id = int(p["image_id"])
        if image_id not in refs:
            raise ValueError("%s: image id %d is not an image of the split" % (path, image_id))
        if image_id in seen:
            raise ValueError("%s: image id %d occurs twice" % (path, image_id))
        seen.add(image_id)
        ids.append(image_id)
        hyps.append(tokenize_caption(p["caption"]))
    if not ids:
        raise ValueError("%s: no predictions" % path)
    return ids, hyps


def evaluate(args):
    refs = references_of(args.src_file, args.split, args.dataset)
    ids, hyps = load_predictions(args.predictions, refs)
    return ids, CaptionMetrics().score([refs[i] for i in ids], hyps, on=args.metrics_on)


def main(argv=None):
    args = build_parser().parse_args(argv)
    ids, res = evaluate(args)
    out = {k: res[k] for k in METRICS + ("images", "scored_on_host")}
    print(json.dumps(out, sort_keys=True))
    if args.output_file:
        with open(args.output_file, "w") as f:
            json.dump(out, f, indent=2, sort_keys=True)
    if args.per_image_file:
        per = res["per_image"]
        rows = [{"image_id": i, "bleu_stats": [int(v) for v in per["bleu_stats"][n]], "ROUGE_L": float(per["ROUGE_L"][n]), "CIDEr": float(per["CIDEr"][n])}
                for n, i in enumerate(ids)]
        with open(args.per_image_file, "w") as f:
            json.dump(rows, f)
    return out


if __name__ == "__main__":
    main(sys.argv[1:])
