"""Build the CIDEr-D document-frequency table of a training set once (vlp_amd.scst.DocFreq) and save it for --scst_df PATH:

    python -m vlp_amd.cider_df --token_file F --max_len_b 20 [--sep_id 102] --out df.npz

F is the training entry's --token_file: a json list of [image id, [caption token ids]].  A document is one image -- all its captions in F, each
cut to --max_len_b tokens and closed with [SEP] (then 0), the form the SCST reward sees.  --max_len_b and --sep_id must be the training
run's: the entry script refuses a table built for others."""
import argparse
import json
import sys

from . import synthetic
from .scst import DocFreq


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--token_file", required=True, help="json list of [image id, [caption token ids]]")
    ap.add_argument("--max_len_b", type=int, required=True, help="the training run's --max_len_b (COCO: 20)")
    ap.add_argument("--sep_id", type=int, default=synthetic.SEP_ID, help="id of [SEP] (default %(default)s)")
    ap.add_argument("--out", required=True, help="the .npz to write")
    a = ap.parse_args(argv)
    with open(a.token_file) as f:
        examples = json.load(f)
    if not examples or any(len(e) != 2 for e in examples):
        ap.error("--token_file %s must hold caption examples [image id, [caption token ids]]" % a.token_file)
    table = DocFreq.from_examples(examples, a.max_len_b, a.sep_id)
    table.save(a.out)
    print("%s: %d n-grams over %d images (%d captions), max_len_b %d, sep_id %d" % (a.out, len(table), table.n_docs, len(examples), a.max_len_b, a.sep_id))
    return 0


if __name__ == "__main__":
    sys.exit(main())
