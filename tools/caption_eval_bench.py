"""Scoring a split's captions on the host against the device: vlp_amd.caption_metrics.CaptionMetrics.score(on="host") and (on="device"), end
to end -- vocabulary, document-frequency table over the evaluated images, scoring (on the device: chunks of 1024 images through
vlp_caption_eval), reduction -- wall time around a synchronise.

    python tools/caption_eval_bench.py [--images 5000 40504] [--rounds 3] [--out profiles/caption_eval.json]

The corpus is seeded: `images` images with 5 references of 8..20 words each over a 2000-word vocabulary with a Zipf-like distribution (T = 21
rows would hold every string); a hypothesis is a copy of one reference with 30 % of its words redrawn.  Every figure comes from a child process
of its own (the device one scores a 16-image corpus first, so that loading the code objects is not timed), the two variants alternate, and
every child runs under its own time limit; a child that fails or runs out of time ends the run.  The record goes under the "timing" key of
--out, next to what is there.  No speed is asserted: this records what is measured."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VOCAB, REFS, MIN_LEN, MAX_LEN = 2000, 5, 8, 20


def corpus(images, seed=0):
    rng = np.random.RandomState(seed)
    p = 1.0 / np.arange(1, VOCAB + 1)
    p /= p.sum()
    lens = rng.randint(MIN_LEN, MAX_LEN + 1, size=(images, REFS))
    words = rng.choice(VOCAB, size=int(lens.sum()), p=p) + 1
    redraw = rng.choice(VOCAB, size=(images, MAX_LEN), p=p) + 1
    refs, hyps, at = [], [], 0
    for i in range(images):
        rs = []
        for r in range(REFS):
            rs.append([int(w) for w in words[at:at + lens[i, r]]])
            at += lens[i, r]
        h = list(rs[rng.randint(REFS)])
        for j in np.flatnonzero(rng.rand(len(h)) < 0.3):
            h[j] = int(redraw[i, j])
        refs.append(rs)
        hyps.append(h)
    return refs, hyps


def child(on, images):
    import torch
    from vlp_amd.caption_metrics import CaptionMetrics
    refs, hyps = corpus(images)
    m = CaptionMetrics()
    if on == "device":
        m.score(*corpus(16, seed=1), on="device")
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = m.score(refs, hyps, on=on)
    if on == "device":
        torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(json.dumps(dict(on=on, images=images, seconds=dt, scored_on_host=out["scored_on_host"], Bleu_4=out["Bleu_4"], ROUGE_L=out["ROUGE_L"],
                          CIDEr=out["CIDEr"])), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, nargs="+", default=[5000, 40504])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "caption_eval.json"))
    ap.add_argument("--child", default=None, choices=("host", "device"))
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.images[0])
    runs = []
    for images in a.images:
        limit = 60 + images // 50                                    # seconds per child: generous for the host scorer, still an end
        t = {"host": [], "device": []}
        values = {}
        for _ in range(a.rounds):
            for on in ("host", "device"):                            # alternating, so that both see the same neighbours on the box
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", on, "--images", str(images)], capture_output=True, text=True,
                                   timeout=limit, cwd=ROOT)
                if r.returncode != 0:
                    print(r.stdout + r.stderr, file=sys.stderr)
                    raise SystemExit("the %s child for %d images ended with %d: nothing more is started" % (on, images, r.returncode))
                rec = json.loads(r.stdout.strip().splitlines()[-1])
                print(json.dumps(rec, sort_keys=True), flush=True)
                t[on].append(rec["seconds"])
                values[on] = rec
        run = dict(images=images, refs=REFS, vocabulary=VOCAB, rounds=a.rounds, host_seconds=t["host"], device_seconds=t["device"],
                   host_seconds_median=float(np.median(t["host"])), device_seconds_median=float(np.median(t["device"])),
                   bleu4_equal=values["host"]["Bleu_4"] == values["device"]["Bleu_4"], rouge_l_equal=values["host"]["ROUGE_L"] == values["device"]["ROUGE_L"],
                   cider_host=values["host"]["CIDEr"], cider_device=values["device"]["CIDEr"], device_scored_on_host=values["device"]["scored_on_host"])
        runs.append(run)
        rec = json.load(open(a.out)) if os.path.exists(a.out) else {}
        timing = rec.setdefault("timing", {"note": "CaptionMetrics.score end to end (vocabulary, table over the evaluated images, scoring, reduction), wall "
                                                   "seconds around a synchronise, one child process per figure, host and device alternating",
                                           "tool": "tools/caption_eval_bench.py", "runs": {}})
        timing["runs"]["images_%d" % images] = run
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=2, sort_keys=True)
        print("wrote", a.out, flush=True)


if __name__ == "__main__":
    main()
