"""The CIDEr-D kernels alone on one MI355X: vlp_cider_d (df from the call's references) and vlp_cider_d_df (df from a resident table), both launches
back to back on one stream, device events around `iters` calls, the two entry points alternating inside one process.

    python tools/cider_d_bench.py [--df 4000000] [--repeats 5] [--out profiles/scst_reward_df.json]

Shapes: the training shapes (G = 16 / 64, R = 1 / 5, T = 21), G = 256 and the largest accepted one (G = 1024, R = 8, T = 64).  References are
seeded rows over a 12-word vocabulary, a hypothesis is a copy of its group's first reference; the table is tools/scst_bench.py's seeded one
(--df n-grams over 113287 documents), so a lookup runs the full log2(N) probes whether it hits or not.  The record goes under the "kernel_alone"
key of --out, next to what is there.  Nothing is asserted: this records what is measured."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from scst_bench import seeded_table                # noqa: E402
from vlp_amd import _lib as K                      # noqa: E402

SHAPES = [(16, 1, 21, 200), (16, 5, 21, 200), (64, 1, 21, 200), (64, 5, 21, 200), (256, 5, 21, 200), (1024, 8, 64, 5)]     # (G, R, T, iters)


def case(G, R, T, dev, seed=0):
    rng = np.random.RandomState(seed)
    ref = np.zeros((G, R, T), dtype=np.int64)
    for g in range(G):
        for r in range(R):
            n = rng.randint(T // 2 + 1, T + 1)
            ref[g, r, :n] = rng.randint(1000, 1012, size=n)
            if n < T:
                ref[g, r, n - 1] = 102
    hyp = np.concatenate([ref[:, 0], ref[:, 0]], 0)
    return torch.from_numpy(hyp).to(dev), torch.from_numpy(ref).to(dev)


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--df", type=int, default=4000000, help="n-grams of the seeded table")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scst_reward_df.json"))
    a = ap.parse_args()
    dev = torch.device("cuda")
    tab = seeded_table(a.df)
    keys, vals = tab.to(dev)
    runs = []
    for G, R, T, iters in SHAPES:
        hyp, ref = case(G, R, T, dev)
        scores, reward = torch.empty(2 * G, device=dev), torch.empty(G, device=dev)
        ws = torch.empty(max(K.cider_d_workspace_bytes(G, R, T, 2), K.cider_d_df_workspace_bytes(G, R, T, 2)), dtype=torch.uint8, device=dev)

        def batch_mode():
            K.cider_d(hyp, ref, None, 2, scores, reward, workspace=ws)

        def table_mode():
            K.cider_d_df(hyp, ref, None, 2, scores, keys, vals, tab.n_docs, reward, workspace=ws)
        t = {"batch": [], "table": []}
        for _ in range(a.repeats):                 # alternating, so that both see the same neighbours on the box
            t["batch"].append(timed(batch_mode, iters))
            t["table"].append(timed(table_mode, iters))
        r = dict(G=G, R=R, T=T, mult=2, iters=iters, table_keys=len(tab),
                 batch_us_per_call_median=float(np.median(t["batch"])), batch_us_per_call_min=float(np.min(t["batch"])),
                 table_us_per_call_median=float(np.median(t["table"])), table_us_per_call_min=float(np.min(t["table"])))
        print(json.dumps(r, sort_keys=True), flush=True)
        runs.append(r)
    rec = json.load(open(a.out)) if os.path.exists(a.out) else {}
    rec["kernel_alone"] = {"note": "both launches of vlp_cider_d ('batch') and of vlp_cider_d_df ('table') back to back on one stream, device events around "
                                   "`iters` calls, the two alternating, median of %d repeats; a hypothesis is a copy of its group's first reference" % a.repeats,
                           "tool": "tools/cider_d_bench.py --df %d --repeats %d" % (a.df, a.repeats), "runs": runs}
    rec.setdefault("device", torch.cuda.get_device_name(0))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=2, sort_keys=True)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
