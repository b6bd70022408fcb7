"""Consensus selection among K samples per image on the device against the host: vlp_amd.consensus.consensus_select_device (the two launches
of vlp_cider_d_consensus) and consensus_utility (scst.CiderD in fp64), on the same seeded inputs.

    python tools/consensus_bench.py [--iters 200] [--out profiles/consensus.json]

Shapes (G images, K samples, T ids): (64, 5, 21), (64, 16, 21), (256, 8, 21), (1024, 5, 21).  The samples of an image are copies of one
seeded caption of 8..20 words over a 2000-word Zipf-like vocabulary with 30 % of the words redrawn, [SEP] and 0 behind them; the table is
counted over 5000 such captions.  Per shape:
  device   `iters` calls between two device events after 10 warm-up calls (workspace and outputs allocated once), three windows, the median;
  gather   where K - 1 <= 8, the alternative the kernel replaces: the other samples gathered into a [K*G, K-1, T] reference array and scored
           by vlp_cider_d_df as K*G groups of one hypothesis (K*G <= 1024), timed the same way, gather included;
  host     one consensus_utility call, wall seconds;
and the largest |device - host| utility with the number of images whose pick differs from the host's.  No speed is asserted: this records
what is measured, under the "timing" key of --out."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VOCAB, MIN_LEN, MAX_LEN, SEP, T = 2000, 8, 20, 102, 21
SHAPES = [(64, 5, 21), (64, 16, 21), (256, 8, 21), (1024, 5, 21)]


def captions(n, seed):
    rng = np.random.RandomState(seed)
    p = 1.0 / np.arange(1, VOCAB + 1)
    p /= p.sum()
    return [[int(w) + 1000 for w in rng.choice(VOCAB, size=rng.randint(MIN_LEN, MAX_LEN + 1), p=p)] for _ in range(n)]


def samples(G, K, seed=1):
    """int64 [K*G, T], row k*G + g: sample k of image g."""
    rng = np.random.RandomState(seed)
    base = captions(G, seed)
    ids = np.zeros((K * G, T), dtype=np.int64)
    for k in range(K):
        for g in range(G):
            row = list(base[g])
            for j in np.flatnonzero(rng.rand(len(row)) < 0.3):
                row[j] = int(rng.randint(VOCAB)) + 1000
            ids[k * G + g, :len(row) + 1] = row + [SEP]
    return ids


def timed(fn, iters, torch):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    windows = []
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        windows.append(e0.elapsed_time(e1) * 1e-3 / iters)
    return windows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "consensus.json"))
    a = ap.parse_args()
    import torch
    from vlp_amd import _lib as K_
    from vlp_amd import consensus as CS
    from vlp_amd.scst import DocFreq
    if not torch.cuda.is_available():
        raise SystemExit("tools/consensus_bench.py measures on the GPU; there is none")
    dev = torch.device("cuda")
    tab = DocFreq.from_examples([(i, c) for i, c in enumerate(captions(5000, 0))], T - 1, SEP)
    keys, vals = tab.to(dev)
    runs = {}
    for G, K, _ in SHAPES:
        ids = samples(G, K)
        h = torch.from_numpy(ids).to(dev)
        utility = torch.empty(K * G, device=dev)
        ws = torch.empty(K_.cider_d_consensus_workspace_bytes(G, K, T), dtype=torch.uint8, device=dev)
        pick = CS.consensus_select_device(h, K, tab, utility_out=utility, workspace=ws)[0]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        want, want_pick = CS.consensus_utility(ids, K, tab)
        host_s = time.perf_counter() - t0
        err = float(np.abs(utility.double().cpu().numpy() - want).max())
        differ = int((pick.cpu().numpy() != want_pick).sum())
        dev_w = timed(lambda: CS.consensus_select_device(h, K, tab, utility_out=utility, workspace=ws), a.iters, torch)
        run = dict(G=G, K=K, T=T, iters=a.iters, device_seconds=dev_w, device_seconds_median=float(np.median(dev_w)), host_seconds=host_s,
                   host_over_device=host_s / float(np.median(dev_w)), max_abs_err=err, picks_differing_from_host=differ, table_keys=len(tab),
                   n_docs=tab.n_docs)
        if K - 1 <= 8 and K * G <= 1024:
            other = torch.tensor([[j * G + g for j in range(K) if j != k] for k in range(K) for g in range(G)], device=dev)
            scores = torch.empty(K * G, device=dev)
            ws2 = torch.empty(K_.cider_d_df_workspace_bytes(K * G, K - 1, T, 1), dtype=torch.uint8, device=dev)

            def gather():
                K_.cider_d_df(h, h[other], None, 1, scores, keys, vals, tab.n_docs, workspace=ws2)
            gat_w = timed(gather, a.iters, torch)
            run.update(gather_seconds=gat_w, gather_seconds_median=float(np.median(gat_w)),
                       gather_over_device=float(np.median(gat_w)) / float(np.median(dev_w)),
                       gather_max_abs_diff=float((scores - utility).abs().max()))
        print(json.dumps(run, sort_keys=True), flush=True)
        runs["G%d_K%d_T%d" % (G, K, T)] = run
    rec = json.load(open(a.out)) if os.path.exists(a.out) else {}
    rec["timing"] = {"note": "consensus_select_device (two launches, buffers allocated once) between device events, median of three windows; host: one "
                             "consensus_utility call (scst.CiderD, fp64), wall seconds; gather: the other samples gathered into [K*G, K-1, T] and "
                             "scored by vlp_cider_d_df, gather included", "tool": "tools/consensus_bench.py", "runs": runs}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=2, sort_keys=True)
    print("wrote", a.out, flush=True)


if __name__ == "__main__":
    main()
