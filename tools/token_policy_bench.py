"""Device-event timing of vlp_token_policy_fwd / _bwd next to vlp_token_logprob_fwd / _bwd (csrc/loss.hip) at the SCST scoring shapes.

    python tools/token_policy_bench.py [--rows 1280 6400] [--temperature 0.8] [--out profiles/scst_policy.json]

One process: N(0, 3^2) fp16 logits [rows, 28996] (ld 29056), every variant warmed, then `--rounds` rounds in which the variants alternate,
each timed as `--reps` back-to-back launches between two events.  Reports the median over the rounds in microseconds per launch and keeps the
record under the "kernels" key of --out (the other keys of the file are left as they are)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vlp_amd import _lib as K          # noqa: E402


def bench(rows, T, rounds, reps, dev):
    V, ld = 28996, 29056
    g = torch.Generator(device=dev).manual_seed(1)
    logits = torch.zeros(rows, ld, device=dev, dtype=torch.half)
    logits[:, :V] = (torch.randn(rows, V, device=dev, generator=g) * 3.0).half()
    ids = torch.randint(0, V, (rows,), device=dev, generator=g)
    logp, lse, ent, lse_t = (torch.zeros(rows, device=dev) for _ in range(4))
    gr, hr = torch.randn(rows, device=dev, generator=g) * 512.0, torch.randn(rows, device=dev, generator=g) * 512.0
    dl = torch.empty(rows, ld, device=dev, dtype=torch.half)
    K.token_logprob_fwd(logits, ld, ids, logp, lse, rows, V)
    K.token_policy_fwd(logits, ld, ids, logp, lse_t, rows, V, temperature=T, entropy=ent)
    variants = [
        ("token_logprob_fwd", lambda: K.token_logprob_fwd(logits, ld, ids, logp, lse, rows, V)),
        ("token_policy_fwd T", lambda: K.token_policy_fwd(logits, ld, ids, logp, lse_t, rows, V, temperature=T)),
        ("token_policy_fwd T+H", lambda: K.token_policy_fwd(logits, ld, ids, logp, lse_t, rows, V, temperature=T, entropy=ent)),
        ("token_logprob_bwd", lambda: K.token_logprob_bwd(logits, ld, ids, lse, gr, dl, ld, rows, V)),
        ("token_policy_bwd T", lambda: K.token_policy_bwd(logits, ld, ids, lse_t, gr, dl, ld, rows, V, temperature=T)),
        ("token_policy_bwd T+h", lambda: K.token_policy_bwd(logits, ld, ids, lse_t, gr, dl, ld, rows, V, temperature=T, h=hr, entropy=ent)),
    ]
    for _, fn in variants:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {n: [] for n, _ in variants}
    for _ in range(rounds):
        for n, fn in variants:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            b.synchronize()
            times[n].append(a.elapsed_time(b) * 1e3 / reps)
    return {"rows": rows, "V": V, "ld": ld, "temperature": T, "rounds": rounds, "reps": reps,
            "us_per_launch": {n: {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))} for n, v in times.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[1280, 6400])
    ap.add_argument("--temperature", type=float, default=0.8)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scst_policy.json"))
    a = ap.parse_args()
    dev = torch.device("cuda")
    runs = []
    for rows in a.rows:
        r = bench(rows, a.temperature, a.rounds, a.reps, dev)
        print(json.dumps(r, sort_keys=True), flush=True)
        runs.append(r)
    rec = json.load(open(a.out)) if os.path.exists(a.out) else {}
    rec["kernels"] = {"device": torch.cuda.get_device_name(0), "tool": "tools/token_policy_bench.py", "runs": runs}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=2, sort_keys=True)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
