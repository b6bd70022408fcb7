"""Device-event timing of scoring given captions (vlp_token_score, BertForSeq2SeqDecoder.score) next to what the tree had before it.

    python tools/caption_score_bench.py [--rounds 7] [--reps 50] [--out profiles/caption_score.json]

(1) kernel: N(0, 3^2) fp16 logits [64 * 20, 28996] (ld 29056).  vlp_token_score against vlp_token_policy_fwd at T = 1 with entropy (the
    same floats, no rank, no arg-max) and against that launch plus the torch ops that give rank and arg-max from the same rows (a gather,
    two comparisons over [rows, V], a sum, a max).
(2) model: the 12-layer decoder at B = 64, T = 20: one score() call (host rule, vlp_scst_layout, dense forward, LM head, vlp_token_score,
    results the caller owns) against Engine.score_samples under no_grad (the same pass with vlp_token_logprob_fwd, a workspace view).
One process; every variant warmed, then `--rounds` rounds in which the variants alternate, each timed as back-to-back calls between two
events.  Reports median / min / max over the rounds in microseconds per call and keeps the record under the "bench" key of --out (the
other keys of the file are left as they are).  No time is asserted anywhere."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vlp_amd import _lib as K          # noqa: E402


def timed(variants, rounds, reps):
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
    return {n: {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))} for n, v in times.items()}


def bench_kernel(rounds, reps, dev):
    rows, V, ld = 64 * 20, 28996, 29056
    g = torch.Generator(device=dev).manual_seed(1)
    logits = torch.zeros(rows, ld, device=dev, dtype=torch.half)
    logits[:, :V] = (torch.randn(rows, V, device=dev, generator=g) * 3.0).half()
    ids = torch.randint(0, V, (rows,), device=dev, generator=g)
    logp, lse, ent, top = (torch.zeros(rows, device=dev) for _ in range(4))
    rank = torch.zeros(rows, device=dev, dtype=torch.int32)
    top_id = torch.zeros(rows, device=dev, dtype=torch.long)
    col = torch.arange(V, device=dev).view(1, V)

    def policy():
        K.token_policy_fwd(logits, ld, ids, logp, lse, rows, V, temperature=1.0, entropy=ent)

    def policy_and_torch():
        policy()
        x = logits[:, :V]
        lid = x.gather(1, ids.view(-1, 1))
        ((x > lid) | ((x == lid) & (col < ids.view(-1, 1)))).sum(1)
        x.max(1)
    variants = [("token_score", lambda: K.token_score(logits, ld, ids, logp, lse, ent, rank, top_id, top, rows, V)),
                ("token_policy_fwd T=1 +H", policy), ("token_policy_fwd T=1 +H, torch rank and arg-max", policy_and_torch)]
    return {"rows": rows, "V": V, "ld": ld, "rounds": rounds, "reps": reps, "us_per_launch": timed(variants, rounds, reps)}


def bench_model(rounds, reps, dev):
    from oracle import vlp_oracle as O                        # parameter init only
    from oracle.make_golden import decode_inputs
    from vlp_amd import synthetic as S
    from vlp_amd.modeling import BertConfig, BertForSeq2SeqDecoder
    V, layers, B, T = 28996, 12, 64, 20
    p = O.init_params(vocab_size=V, layers=layers, seed=5, std=0.02)
    cfg = BertConfig(V, num_hidden_layers=layers, type_vocab_size=6, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    m = BertForSeq2SeqDecoder(cfg, mask_word_id=S.MASK_ID, eos_id=S.SEP_ID, enable_butd=True, len_vis_input=100)
    sd = dict(p)
    sd["cls.predictions.decoder.weight"] = p["bert.embeddings.word_embeddings.weight"]
    m.load_state_dict(sd, strict=True)
    m.half().to(dev).eval()
    t = decode_inputs(B, T, 3, 100)
    inp = (t[0].half().to(dev), t[1].half().to(dev)) + tuple(x.to(dev) for x in t[2:])
    gen = torch.Generator().manual_seed(2)
    lens = torch.randint(5, T, (B,), generator=gen)
    caps = [torch.randint(1000, V, (int(n),), generator=gen).tolist() for n in lens]
    full = torch.randint(1000, V, (B, T), generator=gen).to(dev)

    def score():
        with torch.no_grad():
            m.score(*inp, caps)

    def score_samples():
        with torch.no_grad():
            m.engine.score_samples(*inp, full, S.MASK_ID)
    variants = [("score() B=64 T=20", score), ("score_samples under no_grad", score_samples)]
    return {"V": V, "layers": layers, "B": B, "T": T, "counted_positions": int(lens.sum()) + B, "rounds": rounds, "reps": reps,
            "us_per_call": timed(variants, rounds, reps)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--model_reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "caption_score.json"))
    a = ap.parse_args()
    dev = torch.device("cuda")
    rec = json.load(open(a.out)) if os.path.exists(a.out) else {}
    bench = {"device": torch.cuda.get_device_name(0), "tool": "tools/caption_score_bench.py"}
    bench["kernel"] = bench_kernel(a.rounds, a.reps, dev)
    print(json.dumps(bench["kernel"], sort_keys=True), flush=True)
    bench["model"] = bench_model(a.rounds, a.model_reps, dev)
    print(json.dumps(bench["model"], sort_keys=True), flush=True)
    rec["bench"] = bench
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=2, sort_keys=True)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
