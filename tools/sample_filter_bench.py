"""Cost of temperature / top-k / top-p sampling (vlp_sample_rows_filtered) next to the plain sampler (vlp_sample_rows_rep).

    python tools/sample_filter_bench.py [--rounds 3] [--skip_step]  >  one JSON line

  kernel  one launch at 64 and 320 rows of V = 28 996 (ld 29 056) fp16 logits, N(0, 2^2): the plain sampler, and the filtered one with nothing
          filtered, top_k = 50, top_p = 0.9, and both.  Device events around 2000 launches over 4 rotating logits buffers, after 50 warm-up launches.
  step    Engine.decode_sample_group at B = 64, 12 layers, 20 new tokens, K = 1 and K = 5 samples per image: (1, 0, 1) against
          top_k = 50 / top_p = 0.9 at T = 1; wall time of 5 calls (replayed token steps) ending in a synchronise, per token step.
Every figure comes from a child process of its own; the variants alternate, `rounds` times, and the spread of the rounds is reported.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
V, LD = 28996, 29056
KERNEL_VARIANTS = {"plain": None, "filtered_neutral": (1.0, 0, 1.0), "top_k50": (1.0, 50, 1.0), "top_p0.9": (1.0, 0, 0.9), "top_k50_top_p0.9": (1.0, 50, 0.9),
                   "T0.8_top_k50_top_p0.9": (0.8, 50, 0.9)}
STEP_VARIANTS = {"plain": (1.0, 0, 1.0), "top_k50_top_p0.9": (1.0, 50, 0.9)}


def child_kernel(variant):
    import torch
    from vlp_amd import _lib as K
    dev = torch.device("cuda:0")
    par = KERNEL_VARIANTS[variant]
    out = {}
    for rows in (64, 320):
        g = torch.Generator().manual_seed(rows)
        bufs = [(torch.randn(rows, LD, generator=g) * 2).half().to(dev) for _ in range(4)]
        ids = torch.zeros(rows, dtype=torch.long, device=dev)
        ids2 = torch.zeros(rows, dtype=torch.long, device=dev)
        lp = torch.zeros(rows, dtype=torch.float32, device=dev)
        cell = torch.tensor([17], dtype=torch.long, device=dev)

        def launch(i):
            if par is None:
                K.sample_rows_rep(bufs[i % 4], LD, rows, V, 1, cell, i, 7001, ids, lp, ids2=ids2)
            else:
                K.sample_rows_filtered(bufs[i % 4], LD, rows, V, 1, cell, i, 7001, par[0], par[1], par[2], ids, lp, ids2=ids2)
        for i in range(50):
            launch(i)
        torch.cuda.synchronize()
        n = 2000
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(n):
            launch(i)
        e1.record()
        torch.cuda.synchronize()
        out["rows%d_us" % rows] = round(e0.elapsed_time(e1) * 1e3 / n, 2)
    print(json.dumps(out))


def child_step(variant, Ks):
    import torch
    from vlp_amd import synthetic as S
    from vlp_amd.modeling import BertConfig, BertForSeq2SeqDecoder
    dev = torch.device("cuda:0")
    B, T, Nv = 64, 20, 100
    par = STEP_VARIANTS[variant]
    torch.manual_seed(0)
    cfg = BertConfig(V, num_hidden_layers=12, type_vocab_size=6)
    g = torch.Generator().manual_seed(0)
    img = torch.randn(B, Nv, 2048, generator=g).abs().half().to(dev)
    vis_pe = torch.rand(B, Nv, 1607, generator=g).half().to(dev)
    in_len, out_len = Nv + 2, Nv + 2 + T
    input_ids = torch.tensor([[S.CLS_ID] + [S.UNK_ID] * Nv + [S.SEP_ID]] * B).to(dev)
    token_type = torch.tensor([[4] * in_len + [5] * T] * B).to(dev)
    pos = torch.arange(out_len).unsqueeze(0).expand(B, -1).contiguous().to(dev)
    am = torch.zeros(B, out_len, out_len, dtype=torch.long)
    am[:, :, :in_len] = 1
    am[:, in_len:, in_len:] = torch.tril(torch.ones(T, T, dtype=torch.long))
    am = am.to(dev)
    m = BertForSeq2SeqDecoder(cfg, mask_word_id=S.MASK_ID, eos_id=S.SEP_ID, enable_butd=True, len_vis_input=Nv, allow_random_fc7=True).half().to(dev).eval()
    eng = m.engine

    def run():
        return eng.decode_sample_group(img, vis_pe, input_ids, token_type, pos, am, S.MASK_ID, Ks, temperature=par[0], top_k=par[1], top_p=par[2])
    with torch.no_grad():
        for _ in range(3):                        # plain, captured, replayed
            run()
        torch.cuda.synchronize()
        n = 5
        t0 = time.perf_counter()
        for _ in range(n):
            run()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / n
    ws = eng._ws[("dec", B, in_len + 1, out_len, Ks, "group")]
    print(json.dumps({"ms_per_call": round(dt * 1e3, 3), "ms_per_token_step": round(dt * 1e3 / T, 4), "plan_keys_step1": sorted(str(k) for k in ws["plans"] if k[1] == 1)}))


def spawn(*args):
    sys.stderr.write("child %s\n" % (args,))
    sys.stderr.flush()
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + [str(a) for a in args], capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        sys.stderr.write(r.stdout + r.stderr)
        raise SystemExit("child %s failed with status %d" % (args, r.returncode))          # nothing more is started on the GPU
    return json.loads(r.stdout.strip().splitlines()[-1])


def summarise(runs):
    keys = [k for k in runs[0] if isinstance(runs[0][k], (int, float))]
    out = {k: {"median": sorted(r[k] for r in runs)[len(runs) // 2], "runs": [r[k] for r in runs]} for k in keys}
    out.update({k: runs[0][k] for k in runs[0] if k not in keys})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--skip_step", action="store_true")
    ap.add_argument("--child", nargs="+", default=None)
    a = ap.parse_args()
    if a.child:
        if a.child[0] == "kernel":
            child_kernel(a.child[1])
        else:
            child_step(a.child[1], int(a.child[2]))
        return
    res = {"V": V, "ld": LD, "rounds": a.rounds, "kernel": {}, "step": {}}
    runs = {v: [] for v in KERNEL_VARIANTS}
    for _ in range(a.rounds):
        for v in KERNEL_VARIANTS:                 # alternating
            runs[v].append(spawn("kernel", v))
    res["kernel"] = {v: summarise(r) for v, r in runs.items()}
    if not a.skip_step:
        for Ks in (1, 5):
            runs = {v: [] for v in STEP_VARIANTS}
            for _ in range(max(2, a.rounds - 1)):
                for v in STEP_VARIANTS:
                    runs[v].append(spawn("step", v, Ks))
            res["step"]["K%d" % Ks] = {v: summarise(r) for v, r in runs.items()}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
