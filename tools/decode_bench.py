"""N1 measurement: captions/s of the K/V-cache decoder (12 layers, vocab 28 996, 100 regions, 20 generated tokens), greedy and beam.

    MODES=greedy,beam3,beam5[,beam3_ngram,beam5_ngram]   the *_ngram modes search with forbid_duplicate_ngrams=True, ngram_size=3
    BLOCKING=device|host                                 where their n-gram blocking runs (BertForSeq2SeqDecoder.ngram_blocking); host mode
                                                         only needs interfaces older trees have, so this file also times those
    BACKTRACK=host|device                                where beam_search turns the frames into hypotheses (BertForSeq2SeqDecoder.backtrack)
    N_BEST=N                                             hypotheses kept per image in the beam modes (N > 1 back-tracks on the device)
    BACKTRACK_AB=1                                       instead of the modes: beam 3 and beam 5, each as ONE model whose calls alternate between
                                                         backtrack=host, backtrack=device and device with n_best = beam (same weights, workspace and
                                                         captured token steps; ROUNDS rounds after 3 warm-up calls of each), plus the event time
                                                         around vlp_beam_nbest alone -> profiles/beam_nbest.json
    --beam_groups G[,G..] [--diversity_penalty L] [--beam_size K]
                                                         instead of the modes: diverse beam search (BertForSeq2SeqDecoder(beam_groups=G,
                                                         diversity_penalty=L); default L 0.5, K 6) against the plain search, as ONE model whose
                                                         calls alternate between G = 1 and every G given (ROUNDS rounds after 3 warm-up calls of
                                                         each), plus the event time of one vlp_beam_select_groups launch against one
                                                         vlp_beam_select launch at K = 6 and K = 64 -> profiles/diverse_beam.json
"""
import argparse
import json
import os
import sys
import time

import torch

# the command line is read before anything touches a device (--help needs none); the older modes are chosen by the environment variables above
_p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
_p.add_argument("--beam_groups", default=None, help="comma-separated group counts of the diverse A/B, each dividing --beam_size")
_p.add_argument("--diversity_penalty", type=float, default=0.5)
_p.add_argument("--beam_size", type=int, default=6)
_a = _p.parse_args()

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from vlp_amd import synthetic as S  # noqa: E402
from vlp_amd.modeling import BertConfig, BertForSeq2SeqDecoder  # noqa: E402

dev = torch.device("cuda:0")
B, T, Nv = int(os.environ.get("B", 64)), 20, 100
torch.manual_seed(0)
cfg = BertConfig(28996, num_hidden_layers=12, type_vocab_size=6)
out = {"batch": B, "new_tokens": T, "layers": 12}
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
BLOCKING = os.environ.get("BLOCKING", "device")
assert BLOCKING in ("device", "host")
NGRAM = dict(forbid_duplicate_ngrams=True, ngram_size=3)
BACKTRACK, N_BEST = os.environ.get("BACKTRACK", "host"), int(os.environ.get("N_BEST", 1))
assert BACKTRACK in ("device", "host")


def backtrack_ab():
    """Host against device back-tracking inside a beam-search batch, same process, alternating calls; every call ends in a synchronise."""
    import statistics
    rounds = int(os.environ.get("ROUNDS", 12))
    res = {"batch": B, "new_tokens": T, "layers": 12, "rounds": rounds, "warmup_calls_per_config": 3,
           "timing": "host clock around one beam_search call, synchronised before and after; the three configurations alternate inside every round"}
    for Kb in (3, 5):
        m = BertForSeq2SeqDecoder(cfg, mask_word_id=S.MASK_ID, eos_id=S.SEP_ID, enable_butd=True, len_vis_input=Nv, allow_random_fc7=True,
                                  search_beam_size=Kb).half().to(dev).eval()
        configs = (("host", "host", 1), ("device", "device", 1), ("device_n_best_%d" % Kb, "device", Kb))
        times, preds = {c[0]: [] for c in configs}, {}

        def call(name, where, n):
            m.backtrack, m.n_best = where, n
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = m(img, vis_pe, input_ids, token_type, pos, am)
            torch.cuda.synchronize()
            preds[name] = r["pred_seq"]
            return (time.perf_counter() - t0) * 1e3
        for _ in range(3):
            for c in configs:
                call(*c)
        for _ in range(rounds):
            for c in configs:
                times[c[0]].append(call(*c))
        assert all(torch.equal(preds["host"], p) for p in preds.values()), "host and device back-tracking disagree"
        entry = {name: {"ms_per_batch_median": round(statistics.median(ts), 3), "min": round(min(ts), 3), "max": round(max(ts), 3),
                        "stdev": round(statistics.stdev(ts), 3)} for name, ts in times.items()}
        # the kernel alone: device events around Engine.beam_nbest on the frames of the last search (launch overhead included)
        tot, wids, ptrs = (t.clone() for t in (m.engine._ws[("dec", B, in_len + 1, out_len, Kb)][k][:T] for k in ("tot", "wids", "ptrs")))
        for n in (1, Kb):
            ev = []
            for i in range(25):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                m.engine.beam_nbest(tot, wids, ptrs, n, S.SEP_ID, m.length_penalty, out_len)
                b.record()
                torch.cuda.synchronize()
                if i >= 5:
                    ev.append(a.elapsed_time(b) * 1e3)
            entry["vlp_beam_nbest_n%d_event_us" % n] = {"median": round(statistics.median(ev), 1), "min": round(min(ev), 1), "max": round(max(ev), 1)}
        res["beam%d" % Kb] = entry
        del m
        torch.cuda.empty_cache()
    print(json.dumps(res))


def diverse_ab(Kb, group_list, lam):
    """Plain against diverse beam search inside one process, alternating calls of one model; every call ends in a synchronise."""
    import statistics
    from vlp_amd import _lib as K
    rounds = int(os.environ.get("ROUNDS", 12))
    res = {"batch": B, "new_tokens": T, "layers": 12, "beam": Kb, "diversity_penalty": lam, "rounds": rounds, "warmup_calls_per_config": 3,
           "timing": "host clock around one beam_search call, synchronised before and after; the configurations alternate inside every round"}
    m = BertForSeq2SeqDecoder(cfg, mask_word_id=S.MASK_ID, eos_id=S.SEP_ID, enable_butd=True, len_vis_input=Nv, allow_random_fc7=True,
                              search_beam_size=Kb).half().to(dev).eval()
    configs = [("groups_1", 1, 0.0)] + [("groups_%d" % G, G, lam) for G in group_list]
    times, distinct = {c[0]: [] for c in configs}, {}

    def call(name, G, L):
        m.beam_groups, m.diversity_penalty = G, L
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = m(img, vis_pe, input_ids, token_type, pos, am)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) * 1e3
        distinct[name] = round(float(sum(len(set(row)) for row in r["wids"][:, T - 1].tolist())) / B, 2)
        return dt
    for _ in range(3):
        for c in configs:
            call(*c)
    for _ in range(rounds):
        for c in configs:
            times[c[0]].append(call(*c))
    for name, ts in times.items():
        res[name] = {"ms_per_batch_median": round(statistics.median(ts), 3), "min": round(min(ts), 3), "max": round(max(ts), 3),
                     "stdev": round(statistics.stdev(ts), 3), "distinct_words_in_last_frame_per_image": distinct[name]}
    del m
    torch.cuda.empty_cache()
    # one launch alone: device events around the selection of a later frame (launch overhead included), the two entries alternating
    res["launch_timing"] = "device events around one launch of a later frame, B = %d; 40 alternating launches of each after 10 warm-up" % B
    for Ks, G in ((6, 3), (64, 4)):
        gen = torch.Generator().manual_seed(Ks)
        kk_s = torch.randn(B, Ks, Ks, generator=gen).sort(dim=-1, descending=True)[0].to(dev)
        kk_i = torch.randint(0, 28996, (B, Ks, Ks), generator=gen).to(dev)
        lt, le = torch.randn(B, Ks, generator=gen).to(dev), torch.zeros(B, Ks, device=dev)
        o = [torch.empty(B, Ks, device=dev, dtype=dt) for dt in (torch.float32, torch.long, torch.long, torch.float32)]
        src, nxt = torch.empty(B * Ks, device=dev, dtype=torch.long), torch.empty(B * Ks, 2, device=dev, dtype=torch.long)
        ev = {"vlp_beam_select": [], "vlp_beam_select_groups": []}
        for i in range(50):
            for name in ev:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                if name == "vlp_beam_select":
                    K.beam_select(kk_s, kk_i, lt, le, o[0], o[1], o[2], o[3], src, nxt[:, 0], B, Ks, False, S.SEP_ID)
                else:
                    K.beam_select_groups(kk_s, kk_i, lt, le, o[0], o[1], o[2], o[3], src, nxt[:, 0], B, Ks, False, S.SEP_ID, G, lam)
                b.record()
                torch.cuda.synchronize()
                if i >= 10:
                    ev[name].append(a.elapsed_time(b) * 1e3)
        res["launch_K%d" % Ks] = dict({name + "_event_us": {"median": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1)}
                                       for name, v in ev.items()}, groups=G)
    print(json.dumps(res))


if os.environ.get("BACKTRACK_AB") == "1":
    backtrack_ab()
    sys.exit(0)
if _a.beam_groups:
    diverse_ab(_a.beam_size, [int(v) for v in _a.beam_groups.split(",")], _a.diversity_penalty)
    sys.exit(0)
MODES = [m for m in (("greedy", dict(search_beam_size=1)), ("beam3", dict(search_beam_size=3)), ("beam5", dict(search_beam_size=5)),
                     ("beam3_ngram", dict(search_beam_size=3, **NGRAM)), ("beam5_ngram", dict(search_beam_size=5, **NGRAM)))
         if m[0] in os.environ.get("MODES", "greedy,beam3,beam5").split(",")]
for name, kw in MODES:
    m = BertForSeq2SeqDecoder(cfg, mask_word_id=S.MASK_ID, eos_id=S.SEP_ID, enable_butd=True, len_vis_input=Nv, allow_random_fc7=True, **kw).half().to(dev).eval()
    if name.endswith("_ngram"):
        m.ngram_blocking = BLOCKING
    if name != "greedy":
        m.backtrack, m.n_best = BACKTRACK, N_BEST
        out.setdefault("backtrack", BACKTRACK)
        out.setdefault("n_best", N_BEST)
    for _ in range(2):
        m(img, vis_pe, input_ids, token_type, pos, am)
    torch.cuda.synchronize()
    n = 5
    t0 = time.perf_counter()
    for _ in range(n):
        r = m(img, vis_pe, input_ids, token_type, pos, am)
    t_enq = (time.perf_counter() - t0) / n           # host time to enqueue (beam search also waits for its D2H copies here)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / n
    out[name] = {"ms_per_batch": round(dt * 1e3, 2), "captions_per_s": round(B / dt, 1), "ms_per_token_step": round(dt * 1e3 / T, 3),
                 "host_enqueue_ms": round(t_enq * 1e3, 2)}
    if name.endswith("_ngram"):
        out[name]["ngram_blocking"] = BLOCKING
    if name != "greedy" and BACKTRACK == "host" and N_BEST == 1:
        # beam_search() returns the best sequences, which needs one device -> host copy of the frames: the call itself waits for the GPU, so the
        # "enqueue" figure equals the wall time; the device work is enqueued in ~2 ms (Engine.decode_beam, hipGraph replays) -- decoding is not host-bound
        out[name]["host_enqueue_includes_final_device_to_host_copy"] = True
    if name == "greedy":
        # roofline of a TOKEN step (HBM-bound: every step streams the encoder + head weights and the K/V history once): algorithmic bytes =
        # fp16 weights of the 12 layers + head transform + tied vocabulary matrix, + K | V rows of every position decoded so far (B x Lk x 2H
        # fp16 per layer, Lk averaged over the steps), + the logits written and read back by the argmax; against 8 TB/s (6.29 achievable)
        H, NL, V = cfg.hidden_size, cfg.num_hidden_layers, cfg.vocab_size
        w_bytes = 2 * (sum(p.numel() for n, p in m.named_parameters() if n.startswith("bert.encoder.")) + H * H + V * H)
        lk_avg = sum(in_len + s + 1 for s in range(1, T)) / max(T - 1, 1)
        kv_bytes = B * lk_avg * 2 * H * 2 * NL
        logit_bytes = 2 * B * V * 2
        step_bytes = w_bytes + kv_bytes + logit_bytes
        # the first step (whole prefix, 102 rows per sequence) is a different regime: time it alone and subtract
        first_args = (img, vis_pe, input_ids[:, :in_len], token_type[:, :in_len + 1].contiguous(), pos[:, :in_len + 1].contiguous(),
                      am[:, :in_len + 1, :in_len + 1].contiguous())
        for _ in range(2):
            m(*first_args)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for _ in range(n):
            m(*first_args)
        torch.cuda.synchronize()
        first_ms = (time.perf_counter() - t1) / n * 1e3
        tok_ms = max(dt * 1e3 - first_ms, 0.0) / max(T - 1, 1)
        out[name].update({"first_step_ms": round(first_ms, 3), "ms_per_token_step_excl_first": round(tok_ms, 4)})
        out["roofline"] = {"bound": "hbm", "kernel": "one greedy token step (all launches of the step; B = %d, history %.0f positions)" % (B, lk_avg),
                           "achieved": round(step_bytes / (tok_ms * 1e-3) / 1e9, 1), "peak": 8000.0, "unit": "GB/s",
                           "frac": round(step_bytes / (tok_ms * 1e-3) / 8e12, 4), "traffic": None,
                           "algorithmic_mb": {"weights": round(w_bytes / 1e6, 1), "kv_history": round(kv_bytes / 1e6, 1), "logits": round(logit_bytes / 1e6, 1)},
                           "floor_ms_at_6.29_TBps": round(step_bytes / 6.29e12 * 1e3, 4)}
    del m
    torch.cuda.empty_cache()          # (workspaces + captured graphs of one mode otherwise fragment the next mode's allocations: beam 5 after greedy + beam 3 measured 90 ms instead of 34)
print(json.dumps(out))
if os.environ.get("VLP_DEBUG_TUNE") == "1":
    from vlp_amd.engine import Engine
    print("skinny choices:", sorted(Engine._skinny_choice.items()), file=sys.stderr)
