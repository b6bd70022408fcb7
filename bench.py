#!/usr/bin/env python
"""Headline benchmark of the VLP hot path on MI355X (contract in the task brief / BASELINE.json).

    python bench.py --gpus N --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...
(without a launcher, `--gpus N` re-executes itself under torch.distributed.run: one rank per GPU over RCCL)

One "step" = one full training iteration of the reference's loop (run_img2txt_dist.py:479-585) on a synthetic
COCO-shape batch that is already resident in HBM: forward (region projections, embeddings, 12 BertLayers, LM head,
masked-LM loss) + backward + loss-scaled fused Adam (+ RCCL gradient buckets when N > 1), dropout 0.1 as in training.
Workload = BASELINE.json configs[1]: BERT-base 12L, 100 regions, seq_len 64 (L = 64+100+3 = 167), batch 64 per GPU, fp16.
Rank 0 prints ONE JSON line: whole-job samples/s and ms_per_step of the K timed steps.  A plain run does nothing else: set-up,
W warm-up steps, the K timed steps, the outputs (--dump-outputs DIR), the line.  With --full the line also carries
  parity       -- full-size logits of the bench model vs the oracle on the device, before anything is timed;
  config.varlen -- the same batches through the padding-free (packed) step, timed the same way;
  roofline     -- the dominant kernel (vlp_gemm_nt: every forward / dgrad GEMM): algorithmic FLOPs per launch / average launch
                  duration, measured live with HIP events on the launch stream in a second pass over the same K steps (so the
                  brackets do not perturb the timed steps);
  cpu_baseline -- the oracle (CPU restatement of the reference, fp32 fwd+bwd+BertAdam) timed on this box's host cores
                  on a bounded sample (rank 0, N = 1 only).
The --no-* switches below drop single legs of a --full run.

--dump-outputs DIR writes what the last timed step handed its caller (rank 0), float32, under 64 MB in all: the loss tuple
(mlm_loss, vis_pretext_loss, vqa_loss), the head logits of its forward, and a fixed seeded sample of the updated parameters.  The inputs
(weights, batch pool, dropout seeds) are a function of the arguments alone, so two builds can be compared output for output.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

METRIC = "samples/sec/node (COCO 100-region, seq64, bs64xN) fp16"
MFMA_PEAK_TFLOPS = 2500.0          # dense fp16/bf16 MFMA peak, /opt/skills/guides/MI355X_MICROARCH.md
FLOP_PER_SAMPLE = 92.805e9         # fwd+bwd dense contractions at L=167


def nt_kernel_src_sha16():
    """sha256 over the sources of the dominant kernel family (vlp_gemm_nt): a PMC traffic file is only quoted if it was measured on this code."""
    import hashlib
    h = hashlib.sha256()
    d = os.path.join(ROOT, "vlp_amd", "csrc")
    for f in sorted(os.listdir(d)):
        if f.startswith("gemm_nt") or f == "common.h":
            h.update(open(os.path.join(d, f), "rb").read())
    return h.hexdigest()[:16]


def committed_traffic():
    """HBM bytes per launch of the dominant kernel from the newest profiles/rNN_pmc_traffic.json (a separate rocprofv3 --pmc run of
    this command: counters cannot be read inside the process).  Fails loudly -- (None, reason) -- when the file was measured on other
    kernel sources than the ones built here."""
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_traffic.json")))
    if not files:
        return None, "no profiles/r*_pmc_traffic.json committed"
    tf = files[-1]
    rel = os.path.relpath(tf, ROOT)
    try:
        d = json.load(open(tf))
    except Exception as e:      # noqa: BLE001
        return None, "%s unreadable: %s" % (rel, e)
    want, have = d.get("kernel_src_sha16"), nt_kernel_src_sha16()
    if want != have:
        return None, "%s was measured on kernel sources %s, this build is %s: stale, not quoted" % (rel, want, have)
    return d.get("gemm_nt_bytes_per_launch"), rel + " (separate rocprofv3 --pmc run of the same command; FETCH_SIZE calibrated on fused_adam_kernel + WRITE_SIZE)"


def committed_rocprof_family():
    """The dominant kernel family's average duration in the committed rocprofv3 --kernel-trace --stats summary of this command (profiles/
    rNN_rocprofv3_gemm_nt_family.json, made from rNN_rocprofv3_steady_state_summary.txt), quoted next to the live number only if it was
    measured on the kernel sources built here."""
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_rocprofv3_gemm_nt_family.json")))
    if not files:
        return None
    try:
        d = json.load(open(files[-1]))
    except Exception:      # noqa: BLE001
        return None
    if d.get("kernel_src_sha16") != nt_kernel_src_sha16():
        return {"stale": "%s was measured on other kernel sources" % os.path.relpath(files[-1], ROOT)}
    return {"avg_launch_us": d["avg_launch_us"], "tflops": d["tflops"], "frac": d["frac_of_2500"], "launches": d["launches"],
            "source": os.path.relpath(files[-1], ROOT)}


def event_bracket_overhead_us(dev):
    """What an event pair around ONE launch adds to that launch's duration (the command processor's dispatch latency behind the first event),
    measured live on the launch stream: the SAME GEMM (10 688 x 768 x 768, ~20 us: GPU-bound, not host-launch-bound) bracketed one launch at a
    time vs launched back to back between one event pair.  The back-to-back figure still contains the ordinary inter-kernel gap, so the
    difference UNDER-states the overhead a little: the corrected launch durations stay on the conservative side of rocprofv3's."""
    from vlp_amd import _lib as K
    M, N, Kd, reps = 10688, 768, 768, 40
    x = torch.randn(M, Kd, device=dev).half()
    w = (torch.randn(N, Kd, device=dev) * 0.05).half()
    y = torch.empty(M, N, device=dev, dtype=torch.float16)
    for _ in range(5):
        K.gemm_nt(x, w, y, M, N, Kd, variant=77)
    torch.cuda.synchronize()
    pairs = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        K.gemm_nt(x, w, y, M, N, Kd, variant=77)
        e1.record()
        pairs.append((e0, e1))
    torch.cuda.synchronize()
    single = sorted(a.elapsed_time(b) for a, b in pairs)[reps // 2] * 1e3
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        K.gemm_nt(x, w, y, M, N, Kd, variant=77)
    e1.record()
    torch.cuda.synchronize()
    burst = e0.elapsed_time(e1) * 1e3 / reps
    return max(single - burst, 0.0), single, burst


def self_spawn(n, argv):
    """`python bench.py --gpus N` without a launcher: re-execute under torch.distributed.run, one rank per GPU (RCCL), on this node."""
    import socket
    import subprocess
    have = torch.cuda.device_count() if torch.cuda.is_available() else 0
    if have < n:
        raise SystemExit("bench.py --gpus %d: this node exposes %d GPU(s); one rank per GPU is required (no oversubscription)" % (n, have))
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + argv
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    raise SystemExit(subprocess.call(cmd, env=env))


def cpu_baseline_worker(seconds_budget, threads, B=16):
    """oracle (kind 'port'): fp32 forward + backward + BertAdam on the host cores, B=16 (BASELINE.md section 3 protocol), L=167,
    12 layers.  /root/reference does not exist on the GPU box, so this is the oracle restatement (pinned to the unmodified
    reference in tests/test_oracle_vs_reference.py), not the reference's own code: "reference_code": false."""
    torch.set_num_threads(threads)
    from oracle import vlp_oracle as O
    from vlp_amd import synthetic as S
    p = O.init_params(vocab_size=28996, layers=12, tasks="img2txt", seed=0)
    p = {k: v.requires_grad_(True) for k, v in p.items()}
    batch = S.make_batch(B, max_len_b=64, vocab_size=28996, max_pred=3, seed=1234)
    m = {k: torch.zeros_like(v) for k, v in p.items()}
    v = {k: torch.zeros_like(t) for k, t in p.items()}

    def step():
        for t in p.values():
            t.grad = None
        O.loss_and_grads(p, batch, tasks="img2txt")
        with torch.no_grad():
            for k, t in p.items():
                if t.grad is not None:
                    O.bert_adam_step(t, t.grad, m[k], v[k], 1, lr=3e-5, warmup=0.1, t_total=1000,
                                     weight_decay=0.0 if ("bias" in k or "LayerNorm" in k) else 0.01)

    t0 = time.time()
    step()                                   # warm-up (also the fallback measurement on a very slow host)
    warm = time.time() - t0
    n, t0 = 0, time.time()
    while time.time() - t0 + warm < seconds_budget and n < 8:
        step()
        n += 1
    dt = time.time() - t0
    if n == 0:
        n, dt = 1, warm
    tie, ref_equiv = "", None
    try:        # the port's speed relative to the UNMODIFIED reference, measured side by side in the build container (tools/cpu_baseline_ref_vs_port.py)
        import glob
        f = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_cpu_baseline_reference_vs_port.json")))[-1]
        d = json.load(open(f))
        tie = "; the unmodified reference runs the same step at %.2fx the port's speed on the same %d threads (%s)" % (
            d["reference_over_port"], d["threads"], os.path.relpath(f, ROOT))
        ref_equiv = round(B * n / dt * d["reference_over_port"], 3)
    except Exception:      # noqa: BLE001
        pass
    out = {"value": round(B * n / dt, 3), "unit": "samples/s", "cores": threads, "kind": "port", "reference_code": False, "batch": B,
           "reference_equivalent_value": ref_equiv,      # value x (reference / port speed ratio measured in the build container); derived, not timed here
           "sample": "%d steps of B=%d, L=167, 12 layers, fp32 fwd+bwd+BertAdam (oracle/vlp_oracle.py), %d of %d host threads%s"
                     % (n, B, threads, os.cpu_count() or 1, tie)}
    # BASELINE.md section 3 also names B = 64 (the GPU workload's own batch): one warm-up + THREE timed steps of the same port, same threads
    # (a step is ~8 s of CPU work at this size; the leg stops early when it would not fit its 60 s budget, and says how many steps it timed)
    try:
        batch = S.make_batch(64, max_len_b=64, vocab_size=28996, max_pred=3, seed=1234)
        t0 = time.time()
        step()
        w64 = time.time() - t0
        if w64 < 20.0:
            n64, t0 = 0, time.time()
            while n64 < 3 and (time.time() - t0) + w64 * (n64 + 2) < 60.0 + w64:
                step()
                n64 += 1
            if n64 == 0:
                step()
                n64 = 1
            d64, kind64 = (time.time() - t0) / n64, "%d timed step%s after 1 warm-up" % (n64, "" if n64 == 1 else "s")
        else:
            d64, kind64 = w64, "the first step (no warm-up: it alone took %.0f s)" % w64
        out["b64"] = {"value": round(64 / d64, 3), "unit": "samples/s", "batch": 64, "cores": threads, "sample": kind64}
    except Exception as e:      # noqa: BLE001
        out["b64"] = {"value": None, "sample": "failed: %r" % (e,)}
    return out


def cpu_baseline(seconds_budget=20.0, hard_timeout=240.0):
    """Runs the worker in a fresh process (no HIP context, bounded wall time)."""
    import subprocess
    threads = min(os.cpu_count() or 1, 32)
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--cpu-baseline-only", str(seconds_budget), str(threads)],
                           capture_output=True, text=True, timeout=hard_timeout, env=dict(os.environ, HIP_VISIBLE_DEVICES=""))
        for line in reversed(r.stdout.strip().splitlines()):
            if line.startswith("{"):
                return json.loads(line)
        return {"value": None, "unit": "samples/s", "cores": threads, "kind": "port", "sample": "worker failed: " + r.stderr[-200:]}
    except subprocess.TimeoutExpired:
        return {"value": None, "unit": "samples/s", "cores": threads, "kind": "port", "sample": "timed out after %ds" % hard_timeout}


def parity_block(p32, model, batch, tasks, dev):
    """Parity ON THE DRIVER'S RECORD (VERDICT r5 #6a): before anything is timed, the bench model itself -- full size, dropout off -- against the
    oracle evaluated on the device (oracle/ = the CHECKER here, never the thing measured): max-rel error of the head logits vs the fp32 truth,
    vs the reference's fp16 arithmetic, the reference-fp16's own error, and the distance between two reference-fp16 evaluations that differ only
    in summation order (the noise floor of fp16 arithmetic on this network).  Same protocol and numbers as tests/test_20_fullsize_gpu.py."""
    from oracle import vlp_oracle as O
    from vlp_amd import synthetic as S
    key = "vqa_logits" if tasks == "vqa2" else "mlm_logits"

    def relmax(a, b):
        return float((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-30))

    def oracle(dtype, *flags):
        pd = {k: v.to(dev).to(dtype) for k, v in p32.items()}
        with torch.no_grad(), O.rounding(*flags):
            return O.forward_pretraining_loss_mask(pd, S.batch_to(batch, dev), tasks=tasks)
    was_training = model.training
    model.eval()
    b = S.batch_to(batch, dev, half=True)
    with torch.no_grad():
        losses = model(b.img, b.vis_pe, b.input_ids, b.segment_ids, b.input_mask, b.lm_label_ids, b.ans_labels, b.is_next, masked_pos=b.masked_pos,
                       masked_weights=b.masked_weights, task_idx=b.task_idx, drop_worst_ratio=0.0)
    torch.cuda.synchronize()
    truth = oracle(torch.float32)
    t = truth[key].float()
    ours = (model.last_vqa_logits if tasks == "vqa2" else model.last_mlm_logits).float().reshape(t.shape)
    r16 = oracle(torch.float16)[key].float().reshape(t.shape)
    r16b = oracle(torch.float16, "sum_order")[key].float().reshape(t.shape)
    model.train(was_training)
    out = {"logits": key, "shape": list(t.shape), "metric": "max |a - b| / max |b|",
           "hip_vs_fp32_oracle": round(relmax(ours, t), 6), "hip_vs_reference_fp16_oracle": round(relmax(ours, r16), 6),
           "reference_fp16_vs_fp32_oracle": round(relmax(r16, t), 6), "reference_fp16_summation_order_spread": round(relmax(r16b, r16), 6),
           "loss_hip": round(float((losses[0] + losses[1] + losses[2]).sum()), 5), "loss_fp32_oracle": round(float(truth["loss"].sum()), 5),
           "north_star_tolerance": 1e-3,
           "note": "full size (B x L x layers of this run), dropout off, the weights of the timed model; the literal 1e-3 is below the noise floor of fp16 "
                   "arithmetic at this depth (the spread entry; DESIGN.md section 4): the tests bound hip_vs_fp32 by the reference-fp16's own error + 1e-3"}
    out["hip_closer_to_fp32_than_reference_fp16"] = out["hip_vs_fp32_oracle"] <= out["reference_fp16_vs_fp32_oracle"]
    return out


DUMP_MAX_ELEMS = 5 << 20            # per array: 20 MB of float32; three arrays can be that large (logits, two parameter groups): < 64 MB


def dump_outputs(d, lt, model, eng, tasks):
    """--dump-outputs DIR: the loss tuple train_step returned in the last timed step, the head logits of that step's forward and the
    parameters it left, as DIR/<name>.npy (float32).  An array larger than DUMP_MAX_ELEMS is replaced by a fixed sample: the elements at
    indices drawn from a generator seeded by the array's size alone, so the same run arguments always pick the same elements."""
    import numpy as np
    os.makedirs(d, exist_ok=True)
    m = model.module if hasattr(model, "module") else model
    arrays = dict(zip(("mlm_loss", "vis_pretext_loss", "vqa_loss"), lt))
    arrays["vqa_logits" if tasks == "vqa2" else "mlm_logits"] = m.last_vqa_logits if tasks == "vqa2" else m.last_mlm_logits
    arrays["params_decay"], arrays["params_nodecay"] = eng.flat["decay"], eng.flat["nodecay"]
    for name, t in arrays.items():
        t = t.detach().reshape(-1)
        if t.numel() > DUMP_MAX_ELEMS:
            g = torch.Generator().manual_seed(t.numel())
            idx = torch.randint(0, t.numel(), (DUMP_MAX_ELEMS,), generator=g).sort().values
            t = t[idx.to(t.device)]
        np.save(os.path.join(d, name + ".npy"), t.float().cpu().numpy())


def main():
    if len(sys.argv) >= 2 and sys.argv[1] == "--cpu-baseline-only":
        print(json.dumps(cpu_baseline_worker(float(sys.argv[2]), int(sys.argv[3]))))
        return
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=64, help="per-GPU batch (BASELINE: 64)")
    ap.add_argument("--max_len_b", type=int, default=64)
    ap.add_argument("--layers", type=int, default=12)
    ap.add_argument("--tasks", default="img2txt", choices=["img2txt", "vqa2"],
                    help="img2txt = BASELINE configs[1-3] (masked-LM head); vqa2 = configs[4] (bidirectional, P=1, answer classifier + BCE)")
    ap.add_argument("--s2s_prob", type=float, default=1.0, help="per-sample probability of a seq2seq mask (1.0 = COCO fine-tune, "
                                                                "0.75 = Conceptual Captions pre-training shape, configs[3])")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-kernel-events", action="store_true")
    ap.add_argument("--no-varlen", action="store_true", help="skip the second, padding-free (packed) leg reported under config.varlen")
    ap.add_argument("--no-parity", action="store_true", help="skip the parity object (full-size logits vs the oracle on the device, before timing)")
    ap.add_argument("--pool", type=int, default=8, help="device-resident synthetic batches cycled by the timed steps (config.batch_pool)")
    ap.add_argument("--force-dist", action="store_true", help="initialise RCCL + the DDP wrapper even for one rank (path check)")
    ap.add_argument("--full", action="store_true", help="also the parity object, the padding-free leg, the roofline sampling pass and the "
                                                        "CPU baseline (each can be dropped with its --no-* switch); off: the headline alone")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write what the last timed step computed to DIR/<name>.npy (float32)")
    args = ap.parse_args()
    if args.steps < 1:
        raise SystemExit("bench.py --steps must be >= 1")
    if not args.full:
        args.no_cpu_baseline = args.no_kernel_events = args.no_varlen = True
    want_parity = args.full and not args.no_parity

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available() and not (args.gpus > 1 and "WORLD_SIZE" not in os.environ):
        raise SystemExit("bench.py needs an MI355X: vlp_amd has no CPU path")
    if world != args.gpus:
        if "WORLD_SIZE" not in os.environ and args.gpus > 1:
            self_spawn(args.gpus, sys.argv[1:])           # never returns
        raise SystemExit("bench.py --gpus %d was launched with WORLD_SIZE=%d" % (args.gpus, world))
    # one rank per GPU.  VLP_BENCH_SHARE_GPU=1 (test only: world-2 run of the real engine + DDP hooks on a 1-GPU box, backend gloo)
    # lets several ranks share the visible devices
    dev_index = local_rank % torch.cuda.device_count() if os.environ.get("VLP_BENCH_SHARE_GPU") == "1" else local_rank
    torch.cuda.set_device(dev_index)
    dev = torch.device("cuda", dev_index)
    import torch.distributed as dist
    use_dist = world > 1 or args.force_dist
    if use_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        # RCCL ("nccl" on ROCm).  VLP_DIST_BACKEND=gloo only exists for the shared-GPU path check above
        dist.init_process_group(backend=os.environ.get("VLP_DIST_BACKEND", "nccl"), init_method="env://", world_size=world, rank=rank)

    from vlp_amd import synthetic as S
    from vlp_amd.distributed import DistributedDataParallel as DDP
    from vlp_amd.modeling import BertConfig, BertForPreTrainingLossMask
    from vlp_amd.optimization import warmup_linear
    from vlp_amd.optimization_fp16 import FP16_Optimizer_State, FusedAdam
    from vlp_amd.run_img2txt_dist import train_step

    torch.manual_seed(0)
    cfg = BertConfig(28996, num_hidden_layers=args.layers, type_vocab_size=6, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1)
    model = BertForPreTrainingLossMask(cfg, num_labels=2, enable_butd=True, len_vis_input=100, tasks=args.tasks, allow_random_fc7=True)
    p32, parity_err = None, None
    if not args.no_parity:
        # random-init weights of the architecture, drawn by the oracle's initialiser (init_bert_weights, N(0, 0.02): modeling.py:539-551) so that the
        # parity block below can evaluate the SAME network in fp32 / reference-fp16; every rank loads the same values (a plain run too:
        # its timed steps train the network a --full run times)
        try:
            from oracle import vlp_oracle as O
            p32 = O.init_params(vocab_size=28996, layers=args.layers, tasks=args.tasks, seed=0)
            sd = dict(p32)
            sd["cls.predictions.decoder.weight"] = p32["bert.embeddings.word_embeddings.weight"]
            model.load_state_dict(sd, strict=True)
        except Exception as e:      # noqa: BLE001
            p32 = None
            parity_err = "oracle unavailable: %r" % (e,)
    model.half().to(dev)
    eng = model.engine
    # `value` is the DENSE step (BASELINE.json's workload: all L positions of every sample); the padding-free step is the second leg below.
    # VLP_VARLEN=1 in the environment makes the FIRST leg packed (profiling runs) and the line says so.
    env_varlen = eng.varlen is True
    if not env_varlen:
        eng.varlen = False
    if use_dist:
        model = DDP(model, device_ids=[dev_index], output_device=dev_index, find_unused_parameters=True)
    named = list(model.named_parameters())
    no_decay = ["bias", "LayerNorm.bias", "LayerNorm.weight"]
    groups = [{"params": [p for n, p in named if not any(nd in n for nd in no_decay)], "weight_decay": 0.01},
              {"params": [p for n, p in named if any(nd in n for nd in no_decay)], "weight_decay": 0.0}]
    opt = FP16_Optimizer_State(FusedAdam(groups, lr=3e-5, bias_correction=False, max_grad_norm=1.0), dynamic_loss_scale=True)
    # VLP_ADAM_PIPELINE=1: the optimizer step of iteration i streams underneath the first layers of forward i+1 (same arithmetic, chunk
    # events).  Measured: 11.34 -> 11.30 ms/step while the concurrent GEMMs slow down by 6 % -- a wash, so it stays off.
    opt.pipeline_with_forward = os.environ.get("VLP_ADAM_PIPELINE", "0") == "1"
    model.train()
    pool = [S.batch_to(S.make_batch(args.batch, max_len_b=args.max_len_b, vocab_size=28996, max_pred=1 if args.tasks == "vqa2" else 3,
                                    s2s_prob=args.s2s_prob, tasks=args.tasks, seed=1234 + 100 * rank + i), dev, half=True) for i in range(max(1, args.pool))]
    t_total = 100000
    parity = None
    if want_parity and rank == 0 and world == 1:
        if p32 is None:
            parity = {"error": parity_err}
        else:
            try:
                parity = parity_block(p32, model, S.make_batch(args.batch, max_len_b=args.max_len_b, vocab_size=28996, max_pred=1 if args.tasks == "vqa2" else 3,
                                                               s2s_prob=args.s2s_prob, tasks=args.tasks, seed=1234), args.tasks, dev)
            except Exception as e:      # noqa: BLE001
                parity = {"error": repr(e)}
            torch.cuda.empty_cache()
    p32 = None

    def one(i):
        return train_step(model, opt, pool[i % len(pool)], 3e-5 * warmup_linear((i + 1) / t_total, 0.1))

    for i in range(args.warmup):
        lt = one(i)
    torch.cuda.synchronize()
    if use_dist:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.steps):
        lt = one(args.warmup + i)
    torch.cuda.synchronize()
    if use_dist:
        dist.barrier()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if args.dump_outputs:
        if use_dist:
            eng.wait_params()
        if rank == 0:
            dump_outputs(args.dump_outputs, lt, model, eng, args.tasks)
    # roofline sampling: the SAME K steps once more, now with HIP events around every PROF_EVERY-th launch of the dominant kernel (on
    # the launch stream).  It is a separate, un-timed pass so that the event brackets (and the side-stream joins they need) do not
    # perturb the headline steps above.
    comm = None
    bracket = None
    if not args.no_kernel_events:
        if rank == 0:
            try:
                bracket = event_bracket_overhead_us(dev)
            except Exception:      # noqa: BLE001
                bracket = None
        eng.prof = []
        reducer = model.reducer if use_dist else None
        if reducer is not None:          # communication profile of the same pass: stamps around every collective (vlp_amd/distributed.py)
            reducer.profile = True
            eng.param_gather_stamps = [] if getattr(eng, "shard_plan", None) is not None else None
        for i in range(args.steps):
            one(args.warmup + args.steps + i)
            if reducer is not None:
                reducer.comm_collect()
        torch.cuda.synchronize()
        if reducer is not None:
            reducer.profile = False
            comm = reducer.comm_summary()
            if comm is not None and eng.param_gather_stamps is not None:
                comm["param_gather_wait_ms_per_step"] = round(sum(a.elapsed_time(b) for a, b in eng.param_gather_stamps) / max(args.steps, 1), 4)
            eng.param_gather_stamps = None
        if use_dist:
            dist.barrier()
    if use_dist:
        tt = torch.tensor([dt], device=dev, dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        dt = float(tt)
    loss = float((lt[0] + lt[1] + lt[2]).sum().detach())
    ranks_equal = None
    if use_dist:
        # data-parallel invariant: after any number of steps every rank holds bit-identical parameters
        eng.wait_params()
        mine = torch.stack([eng.flat[k].float().sum() for k in ("decay", "nodecay")] + [eng.flat["decay"].float().abs().sum()])
        allv = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(allv, mine)
        ranks_equal = all(torch.equal(allv[0], v) for v in allv)
        if not ranks_equal and os.environ.get("VLP_BENCH_CHECK_RANKS", "1") == "1":
            raise SystemExit("rank parameter checksums differ: %s" % [v.tolist() for v in allv])
    prof, eng.prof = eng.prof, None

    # ---- second leg: the padding-free (packed) step (Engine.varlen) on the SAME batches, timed the same way.  `value`
    # above stays the dense run; this leg is reported under config.varlen with its EXECUTED work (rows, flops) beside it.
    varlen = None
    imbalance = None
    if not args.no_varlen and not env_varlen:
        eng.varlen = True
        step0 = args.warmup + 2 * args.steps
        for i in range(max(args.warmup, len(pool))):          # (the first pass over the pool derives the kept lengths from the masks: one read-back per batch)
            one(step0 + i)
        torch.cuda.synchronize()
        if use_dist:
            dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rows = 0
        for i in range(args.steps):
            lt_v = one(step0 + args.warmup + i)
            rows += eng.last_packed_rows or args.batch * (args.max_len_b + 103)
        torch.cuda.synchronize()
        if use_dist:
            dist.barrier()
        torch.cuda.synchronize()
        dtv = time.perf_counter() - t0
        vprof = None
        if not args.no_kernel_events:
            eng.prof = []
            for i in range(args.steps):
                one(step0 + args.warmup + args.steps + i)
            torch.cuda.synchronize()
            vprof, eng.prof = eng.prof, None
        if use_dist:
            tt = torch.tensor([dtv], device=dev, dtype=torch.float64)
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            dtv = float(tt)
            # load imbalance of the packed step: every rank's GEMMs run over ITS sum of kept lengths, the all-reduce waits for the busiest rank
            rr = torch.tensor([rows / max(args.steps, 1)], device=dev, dtype=torch.float64)
            allr = [torch.zeros_like(rr) for _ in range(world)]
            dist.all_gather(allr, rr)
            per_rank = [float(v) for v in allr]
            imbalance = {"max_over_mean_rows": round(max(per_rank) / (sum(per_rank) / world), 4), "rows_per_rank": [round(v, 1) for v in per_rank],
                         "note": "synthetic pools are seeded per rank (no loader): vlp_amd.data.balanced_epoch_order brings this to <= 1.001 on real shards"}
        eng.varlen = False
        # executed dense-contraction work per sample, fwd + bwd = 3 x fwd (SURVEY.md 8d's accounting on the KEPT rows): per kept position and layer
        # 7 077 888 GEMM MACs + 2 n_b H attention MACs; region projections and the LM head do not depend on the caption length
        H, NL = 768, args.layers
        gf = []
        for b in pool:
            m = b.input_mask
            n = ((m != 0).any(dim=1).to(torch.int32) * torch.arange(1, m.shape[-1] + 1, device=m.device, dtype=torch.int32)).amax(dim=1).clamp(min=102).double()
            enc = (n * NL * (7077888.0 + 2.0 * n * H) * 2.0).sum() / m.shape[0]
            gf.append(3.0 * (float(enc) + (1.153 + 0.247 + (0.137 if args.tasks != "vqa2" else 0.012)) * 1e9) / 1e9)
        ex_gflop = sum(gf) / len(gf)
        sps = world * args.batch * args.steps / dtv
        varlen = {"value": round(sps, 2), "unit": "samples/s", "ms_per_step": round(dtv / args.steps * 1e3, 3),
                  "real_rows_per_step": round(rows / args.steps, 1), "dense_rows_per_step": args.batch * (args.max_len_b + 103), "rank_imbalance": imbalance,
                  "executed_gflop_per_sample": round(ex_gflop, 3), "dense_gflop_per_sample": FLOP_PER_SAMPLE / 1e9,
                  "step_mfma_frac_executed": round(sps / world * ex_gflop * 1e9 / (MFMA_PEAK_TFLOPS * 1e12), 4),
                  "final_loss": round(float((lt_v[0] + lt_v[1] + lt_v[2]).sum().detach()), 4),
                  "note": "padding-free step: positions past a sample's last token (attended by nothing, read by no loss) are not computed; losses / "
                          "gradients equal the dense step's (tests/test_25_varlen_gpu.py); fractions use EXECUTED flops"}
        if vprof:
            ms = [max(a.elapsed_time(b) - (bracket[0] * 1e-3 if bracket else 0.0), 1e-6) for a, b, _ in vprof]      # same bracket-overhead correction as the dense leg
            fl = [f for _, _, f in vprof]
            ach = (sum(fl) / len(fl)) / (sum(ms) / len(ms) * 1e-3) / 1e12
            varlen["roofline"] = {"bound": "mfma", "kernel": "vlp_gemm_nt family at the packed row counts (executed flops per launch)", "achieved": round(ach, 1),
                                  "peak": MFMA_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": round(ach / MFMA_PEAK_TFLOPS, 4),
                                  "avg_launch_us": round(sum(ms) / len(ms) * 1e3, 2), "avg_gflop_per_launch": round(sum(fl) / len(fl) / 1e9, 3),
                                  "sampled_launches": len(vprof)}

    if args.tasks == "vqa2":
        shape_name = "VQA 2.0 fine-tune shape (bidirectional masks, P=1, answer-classifier head + BCE)"
    elif args.s2s_prob < 1.0:
        shape_name = "Conceptual Captions pre-training shape (per-sample seq2seq w.p. %.2f / bidirectional masks)" % args.s2s_prob
    else:
        shape_name = "COCO Captions fine-tune shape"
    if env_varlen:
        shape_name += " -- VLP_VARLEN=1: THIS LINE IS THE PADDING-FREE STEP (profiling run; flops-based fractions below assume dense work and overstate)"
    if rank == 0:
        roof = None
        if prof:
            ms = [a.elapsed_time(b) for a, b, _ in prof]
            flops = [f for _, _, f in prof]
            raw_us = sum(ms) / len(ms) * 1e3
            ovh_us = bracket[0] if bracket else 0.0          # what the event pair itself adds to a bracketed launch (measured live, see event_bracket_overhead_us)
            ms = [max(m - ovh_us * 1e-3, 1e-6) for m in ms]
            achieved = (sum(flops) / len(flops)) / (sum(ms) / len(ms) * 1e-3) / 1e12
            # HBM traffic of the same kernel comes from a separate rocprofv3 --pmc pass (counters cannot be read inside this
            # process): the newest profiles/rNN_pmc_traffic.json, produced by tools/gpu_pmc_bench.sh on the same command -- quoted
            # only if it was measured on the kernel sources of this build (otherwise null + the reason in `traffic_source`).
            traffic, traffic_src = committed_traffic()
            roof = {"bound": "mfma", "kernel": "vlp_gemm_nt (gemm_nt_kernel + gemm_nt_wp_kernel + gemm_nt_ps_kernel: all forward + dgrad GEMMs; every %dth launch bracketed by HIP events in a second, un-timed pass over the same steps)" % eng.PROF_EVERY, "achieved": round(achieved, 1),
                    "peak": MFMA_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": round(achieved / MFMA_PEAK_TFLOPS, 4), "traffic": traffic, "traffic_source": traffic_src,
                    "launches_per_step": len(prof) * eng.PROF_EVERY // max(args.steps, 1), "sampled_launches": len(prof),
                    "avg_launch_us": round(sum(ms) / len(ms) * 1e3, 2),
                    # the duration above = event-bracketed duration minus the bracket's own overhead, both measured live on the launch stream
                    "avg_launch_us_events_raw": round(raw_us, 2), "event_bracket_overhead_us": round(ovh_us, 2),
                    "event_bracket_calibration": ({"bracketed_single_us": round(bracket[1], 2), "back_to_back_us": round(bracket[2], 2),
                                                   "kernel": "vlp_gemm_nt 10688x768x768 variant 77, 40 launches each way"} if bracket else None),
                    "frac_events_raw": round((sum(flops) / len(flops)) / (raw_us * 1e-6) / 1e12 / MFMA_PEAK_TFLOPS, 4),
                    "rocprofv3": committed_rocprof_family(),
                    "avg_gflop_per_launch": round(sum(flops) / len(flops) / 1e9, 3),
                    "step_mfma_frac": round((world * args.batch * args.steps / dt) / world * FLOP_PER_SAMPLE / (MFMA_PEAK_TFLOPS * 1e12), 4)}
        out = {"metric": METRIC, "value": round(world * args.batch * args.steps / dt, 2), "unit": "samples/s", "n_gpus": world,
               "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(dt / args.steps * 1e3, 3), "higher_is_better": True,
               "scaling": "weak", "vs_baseline": None, "dtype": "f16", "data": "synthetic",
               "config": {"workload": "%s: BERT-base %dL, 100 regions x 2048-d, seq_len %d (L=%d), bs %d/GPU, "
                                      "fwd+bwd+FP16 FusedAdam, dropout 0.1, dynamic loss scale" % (shape_name, args.layers, args.max_len_b, args.max_len_b + 103, args.batch),
                          "global_batch": world * args.batch, "parallelism": "dp%d" % world, "final_loss": round(loss, 4),
                          "batch_pool": len(pool),       # distinct device-resident batches the steps cycle through (masks, lengths, cache contents repeat with this period)
                          "loss_scale": opt.cur_scale, "skipped_steps": opt.skipped_steps,
                          "rccl_ranks": dist.get_world_size() if use_dist else 1, "rank_param_checksums_equal": ranks_equal,
                          # "sharded" (VLP_DDP_MODE=sharded, N > 1): reduce-scatter, Adam on 1/N of the state per rank, parameter all-gather
                          "optimizer": "sharded" if getattr(eng, "shard_plan", None) is not None else "replicated",
                          # N > 1: how the gradient exchange was issued -- collective form, buckets (MB each, completion order), and the
                          # measured communication of rank 0 in the un-timed sampling pass: time the main stream stood still after backward's
                          # last kernel (exposed) vs collective time hidden under backward (overlapped); null when not distributed
                          "ddp_mode": model.reducer.mode if use_dist else None,
                          "buckets": ({"count": len(model.reducer.buckets) + 1, "mb": [round((hi - lo) * 2 / 2.0 ** 20, 4) for lo, hi in model.reducer.buckets]
                                       + [round(eng.gflat["nodecay"].numel() * 2 / 2.0 ** 20, 4)]} if use_dist else None),
                          "comm": comm,
                          "param_checksum": [float(eng.flat[k].float().sum()) for k in ("decay", "nodecay")] + [float(eng.flat["decay"].float().abs().sum())],
                          "varlen": varlen, "first_leg_packed": env_varlen},
               "roofline": roof, "parity": parity}
        if comm is not None and imbalance is not None:
            comm["imbalance"] = imbalance["max_over_mean_rows"]
        if os.environ.get("VLP_DEBUG_TUNE") == "1":  # noqa
            from vlp_amd.engine import Engine
            print("nt choices (M,N,K)->variant:", sorted(Engine._nt_choice.items()), file=sys.stderr)
            print("tn choices (M,N,K)->(variant,splits):", sorted(Engine._tn_choice.items()), file=sys.stderr)
        if world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline()
        print(json.dumps(out))
    if use_dist:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
