"""VQA 2.0 on real data, measured (12 layers, vocab 28 996, 100 regions, questions of up to 20 tokens, B = 64); writes profiles/vqa_bench.json
(OUT=... to put it elsewhere) and prints the same JSON:

    train_step        the VQA training step on a device-resident batch with the dense f32 [B, 3129] target and with SparseAnswers for the SAME
                      target (the two BCE launches differ, nothing else), padding-free (MaskSpec with host lengths);
    loader            BatchPrefetcher over VQA examples (answers scored on the host per batch), samples/s at 1 / 4 worker threads;
    eval              BertForPreTrainingLossMask.answer() at batch 64: questions/s (forward + one vlp_vqa_answer_rows launch + the read-back).

The loss kernels are microseconds inside a multi-millisecond step: these numbers are the record, no gain is claimed from them.
"""
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from vlp_amd import synthetic as S  # noqa: E402
from vlp_amd.data import BatchPrefetcher, PackedRegionStore, TextPreprocessor, write_packed  # noqa: E402
from vlp_amd.input_prep import MaskSpec, SparseAnswers  # noqa: E402
from vlp_amd.modeling import BertConfig, BertForPreTrainingLossMask  # noqa: E402
from vlp_amd.optimization_fp16 import FP16_Optimizer_State, FusedAdam  # noqa: E402
from vlp_amd.run_img2txt_dist import train_step  # noqa: E402

dev = torch.device("cuda:0")
B, T, NA = int(os.environ.get("B", 64)), 20, 3129
STEPS, N = int(os.environ.get("STEPS", 30)), int(os.environ.get("N_IMAGES", 512))
rng = np.random.RandomState(0)
out = {"batch": B, "layers": 12, "max_len_b": T, "steps_timed": STEPS}


def answers_of(n):
    """n questions' answer lists with VQA-like agreement: 1 - 4 distinct answers among 10, some unknown (index 0)."""
    rows = []
    for _ in range(n):
        pool = rng.choice(NA, size=rng.randint(1, 5), replace=False)
        rows.append([int(pool[min(rng.geometric(0.6) - 1, len(pool) - 1)]) for _ in range(10)])
    return rows


cfg = BertConfig(28996, num_hidden_layers=12, type_vocab_size=6)
model = BertForPreTrainingLossMask(cfg, enable_butd=True, len_vis_input=100, tasks="vqa2", allow_random_fc7=True).half().to(dev).train()
named = list(model.named_parameters())
nd = ["bias", "LayerNorm.bias", "LayerNorm.weight"]
groups = [{"params": [p for n_, p in named if not any(x in n_ for x in nd)], "weight_decay": 0.01},
          {"params": [p for n_, p in named if any(x in n_ for x in nd)], "weight_decay": 0.0}]
opt = FP16_Optimizer_State(FusedAdam(groups, lr=1e-5, bias_correction=False, max_grad_norm=1.0), dynamic_loss_scale=True,
                           dynamic_loss_args={"init_scale": 1.0})

# ---- training step: dense against sparse targets --------------------------------------------------------------------------------
raw = S.make_batch(B, max_len_b=T, vocab_size=28996, max_pred=1, tasks="vqa2", seed=1)
nb = [int(raw.input_mask[i].any(dim=0).sum()) - 103 for i in range(B)]
sa = SparseAnswers.from_answer_ids(answers_of(B))
batch = S.batch_to(raw, dev, half=True)._replace(input_mask=MaskSpec.from_lengths(100, nb, False, device=dev))
variants = {"dense_targets": batch._replace(ans_labels=sa.dense(NA).to(dev)), "sparse_targets": batch._replace(ans_labels=sa.to(dev))}


def time_steps(b, n):
    for _ in range(5):
        train_step(model, opt, b, 1e-5)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        train_step(model, opt, b, 1e-5)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


out["train_step"] = {"packed_rows": None, "ms_per_step": {k: [] for k in variants}}
for rep in range(3):                        # interleaved repeats: the spread between repeats is the noise the difference has to be read against
    for name, b in variants.items():
        out["train_step"]["ms_per_step"][name].append(round(time_steps(b, STEPS), 4))
out["train_step"]["packed_rows"] = model.engine.last_packed_rows
out["train_step"]["samples_per_s"] = {k: round(B / (min(v) * 1e-3), 1) for k, v in out["train_step"]["ms_per_step"].items()}

# ---- loader with answers ------------------------------------------------------------------------------------------------------------
with tempfile.TemporaryDirectory() as d:
    feats = np.abs(rng.standard_normal((N, 100, 2048))).astype(np.float16)
    cls = rng.rand(N, 100, 1601).astype(np.float16)
    xy1 = rng.uniform(0, 400, size=(N, 100, 2))
    box = np.concatenate((xy1, xy1 + rng.uniform(10, 200, size=(N, 100, 2)), rng.rand(N, 100, 1), rng.uniform(0.2, 1, size=(N, 100, 1))), axis=2).astype(np.float32)
    ids = ["img%06d" % i for i in range(N)]
    write_packed(d, ids, feats, cls, box)
    del feats, cls, box
    store = PackedRegionStore(d)
    ans = answers_of(5 * N)
    examples = [(ids[i % N], rng.randint(1000, 28000, size=rng.randint(4, T + 1)).tolist(), ans[i], i) for i in range(5 * N)]
    kw = dict(max_pred=1, mask_prob=0.0, vocab_size=28996, cls_id=S.CLS_ID, sep_id=S.SEP_ID, mask_id=S.MASK_ID, unk_id=S.UNK_ID, max_len=100 + T + 3,
              max_len_b=T)
    p_s2s, p_bi = TextPreprocessor(mode="s2s", **kw), TextPreprocessor(mode="bi", **kw)
    out["loader"] = {"host_cpus": len(os.sched_getaffinity(0)), "samples_per_s": {}, "samples_per_s_caption_examples": {}}
    for key, exs in (("samples_per_s", examples), ("samples_per_s_caption_examples", [(e[0], e[1]) for e in examples])):
        for w in (1, 4):
            pf = BatchPrefetcher(store, exs, B, p_s2s, p_bi, s2s_prob=0.0, device=dev, steps=STEPS, seed=0, num_workers=w)
            for _ in pf:                # warm the page cache / pinned slots once
                break
            t0 = time.perf_counter()
            n = 0
            for _ in pf:
                n += 1
            torch.cuda.synchronize()
            out["loader"][key][str(w)] = round(n * B / (time.perf_counter() - t0), 1)

# ---- evaluation ---------------------------------------------------------------------------------------------------------------------
model.eval()
b = variants["sparse_targets"]
with torch.no_grad():
    for _ in range(3):
        model.answer(b.img, b.vis_pe, b.input_ids, b.segment_ids, b.input_mask, answers=b.ans_labels)[0].tolist()
    t0 = time.perf_counter()
    for _ in range(STEPS):
        model.answer(b.img, b.vis_pe, b.input_ids, b.segment_ids, b.input_mask, answers=b.ans_labels)[0].tolist()      # (the read-back eval_vqa2 does per batch)
    dt = (time.perf_counter() - t0) / STEPS
out["eval"] = {"ms_per_batch": round(dt * 1e3, 3), "questions_per_s": round(B / dt, 1), "packed_rows": model.engine.last_packed_rows}

path = os.environ.get("OUT", os.path.join(ROOT, "profiles", "vqa_bench.json"))
with open(path, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print(json.dumps(out))
