"""Per-phase timing of one self-critical (--scst) training step on one MI355X -> profiles/scst_step.json.

    python tools/scst_bench.py [--batches 16 64] [--steps 5] [--warmup 2] [--reward host|device] [--refs R] [--df N] [--samples K]
                               [--cider_weight W] [--bleu_weight W] [--out profiles/scst_step.json]

Every step is the entry script's own vlp_amd.run_img2txt_dist.scst_step (the model's sample_mode paths, the reward, RewardCriterion, the fp16
optimizer) at L = 123 (COCO's --max_len_b 20), 12 layers, the bert-base-cased vocabulary, on a seeded synthetic batch.  scst_step reports the
end of each phase through its `mark` hook; the tool additionally marks the entry of Engine.score_samples, which splits the model's sampled
forward into its two halves:
  greedy_decode    eval() + no_grad greedy decode (the baseline captions; graph-planned token steps)
  sample_decode    the sampled decode of the train() forward (not graph-planned: its seed changes every step)
  score_fwd        Engine.score_samples: scoring layout + training forward + LM head + log-probs
  reward_host      caption cleaning, one device -> host copy, CIDEr-D of 2B captions on the host, the rewards back
  reward_device    (--reward device, in place of reward_host) caption cleaning and the vlp_cider_d kernels; nothing leaves the device
  score_bwd        RewardCriterion and the backward of the scoring forward
  optimizer        FP16_Optimizer_State(FusedAdam).step()
Each mark synchronises the device first (host wall clock), so phases do not overlap; their sum is a serialised step.  Nothing is asserted:
this records what is measured.
--refs R > 1 scores every sample against R references (a CaptionRefs: the sample's ground truth and R - 1 seeded synthetic captions of the
same lengths) instead of its one ground truth.  The default --out is profiles/scst_step.json for the default mode (--reward host --refs 1)
and profiles/scst_reward_device.json otherwise; a run ADDS its records to the runs of an existing --out file (each names its reward and
refs), so the four modes of one session end up in one record.
--df N > 0 passes scst_step a document-frequency table (--scst_df; vlp_amd.scst.DocFreq) of N seeded n-grams over 113287 documents (COCO's
train + restval images), so that the reward phase is the table path's: a binary search of depth log2 N per n-gram on the device, the same
search per n-gram on the host.  Its default --out is profiles/scst_reward_df.json; each record names its df_ngrams (0 = no table).
--samples K >= 2 times the step of --scst_samples K: K samples per image with a leave-one-out baseline.  There is no greedy_decode phase;
sample_decode is Engine.decode_sample_group (K*B rows, graph-planned token steps), score_fwd / score_bwd run over K*B sequences and the
reward phase scores K*B captions.  --batches stays the number of images.  Its default --out is profiles/scst_samples.json; each record names
its samples (1 = the one-sample estimator above) and its sample_decode_token_step_ms (the phase over the T token steps).
--cider_weight / --bleu_weight other than 1 / 0 time the step of --scst_cider_weight / --scst_bleu_weight: the reward phase then scores sentence
BLEU-4 as well (vlp_bleu4 on the device, vlp_amd.scst.Bleu on the host).  With 1 / 0 scst_step is called without the keyword, as before.  Their
default --out is profiles/scst_bleu.json; each record names its reward_weights.
--temperature / --entropy_weight other than 1 / 0 time the step of --scst_temperature / --scst_entropy_weight: score_fwd then ends with
vlp_token_policy_fwd and score_bwd starts with vlp_token_policy_bwd.  Their default --out is profiles/scst_policy.json; each record names its
temperature and entropy_weight."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vlp_amd import run_img2txt_dist as R          # noqa: E402
from vlp_amd import synthetic as S                 # noqa: E402
from vlp_amd.modeling import BertConfig, BertForSeq2SeqDecoder   # noqa: E402
from vlp_amd.optimization_fp16 import FP16_Optimizer_State, FusedAdam   # noqa: E402
from vlp_amd.scst import RewardCriterion           # noqa: E402

PHASES = ("greedy_decode", "sample_decode", "score_fwd", "reward_host", "score_bwd", "optimizer")
RENAME = {"sample_forward": "score_fwd", "backward": "score_bwd"}      # scst_step's phase names -> the finer ones above
NOTE = ("every phase ends with a device synchronisation (host wall clock), so phases do not overlap; sample_decode is not graph-planned "
        "(its seed changes every step)")


def with_refs(batch, R, dev, seed=11):
    """The batch with a CaptionRefs of R references per sample in its 12th slot: row 0 the sample's own ground-truth ids, rows 1..R-1 the
    same rows with their words redrawn (same lengths, [SEP] and padding kept)."""
    from vlp_amd.input_prep import CaptionRefs
    gt = batch.input_ids[:, 102:]
    g = torch.Generator().manual_seed(seed)
    rows = [gt]
    for _ in range(R - 1):
        words = torch.randint(1000, 1200, gt.shape, generator=g).to(dev)
        rows.append(torch.where((gt != 0) & (gt != S.SEP_ID), words, gt))
    refs = CaptionRefs(torch.stack(rows, 1).contiguous(), torch.full((gt.shape[0],), R, dtype=torch.int32, device=dev))
    return batch._replace(ans_labels=refs)


def seeded_table(n, n_docs=113287, vocab=28996, seed=5):
    """A DocFreq of (about) n distinct seeded n-grams of orders 1..4 over the vocabulary, df uniform in 1..n_docs."""
    from vlp_amd.scst import DocFreq
    rng = np.random.RandomState(seed)
    ids = rng.randint(0, vocab, size=(n, 4)).astype(np.uint64) + np.uint64(1)
    order = rng.randint(1, 5, size=n)
    key = np.zeros(n, dtype=np.uint64)
    for j in range(4):
        key |= np.where(order > j, ids[:, j], np.uint64(0)) << np.uint64(48 - 16 * j)
    key = np.unique(key)
    return DocFreq(key, rng.randint(1, n_docs + 1, size=len(key)).astype(np.int32), n_docs, 20, S.SEP_ID)


def bench(B, steps, warmup, dev, reward="host", refs=1, df=None, samples=1, weights=(1.0, 0.0), temperature=1.0, entropy_weight=0.0):
    cfg = BertConfig(28996, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1, type_vocab_size=6)
    torch.manual_seed(0)
    m = BertForSeq2SeqDecoder(cfg, mask_word_id=S.MASK_ID, eos_id=S.SEP_ID, enable_butd=True, len_vis_input=100).half().to(dev)
    named = list(m.named_parameters())
    nd = ["bias", "LayerNorm.bias", "LayerNorm.weight"]
    groups = [{"params": [q for n, q in named if not any(x in n for x in nd)], "weight_decay": 0.01},
              {"params": [q for n, q in named if any(x in n for x in nd)], "weight_decay": 0.0}]
    opt = FP16_Optimizer_State(FusedAdam(groups, lr=1e-6, bias_correction=False, max_grad_norm=1.0), dynamic_loss_scale=True)
    batch = S.batch_to(S.make_batch(B, max_len_b=20, len_vis_input=100, max_pred=0, mask_prob=0.0, seed=7), dev, half=True)
    if refs > 1:
        batch = with_refs(batch, refs, dev)
    crit = RewardCriterion()
    phases = tuple("reward_device" if (k == "reward_host" and reward == "device") else k for k in PHASES if samples == 1 or k != "greedy_decode")
    times = {k: [] for k in phases}
    clock = {"t": 0.0, "rec": False}

    def mark(phase):
        torch.cuda.synchronize()
        now = time.perf_counter()
        if clock["rec"] and phase is not None:
            times[RENAME.get(phase, phase)].append((now - clock["t"]) * 1e3)
        clock["t"] = now

    eng = m.engine
    score = eng.score_samples

    def score_marked(*a, **kw):             # the model's sampled forward calls this after its decode
        mark("sample_decode")
        return score(*a, **kw)
    eng.score_samples = score_marked
    for it in range(warmup + steps):
        clock["rec"] = it >= warmup
        mark(None)                          # the step starts here
        R.scst_step(m, opt, batch, 1e-6, 100, crit, mark=mark, reward_on=reward, df=df, **({"samples": samples} if samples > 1 else {}),
                    **({"reward_weights": weights} if tuple(weights) != (1.0, 0.0) else {}),
                    **({"temperature": temperature} if temperature != 1.0 else {}), **({"entropy_weight": entropy_weight} if entropy_weight else {}))
    L = batch.input_ids.shape[1]
    out = {k: {"median_ms": float(np.median(v)), "min_ms": float(np.min(v))} for k, v in times.items()}
    out["step_ms_sum_of_medians"] = float(sum(out[k]["median_ms"] for k in phases))
    out.update(B=B, L=L, T=L - 102, scoring_length=102 + 2 * (L - 102) - 1, layers=12, vocab=28996, steps=steps, warmup=warmup, reward=reward, refs=refs,
               df_ngrams=0 if df is None else len(df), samples=samples, reward_weights=list(weights), temperature=temperature,
               entropy_weight=entropy_weight, sample_decode_token_step_ms=out["sample_decode"]["median_ms"] / (L - 102))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reward", default="host", choices=["host", "device"], help="where scst_step computes the CIDEr-D reward")
    ap.add_argument("--refs", type=int, default=1, help="references per sample (1 = the sample's ground truth, as the entry script's default)")
    ap.add_argument("--df", type=int, default=0, metavar="N", help="score with a document-frequency table of N seeded n-grams (0 = the step's own references)")
    ap.add_argument("--samples", type=int, default=1, metavar="K", help="samples per image (--scst_samples): 1 = one sample against a greedy decode, "
                                                                        "2..16 = K samples with a leave-one-out baseline")
    ap.add_argument("--cider_weight", type=float, default=1.0, help="the weight of CIDEr-D in the reward (--scst_cider_weight)")
    ap.add_argument("--bleu_weight", type=float, default=0.0, help="the weight of sentence BLEU-4 in the reward (--scst_bleu_weight); 0 = CIDEr-D alone")
    ap.add_argument("--temperature", type=float, default=1.0, help="the temperature of the sampled policy (--scst_temperature)")
    ap.add_argument("--entropy_weight", type=float, default=0.0, help="the weight of the entropy bonus (--scst_entropy_weight); 0 = off")
    ap.add_argument("--out", default=None, help="default: profiles/scst_policy.json with --temperature / --entropy_weight other than 1 / 0, else "
                                                "profiles/scst_step.json for --reward host --refs 1, profiles/scst_reward_df.json with --df, "
                                                "profiles/scst_samples.json with --samples above 1, "
                                                "profiles/scst_bleu.json with reward weights other than 1 / 0, else profiles/scst_reward_device.json")
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "scst_policy.json" if (a.temperature, a.entropy_weight) != (1.0, 0.0) else "scst_bleu.json" if (a.cider_weight, a.bleu_weight) != (1.0, 0.0) else "scst_samples.json" if a.samples > 1 else "scst_reward_df.json" if a.df else
                             "scst_step.json" if (a.reward == "host" and a.refs == 1) else "scst_reward_device.json")
    dev = torch.device("cuda")
    tool = "tools/scst_bench.py --batches %s --steps %d --warmup %d --reward %s --refs %d" % (" ".join(map(str, a.batches)), a.steps, a.warmup, a.reward,
                                                                                             a.refs) + (" --df %d" % a.df if a.df else "") + (" --samples %d" % a.samples if a.samples > 1 else "") + (
        " --cider_weight %g --bleu_weight %g" % (a.cider_weight, a.bleu_weight) if (a.cider_weight, a.bleu_weight) != (1.0, 0.0) else "") + (
        " --temperature %g --entropy_weight %g" % (a.temperature, a.entropy_weight) if (a.temperature, a.entropy_weight) != (1.0, 0.0) else "")
    df = seeded_table(a.df) if a.df else None
    res = {"device": torch.cuda.get_device_name(0), "note": NOTE, "runs": []}
    yardstick = os.path.realpath(a.out) == os.path.realpath(os.path.join(ROOT, "profiles", "scst_step.json"))
    if yardstick:                                 # the single-mode record of the default path: always written afresh
        res["tool"] = tool
    else:
        res["tools"] = []
        if os.path.exists(a.out):
            with open(a.out) as f:
                old = json.load(f)
            for k, v in old.items():              # earlier runs, and what tests/test_81_scst_reward_gpu.py's report() keeps under "test_81"
                if k not in ("device", "note"):
                    res[k] = v
        res["tools"].append(tool)
    for B in a.batches:
        r = bench(B, a.steps, a.warmup, dev, a.reward, a.refs, df, a.samples, (a.cider_weight, a.bleu_weight), a.temperature, a.entropy_weight)
        print(json.dumps(r, sort_keys=True), flush=True)
        res["runs"].append(r)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=2, sort_keys=True)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
