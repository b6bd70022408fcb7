"""MI355X drop-in for `vlp/run_img2txt_dist.py` (the reference's fine-tuning / pre-training entry point).

Same command line as the reference (every flag of run_img2txt_dist.py:47-188 is accepted with the same
default), same per-process launch style (`--local_rank k --global_rank k --world_size N`, file:// rendezvous,
README.md:139-155) and same step loop (:453-586): forward -> summed loss -> (scaled) backward -> warmup_linear
learning rate -> optimizer step -> zero_grad, per-epoch checkpoint `model.{epoch}.bin` on rank 0 (:588-599),
barrier (:604-605).  What differs is underneath: the model / optimizer / DDP come from vlp_amd (HIP kernels
behind libvlp_hip.so, RCCL gradient buckets) instead of torch autograd + apex + torch DDP.

Data: the reference's loader (vlp/seq2seq_loader.py) needs h5py/torchvision and the COCO/CC/VQA feature
files, none of which exist on the build or bench machines; it is the ranked-next row N3 of SURVEY.md 8(f).
`--synthetic STEPS_PER_EPOCH` feeds seeded synthetic batches that follow the same 12-tuple contract
(vlp_amd/synthetic.py); without it the script stops with a clear message.

Launched by torchrun (RANK / LOCAL_RANK / WORLD_SIZE in the environment) it takes ranks from there.
"""
import argparse
import copy
import glob
import json
import logging
import math
import os
import random
import time
from pathlib import Path

import numpy as np
import torch

from . import synthetic
from .distributed import DistributedDataParallel as DDP
from .input_prep import CaptionRefs, MaskSpec
from .modeling import BertConfig, BertForPreTrainingLossMask, BertForSeq2SeqDecoder, load_checkpoint_state
from .optimization import BertAdam, warmup_linear           # noqa: F401  (re-exported like the reference imports them)
from .optimization_fp16 import FP16_Optimizer_State, FusedAdam

KNOWN_VOCABS = {"bert-base-cased": 28996, "bert-large-cased": 28996, "bert-base-uncased": 30522, "bert-large-uncased": 30522}


def _get_max_epoch_model(output_dir):   # reference :33-43
    fn_model_list = glob.glob(os.path.join(output_dir, "model.*.bin"))
    fn_optim_list = glob.glob(os.path.join(output_dir, "optim.*.bin"))
    if (not fn_model_list) or (not fn_optim_list):
        return None
    both = set(int(Path(fn).stem.split(".")[-1]) for fn in fn_model_list) & set(int(Path(fn).stem.split(".")[-1]) for fn in fn_optim_list)
    return max(both) if both else None


def _to_cpu(x):
    if torch.is_tensor(x):
        return x.detach().cpu()
    if isinstance(x, dict):
        return {k: _to_cpu(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return type(x)(_to_cpu(v) for v in x)
    return x


def build_parser():
    p = argparse.ArgumentParser()
    # General (same names / defaults as the reference)
    p.add_argument("--bert_model", default="bert-base-cased", type=str)
    p.add_argument("--config_path", default=None, type=str)
    p.add_argument("--output_dir", default="tmp", type=str)
    p.add_argument("--log_file", default="training.log", type=str)
    p.add_argument("--model_recover_path", default=None, type=str)
    p.add_argument("--do_train", action="store_true")
    p.add_argument("--do_lower_case", action="store_true")
    p.add_argument("--train_batch_size", default=64, type=int)
    p.add_argument("--learning_rate", default=3e-5, type=float)
    p.add_argument("--label_smoothing", default=0, type=float)
    p.add_argument("--weight_decay", default=0.01, type=float)
    p.add_argument("--finetune_decay", action="store_true")
    p.add_argument("--num_train_epochs", default=30, type=int)
    p.add_argument("--warmup_proportion", default=0.1, type=float)
    p.add_argument("--no_cuda", action="store_true")
    p.add_argument("--local_rank", type=int, default=-1)
    p.add_argument("--global_rank", type=int, default=-1)
    p.add_argument("--seed", type=int, default=42)
    p.add_argument("--gradient_accumulation_steps", type=int, default=1)
    p.add_argument("--fp16", action="store_true")
    p.add_argument("--fp32_embedding", action="store_true")
    p.add_argument("--loss_scale", type=float, default=0)
    p.add_argument("--amp", action="store_true")
    p.add_argument("--from_scratch", action="store_true")
    p.add_argument("--new_segment_ids", action="store_true")
    p.add_argument("--tokenized_input", action="store_true")
    p.add_argument("--len_vis_input", type=int, default=100)
    p.add_argument("--max_len_b", type=int, default=20)
    p.add_argument("--trunc_seg", default="b")
    p.add_argument("--always_truncate_tail", action="store_true")
    p.add_argument("--mask_prob", default=0.15, type=float)
    p.add_argument("--max_pred", type=int, default=3)
    p.add_argument("--num_workers", default=4, type=int)
    p.add_argument("--max_position_embeddings", type=int, default=None)
    # Others for VLP
    p.add_argument("--src_file", default=["/mnt/dat/COCO/annotations/dataset_coco.json"], type=str, nargs="+")
    p.add_argument("--enable_visdom", action="store_true")
    p.add_argument("--visdom_port", type=int, default=8888)
    p.add_argument("--image_root", type=str, default="/mnt/dat/COCO/images")
    p.add_argument("--dataset", default="coco", type=str)
    p.add_argument("--split", type=str, nargs="+", default=["train", "restval"])
    p.add_argument("--world_size", default=1, type=int)
    p.add_argument("--dist_url", default="file://[PT_OUTPUT_DIR]/nonexistent_file", type=str)
    p.add_argument("--file_valid_jpgs", default="/mnt/dat/COCO/annotations/coco_valid_jpgs.json", type=str)
    p.add_argument("--sche_mode", default="warmup_linear", type=str)
    p.add_argument("--drop_prob", default=0.1, type=float)
    p.add_argument("--use_num_imgs", default=-1, type=int)
    p.add_argument("--vis_mask_prob", default=0, type=float)
    p.add_argument("--max_drop_worst_ratio", default=0, type=float)
    p.add_argument("--drop_after", default=6, type=int)
    p.add_argument("--s2s_prob", default=1, type=float)
    p.add_argument("--bi_prob", default=0, type=float)
    p.add_argument("--enable_butd", action="store_true")
    p.add_argument("--region_bbox_file", default="coco_detection_vg_thresh0.2_feat_gvd_checkpoint_trainvaltest.h5", type=str)
    p.add_argument("--region_det_file_prefix", default="feat_cls_1000/coco_detection_vg_100dets_gvd_checkpoint_trainval", type=str)
    p.add_argument("--tasks", default="img2txt")
    p.add_argument("--relax_projection", action="store_true")
    p.add_argument("--scst", action="store_true")
    # vlp_amd additions
    p.add_argument("--synthetic", type=int, default=0, metavar="STEPS_PER_EPOCH",
                   help="train on seeded synthetic batches (vlp_amd/synthetic.py) for this many steps per epoch")
    p.add_argument("--packed_features", default="", help="directory of a vlp_amd.data packed region store (write_packed / pack_from_h5)")
    p.add_argument("--token_file", default="", help="json list of [image id, [caption token ids]] (captions pre-tokenised with the "
                                                     "reference's WordPiece vocabulary), or for --tasks vqa2 of [image id, [question token ids], "
                                                     "[answer ids], question id] (vlp_amd.data.vqa_examples_from_imdb); used with --packed_features")
    p.add_argument("--num_hidden_layers", type=int, default=None, help="override the config's depth (plumbing tests)")
    p.add_argument("--optim_format", default="vlp", choices=["vlp", "apex"],
                   help="layout of optim.N.bin: 'vlp' = the engine's flat buffers (+ dropout stream position: bit-exact resume), 'apex' = the "
                        "reference stack's FP16_Optimizer(FusedAdam) state_dict, loadable by the reference; both are accepted on resume")
    p.add_argument("--stop_after_epoch", type=int, default=0, help="stop after this epoch (schedule still spans --num_train_epochs); 0 = off")
    p.add_argument("--log_every", type=int, default=100, help="steps between loss read-backs (each read-back is a host sync)")
    p.add_argument("--allow_fp16_compute", action="store_true",
                   help="without --fp16 the reference trains in fp32 under BertAdam (run_img2txt_dist.py:421-426; its README's `--amp` commands do "
                        "exactly that, because amp only engages together with --fp16, :305).  vlp_amd has no fp32 compute path: this switch runs "
                        "that command line with fp16 storage / fp32 accumulate and BertAdam on fp32 master weights (static loss scale --loss_scale, "
                        "default 1024)")
    p.add_argument("--no_padding_free", action="store_true",
                   help="compute all L positions of every sample like the reference does; by default positions past a sample's last token "
                        "(attended by nothing, read by no loss) are not computed when the batch says where they start (DESIGN.md section 7)")
    p.add_argument("--shard_order", default="balanced", choices=["balanced", "reference"],
                   help="world_size > 1 with --packed_features: 'balanced' deals every global batch (DistributedSampler's sample set) to the ranks "
                        "by caption length so that padding-free row counts per rank match; 'reference' is DistributedSampler's index order bit for bit")
    p.add_argument("--scst_reward", default="host", choices=["host", "device"],
                   help="--scst: where the CIDEr-D reward is computed.  'host' is the reference's way (the cleaned ids are copied to the host and "
                        "scored there, vlp_amd.scst.CiderD); 'device' scores them with the vlp_cider_d kernels: same reward to fp32 rounding, no "
                        "host synchronisation between the sampled decode and the backward")
    p.add_argument("--scst_refs", default="caption", choices=["caption", "image"],
                   help="--scst: the references of the reward.  'caption' is the reference's recipe: the one caption the loader drew for the "
                        "sample.  'image' scores against up to 5 captions of the sample's image (all of COCO's), which is how CIDEr is defined -- a "
                        "deliberate departure from the reference's objective; needs --packed_features (the loader collects the captions per "
                        "image id from --token_file)")
    p.add_argument("--scst_samples", type=int, default=1, metavar="K",
                   help="--scst: samples drawn per image.  1 is the reference's estimator: one sample against a greedy decode.  K in 2..16 draws K "
                        "samples per image and baselines each with the mean reward of the other K - 1 (leave-one-out): no greedy decode, lower "
                        "variance -- a deliberate departure from the reference's estimator.  --train_batch_size stays the number of images per "
                        "step; K x that many sequences (at most 1024) are decoded and scored")
    p.add_argument("--scst_df", default="batch", metavar="{batch,train,PATH}",
                   help="--scst: the document frequencies of the CIDEr-D reward.  'batch' is the reference's Cider(df='corpus'): counted over the "
                        "references of each step.  'train' counts them once at start-up over ALL captions of --token_file, one document per image "
                        "(vlp_amd.scst.DocFreq; needs --packed_features and a caption --token_file; every rank builds the same table from the whole "
                        "list); a PATH loads a table saved by `python -m vlp_amd.cider_df` (its --max_len_b and [SEP] id must be this run's).  A "
                        "deliberate departure from the reference's objective, like --scst_refs image; works with either --scst_reward and either "
                        "--scst_refs (with 'device' the table is uploaded once and stays resident)")
    p.add_argument("--scst_cider_weight", type=float, default=1.0, metavar="W",
                   help="--scst: the reward of a caption is W x CIDEr-D + --scst_bleu_weight x sentence BLEU-4 (the usual self-critical recipe; "
                        "CIDEr-D here is on its 0..10 scale, BLEU-4 on 0..1).  1 and 0, the defaults, are the reference's CIDEr-D-only reward")
    p.add_argument("--scst_bleu_weight", type=float, default=0.0, metavar="W",
                   help="--scst: the weight of sentence BLEU-4 (coco-caption's per-sentence BLEU with the closest reference length, "
                        "vlp_amd.scst.Bleu) in the reward; 0 = off.  Works with either --scst_reward (on the device one more kernel, vlp_bleu4, "
                        "scores, mixes and baselines), either --scst_refs, any --scst_df (which keeps applying to CIDEr-D only) and any "
                        "--scst_samples.  Weights must be finite and not negative, and not both 0")
    p.add_argument("--scst_temperature", type=float, default=1.0, metavar="T",
                   help="--scst: the sampled captions are drawn from softmax(logits / T) and the policy gradient differentiates that same "
                        "tempered policy (vlp_token_policy_fwd / _bwd); the greedy baseline of --scst_samples 1 does not depend on it.  T must be "
                        "finite and > 0; 1, the default, is the reference's policy")
    p.add_argument("--scst_entropy_weight", type=float, default=0.0, metavar="W",
                   help="--scst: subtracts W x the mean entropy of the sampled policy (over the positions RewardCriterion counts) from the loss, "
                        "the usual remedy when the samples collapse onto the greedy caption; the entropy and its gradient come from the scoring "
                        "pass's vocabulary-row kernels and the training log carries the mean entropy.  W must be finite and >= 0; 0 = off.  Both "
                        "flags combine freely with --scst_samples, --scst_reward, --scst_refs, --scst_df and the reward weights")
    return p


def derive_args(args):
    """Derived fields + the reference's argument checks (:193-209, :238-243)."""
    if "RANK" in os.environ and args.global_rank == -1:     # torchrun style launch
        args.global_rank = int(os.environ["RANK"])
        args.local_rank = int(os.environ.get("LOCAL_RANK", 0))
        args.world_size = int(os.environ.get("WORLD_SIZE", 1))
        if args.dist_url.startswith("file://[PT_OUTPUT_DIR]"):
            args.dist_url = "env://"
    args.max_seq_length = args.max_len_b + args.len_vis_input + 3     # +3 for 2x[SEP] and [CLS]
    args.mask_image_regions = args.vis_mask_prob > 0
    args.dist_url = args.dist_url.replace("[PT_OUTPUT_DIR]", args.output_dir)
    assert args.tasks in ("img2txt", "vqa2")
    assert args.enable_butd is True, "only support region attn! featmap attn deprecated"
    assert (not args.scst) or args.dataset == "coco", "scst support on coco only!"
    if args.scst:                                        # :201-204
        assert args.max_pred == 0 and args.mask_prob == 0, "no mask for scst!"
    if args.scst_refs == "image" and not (args.scst and args.packed_features):
        raise ValueError("--scst_refs image needs --scst and --packed_features (the captions of an image come from the packed loader)")
    if not 1 <= args.scst_samples <= 16:
        raise ValueError("--scst_samples %d: 1 (the reference's estimator) or 2..16 samples per image" % args.scst_samples)
    if args.scst_samples > 1:
        if not args.scst:
            raise ValueError("--scst_samples %d needs --scst (it chooses the estimator of self-critical training)" % args.scst_samples)
        per_step = args.train_batch_size // max(args.gradient_accumulation_steps, 1)
        if args.scst_samples * per_step > 1024:
            raise ValueError("--scst_samples %d x %d images per step = %d sequences; the sampled decode takes at most 1024: lower --train_batch_size "
                             "or --scst_samples, or raise --gradient_accumulation_steps" % (args.scst_samples, per_step, args.scst_samples * per_step))
    if args.scst_df != "batch":
        if not args.scst:
            raise ValueError("--scst_df %s needs --scst (it chooses the document frequencies of the SCST reward)" % args.scst_df)
        if args.scst_df == "train" and not (args.packed_features and args.token_file):
            raise ValueError("--scst_df train needs --packed_features and a caption --token_file (the table is counted over the captions of "
                             "--token_file); or give the path of a table saved by `python -m vlp_amd.cider_df`")
        if args.scst_df != "train" and not os.path.isfile(args.scst_df):
            raise ValueError("--scst_df: 'batch', 'train' or the path of a saved table; there is no file %s" % args.scst_df)
    if (args.scst_cider_weight, args.scst_bleu_weight) != (1.0, 0.0):
        if not args.scst:
            raise ValueError("--scst_cider_weight / --scst_bleu_weight need --scst (they weigh the two metrics of the SCST reward)")
        from .scst import check_reward_weights
        try:
            check_reward_weights(args.scst_cider_weight, args.scst_bleu_weight)
        except ValueError as e:
            raise ValueError("--scst_cider_weight %r --scst_bleu_weight %r: %s" % (args.scst_cider_weight, args.scst_bleu_weight, e))
    if not (0.0 < args.scst_temperature < float("inf")):
        raise ValueError("--scst_temperature %r: the temperature of the sampled policy must be finite and > 0" % args.scst_temperature)
    if not (0.0 <= args.scst_entropy_weight < float("inf")):
        raise ValueError("--scst_entropy_weight %r: the weight of the entropy bonus must be finite and >= 0" % args.scst_entropy_weight)
    if args.scst_temperature != 1.0 and not args.scst:
        raise ValueError("--scst_temperature %r needs --scst (it is the temperature of the policy self-critical training samples)" % args.scst_temperature)
    if args.scst_entropy_weight != 0.0 and not args.scst:
        raise ValueError("--scst_entropy_weight %r needs --scst (it weighs the entropy bonus of the self-critical loss)" % args.scst_entropy_weight)
    if args.gradient_accumulation_steps < 1:
        raise ValueError("Invalid gradient_accumulation_steps parameter: {}, should be >= 1".format(args.gradient_accumulation_steps))
    args.train_batch_size = int(args.train_batch_size / args.gradient_accumulation_steps)
    return args


def check_scst_start(args, recover_step):
    """:322: SCST fine-tunes a maximum-likelihood checkpoint (--model_recover_path, or a resume of this output directory)."""
    if (recover_step is None) and (args.model_recover_path is None):
        assert args.scst is False, "must init from maximum likelihood training"


def model_config(args):
    cfg_file = args.config_path or (os.path.join(args.bert_model, "bert_config.json") if os.path.isdir(args.bert_model) else None)
    if cfg_file:
        config = BertConfig.from_json_file(cfg_file)
    elif args.bert_model in KNOWN_VOCABS:
        large = "large" in args.bert_model
        config = BertConfig(KNOWN_VOCABS[args.bert_model], hidden_size=1024 if large else 768, num_hidden_layers=24 if large else 12,
                            num_attention_heads=16 if large else 12, intermediate_size=4096 if large else 3072)
    else:
        raise EnvironmentError("--bert_model must be a local directory with bert_config.json (no network)")
    config.type_vocab_size = 6 if args.new_segment_ids else 2
    config.hidden_dropout_prob = config.attention_probs_dropout_prob = args.drop_prob
    if args.max_position_embeddings:
        config.max_position_embeddings = args.max_position_embeddings
    if args.num_hidden_layers:
        config.num_hidden_layers = args.num_hidden_layers
    if getattr(args, "label_smoothing", None):    # the from_pretrained kwarg of the reference (:328, 351): the masked-LM loss only, not VQA's
        config.label_smoothing = args.label_smoothing
    for key, default in (("relax_projection", 0), ("task_idx", None), ("fp32_embedding", False), ("label_smoothing", None)):
        if not hasattr(config, key):
            setattr(config, key, default)
    return config


def build_model(args, device):
    """run_img2txt_dist.py:310-377: construct (from scratch or from a checkpoint), .half(), .to(device)."""
    if args.relax_projection:
        raise NotImplementedError("--relax_projection is not supported by vlp_amd")
    if not args.fp16 and not args.allow_fp16_compute:
        raise NotImplementedError(
            "vlp_amd implements the reference's --fp16 path (fp16 storage, fp32 accumulate, FusedAdam in FP16_Optimizer_State) and has no fp32 compute "
            "path.  This command line has no --fp16%s.  Add --fp16 (the reference's fp16 recipe), or --allow_fp16_compute to keep the optimizer this "
            "command line selects (BertAdam, run_img2txt_dist.py:421-426) on fp32 master weights with fp16 compute."
            % (": the reference README's example commands pass --amp alone (README.md:112,131), and amp only engages together with --fp16 "
               "(run_img2txt_dist.py:305), so the reference itself runs them in fp32" if args.amp else ""))
    config = model_config(args)
    state = None
    if args.model_recover_path:
        state = torch.load(args.model_recover_path, map_location="cpu")
    elif not args.from_scratch:
        wpath = os.path.join(args.bert_model, "pytorch_model.bin") if os.path.isdir(args.bert_model) else None
        if not wpath or not os.path.exists(wpath):
            raise EnvironmentError("no pretrained weights available offline: pass --from_scratch or --model_recover_path")
        state = torch.load(wpath, map_location="cpu")
    if args.scst:
        # :355-361: the incremental decoder, built from the maximum-likelihood checkpoint; [MASK] / [SEP] as mask_word_id / eos_id (:319-320)
        model = BertForSeq2SeqDecoder(config, mask_word_id=synthetic.MASK_ID, num_labels=2, search_beam_size=1, eos_id=synthetic.SEP_ID,
                                      enable_butd=args.enable_butd, len_vis_input=args.len_vis_input)
    else:
        model = BertForPreTrainingLossMask(config, num_labels=2, enable_butd=args.enable_butd, len_vis_input=args.len_vis_input,
                                           tasks=args.tasks, allow_random_fc7=bool(args.synthetic))
    if state is not None:
        # the reference always goes through from_pretrained(state_dict=...) (:324-336): gamma/beta renames, segment table 2 -> 6
        # rows for --new_segment_ids, position-table tiling for --max_position_embeddings, and an ERROR on any other size mismatch
        load_checkpoint_state(model, state)
    model.half()
    model.to(device)
    return model


def build_optimizer(args, model, t_total):
    """run_img2txt_dist.py:393-426: two param groups by name, FusedAdam inside the fp16 wrapper."""
    named = list(model.named_parameters())
    no_decay = ["bias", "LayerNorm.bias", "LayerNorm.weight"]
    groups = [{"params": [p for n, p in named if not any(nd in n for nd in no_decay)], "weight_decay": 0.01},
              {"params": [p for n, p in named if any(nd in n for nd in no_decay)], "weight_decay": 0.0}]
    if not args.fp16:        # --allow_fp16_compute: the reference's else-branch (:421-426) on fp32 masters of the fp16 parameters
        from .optimization import BertAdam
        opt = BertAdam(groups, lr=args.learning_rate, warmup=args.warmup_proportion, schedule=args.sche_mode, t_total=t_total)
        opt.grad_scale = float(args.loss_scale) if args.loss_scale > 0 else 1024.0     # fp16 backward needs a scaled loss; step() divides it out
        return opt
    inner = FusedAdam(groups, lr=args.learning_rate, bias_correction=False, max_grad_norm=1.0)
    if args.loss_scale == 0:
        return FP16_Optimizer_State(inner, dynamic_loss_scale=True)
    return FP16_Optimizer_State(inner, static_loss_scale=args.loss_scale)


def train_step(model, optimizer, batch, lr_this_step, mask_image_regions=False, drop_worst_ratio=0.0, accumulate=False, accum_steps=1):
    """One iteration of the reference's inner loop (:479-585) on device-resident tensors.  Returns the (un-normalised) loss
    tuple (device tensors; nothing is read back).  With gradient accumulation the back-propagated loss is divided by
    `accum_steps` exactly as the reference does before `optimizer.backward` (:567-571)."""
    (input_ids, segment_ids, input_mask, lm_label_ids, masked_pos, masked_weights, is_next, task_idx, img, vis_masked_pos, vis_pe,
     ans_labels) = batch
    loss_tuple = model(img, vis_pe, input_ids, segment_ids, input_mask, lm_label_ids, ans_labels, is_next, masked_pos=masked_pos,
                       masked_weights=masked_weights, task_idx=task_idx, vis_masked_pos=vis_masked_pos,
                       mask_image_regions=mask_image_regions, drop_worst_ratio=drop_worst_ratio)
    masked_lm_loss, pretext_loss, ans_loss = loss_tuple
    # :531 `loss = masked_lm_loss + pretext_loss + ans_loss`; the engine's shared zero placeholder (a loss this task does not have) is
    # recognised by identity and not added: no add launches for `+ 0`
    eng = getattr(model.module if hasattr(model, "module") else model, "engine", None)
    terms = [t for t in loss_tuple if eng is None or not eng.is_zero_placeholder(t)]
    if not terms:
        raise RuntimeError("train_step: this batch has no live loss (no masked positions, no answer labels, no masked regions): nothing to back-propagate")
    loss = terms[0]
    for t in terms[1:]:
        loss = loss + t
    if accum_steps > 1:
        loss = loss / accum_steps                            # :567-568
    if hasattr(optimizer, "backward"):
        optimizer.backward(loss)                             # :571
    else:                                                    # :573 `loss.backward()` (BertAdam; --allow_fp16_compute scales the fp16 backward)
        gs = getattr(optimizer, "grad_scale", 1.0)
        loss.float().backward(gradient=torch.full_like(loss, gs, dtype=torch.float32) if gs != 1.0 else None)
    if not accumulate:
        if hasattr(optimizer, "backward"):
            for g in optimizer.param_groups:                 # :580-583 (fp16 only: BertAdam runs its own schedule)
                g["lr"] = lr_this_step
        optimizer.step()
        optimizer.zero_grad()
    return loss_tuple


def read_examples(token_file):
    """--token_file: the whole example list, (image id, [caption token ids]) or the 4-tuples of VQA."""
    with open(token_file) as f:
        return [tuple(e) if len(e) == 4 else (e[0], e[1]) for e in json.load(f)]


def scst_doc_freq(args):
    """--scst_df: None for 'batch'; the table counted over the WHOLE --token_file list for 'train' (not the rank's shard: every rank holds the
    same table); a saved table for a path, refused when it was built for another caption format than this run's."""
    from .data import examples_have_answers
    from .scst import DocFreq
    if args.scst_df == "batch":
        return None
    if args.scst_df == "train":
        examples = read_examples(args.token_file)
        if examples_have_answers(examples):
            raise ValueError("--scst_df train needs a caption --token_file, and %s holds VQA examples" % args.token_file)
        return DocFreq.from_examples(examples, args.max_len_b, synthetic.SEP_ID)
    table = DocFreq.load(args.scst_df)
    if (table.max_len_b, table.sep_id) != (args.max_len_b, synthetic.SEP_ID):
        raise ValueError("--scst_df %s was built for --max_len_b %s and [SEP] id %s; this run has --max_len_b %d and [SEP] id %d: rebuild it with "
                         "python -m vlp_amd.cider_df" % (args.scst_df, table.max_len_b, table.sep_id, args.max_len_b, synthetic.SEP_ID))
    return table


def scst_step(model, optimizer, batch, lr_this_step, len_vis_input, rl_crit, accumulate=False, accum_steps=1, mark=None, reward_on="host", df=None,
              samples=1, reward_weights=(1.0, 0.0), temperature=1.0, entropy_weight=0.0, stats=None):
    """One self-critical step (run_img2txt_dist.py:486-523, then :567-585): a greedy decode in eval() mode as the baseline, a sampled decode in
    train() mode whose log-probabilities are differentiable (BertForSeq2SeqDecoder, Engine.score_samples), the CIDEr-D reward of sample minus
    baseline (vlp_amd.scst, on the host) and RewardCriterion.  Returns (loss, mean reward) as device tensors.  mark(phase), if given, is
    called at the end of each phase: "greedy_decode", "sample_forward" (sampled decode + scoring forward), "reward_host", "backward" and,
    unless accumulating, "optimizer" (tools/scst_bench.py times them).
    reward_on="device" (--scst_reward device) computes the reward with vlp_amd.scst.self_critical_reward_device instead: nothing leaves the
    device between the sampled decode and the backward, and the phase is marked "reward_device".  A batch whose 12th element is a CaptionRefs
    (--scst_refs image) is scored against those references, on either side, instead of its own ground-truth ids.  df (--scst_df): a
    vlp_amd.scst.DocFreq whose document frequencies the reward uses, on either side, instead of the step's own references'; None = those.
    samples=K >= 2 (--scst_samples): K samples per image, each baselined by the mean score of the image's other K - 1
    (self_critical_reward_group / _group_device).  There is no greedy decode and no "greedy_decode" phase; the log-probabilities, the reward
    and RewardCriterion run over the K*B rows (row k*B + b is sample k of image b).
    reward_weights (--scst_cider_weight, --scst_bleu_weight): the score of a caption is cider_weight * CIDEr-D + bleu_weight * sentence BLEU-4,
    in whichever of the five reward functions the step calls; (1, 0) calls them as before.  The phase marks do not change.
    temperature (--scst_temperature) T != 1: the samples are drawn from softmax(logits / T) and the log-probabilities differentiated are that
    policy's; the greedy baseline is unaffected (an argmax does not depend on T).  entropy_weight (--scst_entropy_weight) W > 0: the loss is
    vlp_amd.scst.policy_loss, RewardCriterion - W x the masked mean entropy of the sampled policy; `stats`, if a dict, then receives that mean
    as stats["entropy"] (a device tensor).  (1, 0) is the step without them, call for call."""
    if mark is None:
        def mark(phase):
            pass
    from .scst import (clean_captions, self_critical_reward, self_critical_reward_device, self_critical_reward_refs, self_critical_reward_group,
                       self_critical_reward_group_device)
    (input_ids, segment_ids, input_mask, lm_label_ids, masked_pos, masked_weights, is_next, task_idx, img, vis_masked_pos, vis_pe,
     ans_labels) = batch
    L = input_ids.shape[1]
    if isinstance(input_mask, MaskSpec):
        input_mask = input_mask.dense(L)                  # the decoder reads the dense [B, L, L] mask
    position_ids = torch.arange(L, dtype=input_ids.dtype, device=input_ids.device).unsqueeze(0).expand_as(input_ids)
    input_dummy = input_ids[:, :len_vis_input + 2]        # +2 for [CLS] and [SEP]
    samples = int(samples)
    if samples < 1:
        raise ValueError("scst_step: samples must be >= 1 (got %d)" % samples)
    temperature, entropy_weight = float(temperature), float(entropy_weight)
    if not (0.0 < temperature < float("inf")) or not (0.0 <= entropy_weight < float("inf")):
        raise ValueError("scst_step: temperature must be finite and > 0, entropy_weight finite and >= 0 (got %r, %r)" % (temperature, entropy_weight))
    pkw = {}                                              # the policy keywords: none at (1, 0), the call as it always was
    if temperature != 1.0:
        pkw["temperature"] = temperature
    if entropy_weight > 0:
        pkw["return_entropy"] = True
    entropy = None
    if samples == 1:
        model.eval()
        with torch.no_grad():
            greedy_raw, _ = model(img, vis_pe, input_dummy, segment_ids, position_ids, input_mask, task_idx=task_idx, sample_mode="greedy")
        mark("greedy_decode")
        model.train()
        out = model(img, vis_pe, input_dummy, segment_ids, position_ids, input_mask, task_idx=task_idx, sample_mode="sample", **pkw)
    else:
        model.train()
        out = model(img, vis_pe, input_dummy, segment_ids, position_ids, input_mask, task_idx=task_idx, sample_mode="sample", n_samples=samples, **pkw)
    gen_raw, sample_logprobs = out[0], out[1]
    if entropy_weight > 0:
        entropy = out[2]
    mark("sample_forward")
    gen_result = clean_captions(gen_raw, synthetic.SEP_ID, synthetic.PAD_ID)
    gt_ids = input_ids[:, len_vis_input + 2:]
    kw = {} if df is None else {"df": df}
    if tuple(reward_weights) != (1.0, 0.0):
        kw.update(cider_weight=float(reward_weights[0]), bleu_weight=float(reward_weights[1]))
    if samples > 1:
        refs = ans_labels if isinstance(ans_labels, CaptionRefs) else gt_ids
        if reward_on == "device":
            reward, _ = self_critical_reward_group_device(gen_result, refs, samples, **kw)
        else:
            reward, _ = self_critical_reward_group(gen_result, refs, samples, **kw)
            reward = torch.from_numpy(reward).float().to(gen_result.device)
        mean_reward = reward.mean()
        mark("reward_device" if reward_on == "device" else "reward_host")
    elif reward_on == "device":
        greedy_res = clean_captions(greedy_raw, synthetic.SEP_ID, synthetic.PAD_ID)
        reward, _ = self_critical_reward_device(greedy_res, ans_labels if isinstance(ans_labels, CaptionRefs) else gt_ids, gen_result, **kw)
        mean_reward = reward.mean()
        mark("reward_device")
    else:
        greedy_res = clean_captions(greedy_raw, synthetic.SEP_ID, synthetic.PAD_ID)
        if isinstance(ans_labels, CaptionRefs):
            reward, _ = self_critical_reward_refs(greedy_res, ans_labels, gen_result, **kw)
        else:
            reward, _ = self_critical_reward(greedy_res, gt_ids, gen_result, gt_ids.size(0), **kw)
        reward = torch.from_numpy(reward).float().to(gen_result.device)
        mean_reward = reward.mean()
        mark("reward_host")
    if entropy is None:
        loss = rl_crit(sample_logprobs, gen_result, reward)
    else:
        from .scst import policy_loss
        loss, mean_h = policy_loss(sample_logprobs, gen_result, reward, entropy=entropy, entropy_weight=entropy_weight, crit=rl_crit)
        if isinstance(stats, dict):
            stats["entropy"] = mean_h
    bwd = loss / accum_steps if accum_steps > 1 else loss
    if hasattr(optimizer, "backward"):
        optimizer.backward(bwd)
    else:
        gs = getattr(optimizer, "grad_scale", 1.0)
        bwd.float().backward(gradient=torch.full_like(bwd, gs, dtype=torch.float32) if gs != 1.0 else None)
    mark("backward")
    if not accumulate:
        if hasattr(optimizer, "backward"):
            for g in optimizer.param_groups:
                g["lr"] = lr_this_step
        optimizer.step()
        optimizer.zero_grad()
        mark("optimizer")
    return loss, mean_reward


def build_packed_loader(args, device):
    """Img2txtDataset + Preprocess4Seq2seq (vlp/seq2seq_loader.py:62-359, run_img2txt_dist.py:248-300) on a packed region store:
    s2s / bidirectional preprocessors drawn per sample with --s2s_prob / --bi_prob.  With world_size > 1 the per-epoch order is
    DistributedSampler's (:295, 455): one global permutation per epoch (seeded by the epoch, the same on every rank), padded by
    wrapping around so that every rank gets ceil(N / W) samples, rank r taking every W-th element (vlp_amd.data.distributed_sampler_indices)."""
    from .data import BatchPrefetcher, PackedRegionStore, TextPreprocessor, examples_have_answers, VQA_EXAMPLE_FORMAT
    store = PackedRegionStore(args.packed_features)
    examples = read_examples(args.token_file)
    if args.tasks == "vqa2" and not examples_have_answers(examples):     # (a file that mixes the two forms raises in there)
        raise ValueError("--tasks vqa2 needs answers, and --token_file %s has none: %s" % (args.token_file, VQA_EXAMPLE_FORMAT))
    kw = dict(max_pred=args.max_pred, mask_prob=args.mask_prob, vocab_size=KNOWN_VOCABS.get(args.bert_model, 28996), cls_id=synthetic.CLS_ID,
              sep_id=synthetic.SEP_ID, mask_id=synthetic.MASK_ID, unk_id=synthetic.UNK_ID, max_len=args.max_seq_length, max_len_b=args.max_len_b,
              len_vis_input=args.len_vis_input, new_segment_ids=args.new_segment_ids, trunc_seg=args.trunc_seg,
              always_truncate_tail=args.always_truncate_tail)
    return BatchPrefetcher(store, examples, args.train_batch_size, TextPreprocessor(mode="s2s", **kw), TextPreprocessor(mode="bi", **kw),
                           s2s_prob=args.s2s_prob, device=device, seed=args.seed, vis_mask_prob=args.vis_mask_prob,
                           rank=max(args.global_rank, 0), world=max(args.world_size, 1), num_workers=args.num_workers,
                           balance_lengths=(args.shard_order == "balanced" and not args.no_padding_free),
                           caption_refs=5 if args.scst_refs == "image" else 0)


def synthetic_batches(args, device, steps, rank):
    """Device-resident synthetic batches (a small rotating pool, seeded per rank like a DistributedSampler shard).  The pool is built once per
    run and reused by every epoch: the same tensor objects come back, so the padding-free step derives their kept lengths once."""
    pool = getattr(args, "_synthetic_pool", None)
    if pool is not None:
        for s in range(steps):
            yield pool[s % len(pool)]
        return
    pool = args._synthetic_pool = []
    for i in range(min(4, steps)):
        b = synthetic.make_batch(args.train_batch_size, max_len_b=args.max_len_b, len_vis_input=args.len_vis_input,
                                 vocab_size=KNOWN_VOCABS.get(args.bert_model, 28996), max_pred=args.max_pred, mask_prob=args.mask_prob,
                                 s2s_prob=args.s2s_prob, tasks=args.tasks, seed=args.seed + 1000 * max(rank, 0) + i,
                                 new_segment_ids=args.new_segment_ids, vis_mask_prob=args.vis_mask_prob)
        pool.append(synthetic.batch_to(b, device, half=True))
    for s in range(steps):
        yield pool[s % len(pool)]


def main(argv=None):
    args = derive_args(build_parser().parse_args(argv))
    os.makedirs(args.output_dir, exist_ok=True)
    json.dump(args.__dict__, open(os.path.join(args.output_dir, "opt.json"), "w"), sort_keys=True, indent=2)
    logging.basicConfig(filename=os.path.join(args.output_dir, args.log_file), filemode="w",
                        format="%(asctime)s - %(levelname)s - %(name)s -   %(message)s", datefmt="%m/%d/%Y %H:%M:%S", level=logging.INFO,
                        force=True)      # (a second main() in one process logs to ITS output_dir, not to the first one's file)
    logger = logging.getLogger(__name__)
    if args.no_cuda or not torch.cuda.is_available():
        raise RuntimeError("vlp_amd has no CPU path: an MI355X is required (the reference's --no_cuda mode is not provided)")
    distributed = args.local_rank != -1
    if distributed:
        torch.cuda.set_device(args.local_rank)
        device = torch.device("cuda", args.local_rank)
        torch.distributed.init_process_group(backend="nccl", init_method=args.dist_url, world_size=args.world_size, rank=args.global_rank)
    else:
        device = torch.device("cuda")
    random.seed(args.seed)
    np.random.seed(args.seed)
    torch.manual_seed(args.seed)
    torch.cuda.manual_seed_all(args.seed)

    loader = None
    if args.packed_features:
        loader = build_packed_loader(args, device)
        steps_per_epoch = loader.steps
    elif args.synthetic:
        steps_per_epoch = args.synthetic
    else:
        raise NotImplementedError("give --packed_features DIR --token_file FILE (vlp_amd.data; the reference's h5 files are converted once "
                                  "with vlp_amd.data.pack_from_h5) or --synthetic STEPS_PER_EPOCH; the tokenizer itself is out of scope")
    t_total = int(steps_per_epoch * args.num_train_epochs * 1. / args.gradient_accumulation_steps)

    recover_step = _get_max_epoch_model(args.output_dir)     # :310: resume from the newest epoch that has model AND optimizer files
    check_scst_start(args, recover_step)
    if recover_step:
        logger.info("***** Recover model: %d *****", recover_step)
        args.model_recover_path = os.path.join(args.output_dir, "model.{0}.bin".format(recover_step))
    rl_crit, scst_df = None, None
    if args.scst:
        from .scst import RewardCriterion
        rl_crit = RewardCriterion()
        scst_df = scst_doc_freq(args)
        if scst_df is not None:
            logger.info("--scst_df %s: %d n-grams over %d images", args.scst_df, len(scst_df), scst_df.n_docs)
        if args.drop_prob > 0:
            logger.info("--scst: --drop_prob %g is inert: the sampled decode and the scoring pass both run without dropout (INTEGRATION.md)",
                        args.drop_prob)
    model = build_model(args, device)
    if distributed:
        model = DDP(model, device_ids=[args.local_rank], output_device=args.local_rank, find_unused_parameters=True)
    optimizer = build_optimizer(args, model, t_total)
    eng = (model.module if hasattr(model, "module") else model).engine
    if args.no_padding_free:
        eng.varlen = False
    elif eng.varlen == "auto":
        # padding-free by default: the packed loader's MaskSpec carries the lengths on the host; a --synthetic pool of dense
        # masks is reduced + read back once per pooled tensor (budget), then remembered; anything else runs dense and says so once
        eng.varlen_readback_budget = 8
    logger.info("padding-free step: %s", eng.varlen)
    if hasattr(optimizer, "pipeline_with_forward"):
        # this loop touches parameters only through the engine, so the optimizer step MAY stream underneath the next forward
        # (VLP_ADAM_PIPELINE=1; bit-identical).  On one MI355X it is a wash (the HBM-bound update slows the concurrent GEMMs), so off.
        optimizer.pipeline_with_forward = os.environ.get("VLP_ADAM_PIPELINE", "0") == "1"
    global_step = 0
    if recover_step:                                         # :428-437
        logger.info("***** Recover optimizer: %d *****", recover_step)
        optimizer.load_state_dict(torch.load(os.path.join(args.output_dir, "optim.{0}.bin".format(recover_step)), map_location=device))
        if args.loss_scale == 0:
            optimizer.dynamic_loss_scale = True
        global_step = math.floor(recover_step * t_total * 1. / args.num_train_epochs)      # :337-338
    logger.info("***** Running training *****  batch %d, steps %d", args.train_batch_size, t_total)
    scst_policy = {}                     # scst_step's policy keywords: none at the defaults
    if args.scst and args.scst_temperature != 1.0:
        scst_policy["temperature"] = args.scst_temperature
    if args.scst and args.scst_entropy_weight > 0:
        scst_policy.update(entropy_weight=args.scst_entropy_weight, stats={})
    model.train()
    stop_after = args.stop_after_epoch if args.stop_after_epoch > 0 else args.num_train_epochs
    for i_epoch in range((recover_step or 0) + 1, min(args.num_train_epochs, stop_after) + 1):
        t0 = time.time()
        losses, rewards, entropies = [], [], []
        if loader is not None:
            loader.set_epoch(i_epoch - 1)                                                             # train_sampler.set_epoch(i_epoch-1), :455
        for step, batch in enumerate(loader if loader is not None else synthetic_batches(args, device, steps_per_epoch, args.global_rank)):
            acc = (step + 1) % args.gradient_accumulation_steps != 0
            lr = args.learning_rate * warmup_linear(global_step / t_total, args.warmup_proportion)
            if args.scst:
                loss, mean_r = scst_step(model, optimizer, batch, lr, args.len_vis_input, rl_crit, accumulate=acc,
                                         accum_steps=args.gradient_accumulation_steps, reward_on=args.scst_reward, df=scst_df,
                                         samples=args.scst_samples, reward_weights=(args.scst_cider_weight, args.scst_bleu_weight),
                                         **scst_policy)
                rewards.append(mean_r.detach())
                if "stats" in scst_policy:
                    entropies.append(scst_policy["stats"]["entropy"])
            else:
                lt = train_step(model, optimizer, batch, lr, mask_image_regions=args.mask_image_regions,
                                drop_worst_ratio=args.max_drop_worst_ratio if i_epoch > args.drop_after else 0,
                                accumulate=acc, accum_steps=args.gradient_accumulation_steps)
            if not acc:
                global_step += 1
            if step % args.log_every == 0:        # the only host read-back; the reference does 4 per step (:535-538)
                if args.scst:                     # :540 adds the mean reward
                    losses.append(float(loss.detach()))
                    if entropies:
                        logger.info("Epoch %d, Iter %d, Loss %.3f, Mean R %.3f, Mean H %.3f", i_epoch, step, losses[-1],
                                    float(torch.stack(rewards).mean()), float(torch.stack(entropies).mean()))
                    else:
                        logger.info("Epoch %d, Iter %d, Loss %.3f, Mean R %.3f", i_epoch, step, losses[-1], float(torch.stack(rewards).mean()))
                else:
                    losses.append(float((lt[0] + lt[1] + lt[2]).detach()))
                    logger.info("Epoch %d, Iter %d, Loss %.3f", i_epoch, step, losses[-1])
        torch.cuda.synchronize()
        dt = time.time() - t0
        if hasattr(optimizer, "consolidate"):
            optimizer.consolidate()        # collective under VLP_DDP_MODE=sharded (every rank; rank 0 alone writes the file below)
        if args.global_rank in (-1, 0):
            print("epoch %d: %d steps, %.1f samples/s/rank, loss %s" % (i_epoch, steps_per_epoch, steps_per_epoch * args.train_batch_size / dt,
                                                                        ["%.3f" % l for l in losses[-3:]]))
            to_save = model.module if hasattr(model, "module") else model
            torch.save(copy.deepcopy(to_save).cpu().state_dict(), os.path.join(args.output_dir, "model.{0}.bin".format(i_epoch)))
            # the reference disabled this line ("need to sanitize state and ship everything back to cpu", :599); here the optimizer
            # state is three flat fp32 buffers per group + a few scalars, shipped to the host as they are
            osd = optimizer.apex_state_dict() if (args.optim_format == "apex" and hasattr(optimizer, "apex_state_dict")) else optimizer.state_dict()
            torch.save(_to_cpu(osd), os.path.join(args.output_dir, "optim.{0}.bin".format(i_epoch)))
        if args.world_size > 1:
            torch.distributed.barrier()
    if distributed:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
