"""Fused forward/backward executor of the VLP unified transformer on MI355X.

This is the host-side orchestration that replaces the reference's per-op autograd graph
(pytorch_pretrained_bert/modeling.py:217-482, 1033-1143): one Python call sequence over the C ABI of
libvlp_hip.so per training step, with

  * parameters living in two flat fp16 buffers (weight-decay group / no-decay group -- the same two
    groups the train script builds, run_img2txt_dist.py:394-401), laid out in *backward completion
    order* so that a gradient bucket is a contiguous slice that can be handed to RCCL the moment the
    last weight-gradient GEMM of that slice has been launched;
  * gradients written by the kernels straight into matching flat fp16 buffers (`param.grad` are views);
  * activations kept in a per-shape workspace that is reused every step (3.4 GB at B = 64, L = 167 -- small against the
    chip's 288 GB, so nothing is recomputed except dropout masks, which are a pure function of (seed, stream, index));
  * transposed weight shadows for the dgrad GEMMs refreshed once per backward.

PyTorch is used for memory (torch.empty), streams and the autograd hand-off only.  There is no
fallback: every compute step is a HIP kernel.
"""
import math
import os
import weakref

import numpy as np
import torch

from . import _lib as K
from . import tuning
from ._common import PE_DIM, PE_PAD, VlpPerformanceWarning, _ru
from .decoder import Decoder, sample_major        # noqa: F401 (sample_major: callers import it from here)
from .input_prep import MaskSpec, RawRegions, SparseAnswers

ALIGN = 64            # elements; every parameter starts on a 128-byte boundary inside its flat buffer
NO_DECAY = ("bias", "LayerNorm.bias", "LayerNorm.weight")    # run_img2txt_dist.py:395


def is_no_decay(name):
    return any(nd in name for nd in NO_DECAY)


def layer_param_names(i):
    """{field of the layer handle table: the names of encoder layer i's parameters behind it}.  The one place that writes a layer's
    parameter names down (besides _ordered_names, whose job is their order in the flat buffers); q / k / v lie back to back there and
    are one packed [3H, H] weight and one [3H] bias to every kernel."""
    L = "bert.encoder.layer.%d." % i
    qkv = [L + "attention.self." + n for n in ("query", "key", "value")]
    one = {"o": "attention.output.dense", "ln1": "attention.output.LayerNorm", "fc1": "intermediate.dense", "fc2": "output.dense",
           "ln2": "output.LayerNorm"}
    names = {"qkv_w": tuple(n + ".weight" for n in qkv), "qkv_b": tuple(n + ".bias" for n in qkv)}
    for f, n in one.items():
        names[f + "_w"], names[f + "_b"] = (L + n + ".weight",), (L + n + ".bias",)
    return names


class _LayerViews(object):
    """One encoder layer's twelve views of a flat buffer (Engine._layers): weight `*_w` and bias `*_b` of the packed QKV projection, the
    attention-output dense (o), LayerNorm 1 (gamma = ln1_w, beta = ln1_b), the intermediate (fc1) and output (fc2) dense and LayerNorm 2."""
    __slots__ = tuple(layer_param_names(0))


class _State(object):
    """What one forward leaves behind for its backward."""
    __slots__ = ("gen", "B", "L", "P", "seed", "p_drop", "ws", "batch", "has_mlm", "task_labels", "pretext", "pk", "mlm_smooth", "pos_ids", "policy", "kept")

    def __init__(self):
        self.gen = self.B = self.L = self.P = 0      # engine generation, batch, sequence length, masked positions per sample
        self.ws = None               # the (B, L, P) workspace holding the activations
        self.seed, self.p_drop = 0, (0.0, 0.0)       # dropout: seed of the step, (hidden, attention) probabilities
        self.batch = None            # (img, input_ids, token_type_ids, masked_pos) as the kernels read them
        self.has_mlm = False         # P > 0: the masked-LM head ran
        self.pos_ids = None          # explicit position ids ([B, L] int64) or None = 0..L-1
        self.pk = None               # (row_off, row_map, M') of a packed forward
        self.kept = None             # (map, count) on the device: the kept rows of a dense training forward (the mapped grouped wgrad walks them)
        self.pretext = None          # (pretext workspace, vis_masked_pos) of a mask_image_regions forward
        self.task_labels = None      # set by the loss of this forward (mlm_loss / vqa_loss / score_samples), read by its backward
        self.mlm_smooth = None       # label-smoothed loss: the scalar arguments of the matching backward launch
        self.policy = None           # score_samples with a temperature / entropy: (temperature, entropy rows or None) of vlp_token_policy_fwd


class _Backward(object):
    """What the phases of one Engine.backward share: the forward's state and shapes, the streams, and the listed-row state."""
    __slots__ = ("eng", "st", "ws", "sh", "beta", "NL", "H", "I", "A", "V", "Nv", "M", "Mv", "ro", "rm", "p", "pa", "seed", "scale", "grouped",
                 "kept", "main", "side", "use_side", "live", "R", "live_ready")

    def __init__(self, eng, st, task):
        model = eng._model()
        cfg = model.config
        self.eng, self.st, self.ws, self.sh, self.NL = eng, st, st.ws, None, cfg.num_hidden_layers       # sh: the W^T shadows (prologue)
        self.H, self.I, self.A, self.V, self.Nv = cfg.hidden_size, cfg.intermediate_size, cfg.num_attention_heads, cfg.vocab_size, model.len_vis_input
        # (packed rows: every [M, *] activation of the step has M' = sum of the kept lengths rows)
        self.ro, self.rm, self.M = st.pk if st.pk is not None else (None, None, st.B * st.L)
        self.Mv, self.beta = st.B * self.Nv, 1 if eng.grads_dirty else 0
        (self.p, self.pa), self.seed, self.scale = st.p_drop, st.seed, 1.0 / math.sqrt(self.H // self.A)
        # one vlp_gemm_tn_grouped launch per layer instead of 4 split-M wgrads + 4 reduces where there are enough rows for a long contraction
        # per workgroup; tiny batches keep split-M
        self.grouped = self.M >= 2048
        # the forward's map of kept rows (dense training steps only; never a score_samples forward); VLP_WGRAD_KEPT=0 read per call
        self.kept = st.kept if (self.grouped and st.pk is None and task != "logprob" and os.environ.get("VLP_WGRAD_KEPT", "1") != "0") else None
        self.main, self.use_side = torch.cuda.current_stream(), eng.WGRAD_SIDE_STREAM
        self.side = eng._side_stream() if self.use_side else None
        self.live = self.R = self.live_ready = None      # the last layer's row list, its capacity, the event behind its prologue

    def on_side(self, fn):
        """Run fn() on the side stream, ordered behind everything the main stream has issued so far (without one: here and now)."""
        if not self.use_side:
            fn()
            return
        self.side.wait_stream(self.main)
        with torch.cuda.stream(self.side):
            fn()

    def ln_slot(self, k):
        """The private dgamma / dbeta partials of LayerNorm k (the order of Engine._ln_table)."""
        n = self.ws["ln_slot_bytes"]
        return self.ws["ln_slots"][k * n:(k + 1) * n]

    def wgrads_issued(self, i):
        """Layer i's weight gradients are issued: its gradient slice is complete in this stream's order, and the event behind them guards
        the dY set they read."""
        self.eng._bucket_done(self.NL - i)
        if self.use_side:
            ev = torch.cuda.Event()
            ev.record(self.side)
            self.eng._side_done[i & 1] = ev


class Engine(Decoder):
    """Parameters, workspaces and the training step; the caption decoders (decode_greedy / decode_sample_group / decode_beam, their
    workspaces and switches) are the base class, vlp_amd/decoder.py."""
    GEMM_NT_VARIANT = None   # None -> vlp_amd.tuning (committed table, else shape heuristic; timing search only with VLP_AUTOTUNE=1); or force an int
    NT_CANDIDATES = (1, 2, 4, 5, 9, 10, 11, 12, 13, 27, 29, 73, 77, 264)   # product variants (+8 = XCD-aware tile order, +16 = ring, 64 + cfg = wave-pipelined, 256 = persistent k stream); see include/vlp_hip.h
    NT_CANDIDATES_SKINNY = (1, 2, 9, 10, 11, 17)      # M <= 1024 (decoding, LM head): few workgroups, latency-bound -> also the 4-stage ring
    GEMM_TN_VARIANT = 2      # ds_read_b64_tr_b16 fragment reads + LDS-DMA staging
    # weight-gradient GEMMs of the encoder layers on a second HIP stream, concurrent with the dgrad chain (the wgrad grids are a single
    # round of 430-580 workgroups whose tails leave CUs idle; so do LN / attention backward): +2.6 % step throughput on one MI355X.
    # Results are bit-identical with and without (tests/test_10_model_gpu.py).  VLP_WGRAD_SIDE_STREAM=0 turns it off (clean
    # single-kernel timings under rocprofv3).  bench.py's live roofline samples stay single-kernel measurements: a sampled launch
    # first lets the side stream drain (see _nt).
    WGRAD_SIDE_STREAM = os.environ.get("VLP_WGRAD_SIDE_STREAM", "1") == "1"
    # mask_image_regions: the reference's loader line `input_mask[:, vis_masked_pos].fill_(0)` (seq2seq_loader.py:303-304) indexes with a
    # numpy array -- advanced indexing, i.e. it fills a COPY and leaves the mask untouched (checked on torch 2.10 and, against the unmodified
    # loader, by the reference-pinning CPU tests): masked regions enter the encoder as zeros but stay attendable.
    # Parity follows that behaviour; VLP_BLOCK_MASKED_REGIONS=1 follows the line's comment instead ("block the masked visual feature")
    # on the MaskSpec path (a dense attention_mask is always used as given).
    BLOCK_MASKED_REGION_KEYS = os.environ.get("VLP_BLOCK_MASKED_REGIONS", "0") == "1"
    # Padding-free (packed) step, opt-in (VLP_VARLEN=1 or engine.varlen = True; training / grad-enabled forwards only).  A sample's
    # positions past its last token are INERT in the reference's computation: no kept query attends them (their mask columns are 0 for
    # every row: seq2seq_loader.py:295-304), no loss reads them (masked_pos, h[:, 0], h[:, Nv+1] lie before them), so their hidden states
    # feed nothing and every gradient contribution through them is exactly zero (dO = 0 for pad queries, P = 0 for pad keys:
    # modeling.py:289-298).  The packed step keeps the first n_b positions of sample b (n_b derived from the mask itself, _packing())
    # as rows [row_off[b], row_off[b+1]) of every [M, *] activation and runs every row-wise kernel on M' = sum n_b rows; attention takes
    # row_off; dropout hashes keep the logical (b*L + l, col) element, so masks -- and with them losses, logits and gradients --
    # equal the dense run's up to the fp32 summation order of the weight-gradient / LayerNorm-parameter sums.
    # Round 6: ON BY DEFAULT where it costs nothing -- VLP_VARLEN unset = "auto": a batch whose kept lengths are known on the host (MaskSpec.lens_host:
    # the loader's form) or remembered for this very mask tensor (a device-resident pool) runs packed; a FRESH dense int64 mask would need a
    # device -> host read-back before the forward can be enqueued (a pipeline bubble per step), so in auto mode it runs dense after
    # `varlen_readback_budget` read-backs (0 here; the entry script allows 8 so that a --synthetic pool warms up) and a one-time
    # VlpPerformanceWarning says so.  VLP_VARLEN=1 / engine.varlen = True: always packed, read-backs accepted (warned about once);
    # VLP_VARLEN=0 / False: never.
    VARLEN = {"1": True, "0": False}.get(os.environ.get("VLP_VARLEN", ""), "auto")
    # (Round 5, measured and NOT kept -- the gradient norm in front of the optimizer step stays one vlp_sumsq pass over the buffer, 53 us:
    # one partial-sum launch per finished gradient slice on the side stream during backward LOSES, 9.738 / 9.722 vs 9.666 / 9.671 ms/step;
    # summing the 93 % of the buffer that is final when the side stream reaches the embedding tables, under the region-projection backward,
    # is a wash, 9.568 / 9.548 vs 9.558 / 9.573 -- profiles/r05_instep_ab_norm_per_slice.txt.  Both forms were removed.)
    TN_SPLITS = None         # None -> vlp_amd.tuning (variant flags, split-M factor) per (M, N, K); candidates: tuning.TN_SPLIT_CANDIDATES
    TN_VARIANT_CANDIDATES = (2, 26)     # 26 = LDS-DMA kernel + XCD-aware tile order + split-major block order
    # bench.py's live roofline: an event pair around a launch costs ~2 x 2.5 us of serialisation (5-6 % of the step when all 103
    # NT launches of a step are bracketed), so every 8th launch is sampled; 103 is coprime to 8, so successive steps sample
    # different launch positions and K >= 8 steps cover every launch of the step.
    PROF_EVERY = 8
    _nt_choice = {}          # shared across engines of one process: (M, N, K) -> variant
    _tn_choice = {}          # (M, N, K) -> splits
    _skinny_choice = {}      # (M, N, K) -> ("v", variant) | ("s", splits)

    def __init__(self, model):
        self._model = weakref.ref(model)
        self.packed = False
        self.gen = 0
        self.step_seed = 0
        self._warned_group_unfused = False        # decode_sample_group beyond 512 sequences: said once
        self.base_seed = 0x5EED
        self.grads_dirty = False          # False -> next backward overwrites (beta = 0), True -> accumulates
        self.grad_ready_hook = None       # callable(bucket_index) set by the DDP wrapper
        self.post_backward_hook = None    # callable() set by the DDP wrapper
        self.names = self.offsets = self.sizes = self.buckets = None      # plan_layout() of the packed model (pack)
        self.flat = self.gflat = None     # {"decay" | "nodecay": flat fp16 parameter / gradient buffer} (pack)
        self._params = None               # name -> parameter (pack)
        self._unused = None               # names of the parameters the task never gives a gradient (pack)
        self._anchor = None               # autograd anchor of the hand-off in modeling.py (pack)
        self.device = None
        self._ws = {}
        self._shadow = None
        self._shadow_ev = None            # event behind the W^T shadows a training forward transposed on the side stream, consumed by its backward
        self._ln_tab = None               # _ln_table()
        self._layer_tab = None            # _layers()
        self._zero1 = None                # zero_placeholder()
        self._pretext_on = False          # the latest forward ran with mask_image_regions
        self._pooler_dirty = False        # the pooler gradient buffer holds something a beta == 0 backward without the pretext branch must clear
        self.prof = None                  # list -> every PROF_EVERY-th NT-GEMM launch is bracketed by HIP events (bench.py roofline)
        self._opt_stream = None           # optimizer stream of the pipelined FusedAdam step (optimization_fp16._step_pipelined)
        self._param_events = None         # {"nodecay" | bucket index: event} of the last pipelined optimizer step, consumed by forward
        self._params_done = None          # event behind its last chunk
        self.shard_plan = None            # vlp_amd.distributed.ShardPlan when the optimizer step is sharded over the ranks (VLP_DDP_MODE=sharded)
        self._param_works = None          # {"nodecay" | reducer bucket: collective work} of the last sharded step's parameter all-gather
        self.param_gather_stamps = None   # list -> (before, after) event pairs around every wait for a parameter all-gather (comm profile)
        self._side = None                 # second HIP stream for the layer wgrads (_side_stream: created on first use)
        self._side_done = None            # with it: per dY-set parity, the event behind the last layer wgrads that read the set
        self._side_busy = False           # True while backward may have work queued on it
        self._prof_ctr = 0
        self.varlen = self.VARLEN         # padding-free (packed) training step: True | False | "auto", see VARLEN
        self.varlen_readback_budget = 0   # auto mode: how many fresh dense masks may still be reduced + read back (pool warm-up)
        self._rb_streak = 0               # consecutive read-backs without a cache hit in between
        self._rb_warned = False
        self._pk_stage = None             # ring of pinned row_off staging buffers (+ events) for _packing
        self._pk_stage_i = 0              # next slot of that ring
        self._pk_cache = {}               # kept-length tuple -> (row_off, row_map device tensors, M'): batches repeat in bench / epochs
        self._pk_lens = {}                # id(mask tensor) -> (weakref, version, ..., lens): lengths derived from a dense mask, once per tensor
        self.last_packed_rows = None      # M' of the latest packed forward (None: dense) -- bench.py / tests read it
        self.last_wgrad_mapped = False    # the latest backward's layer wgrads walked the map of kept rows (dense step, VLP_WGRAD_KEPT) -- tests read it
        self._live_n = None               # device int32 [1]: rows the latest backward's listed-row path walked (None: the full path ran)

    # ------------------------------------------------------------------------------------------
    # parameter packing
    # ------------------------------------------------------------------------------------------
    def _ordered_names(self, model):
        cfg = model.config
        tasks = model.tasks
        names = {n for n, _ in model.named_parameters()}
        decay, buckets = [], []

        def add(group):
            start = len(decay)
            decay.extend(group)
            buckets.append((start, len(decay)))

        head_unused = []
        if tasks == "vqa2":
            add(["ans_classifier.2.weight", "ans_classifier.0.weight"])
            head_unused.append("cls.predictions.transform.dense.weight")
        else:
            add(["cls.predictions.transform.dense.weight"])
        for i in reversed(range(cfg.num_hidden_layers)):
            L = "bert.encoder.layer.%d." % i
            add([L + "output.dense.weight", L + "intermediate.dense.weight", L + "attention.output.dense.weight",
                 L + "attention.self.query.weight", L + "attention.self.key.weight", L + "attention.self.value.weight"])
        # two slices: the embedding tables are final after embed_bwd (45 MB: the tied word embedding), the region projections only after
        # the three wgrads that follow -- the big slice's all-reduce overlaps them instead of waiting for the end of backward
        add(["bert.embeddings.position_embeddings.weight", "bert.embeddings.token_type_embeddings.weight",
             "bert.embeddings.word_embeddings.weight"])
        add(["vis_pe_embed.0.weight", "vis_embed.2.weight", "vis_embed.0.weight", "bert.pooler.dense.weight"] + head_unused)
        nodecay = sorted(n for n in names if is_no_decay(n))
        # q/k/v biases of a layer must be contiguous (packed QKV GEMM)
        for i in range(cfg.num_hidden_layers):
            L = "bert.encoder.layer.%d.attention.self." % i
            for n in (L + "query.bias", L + "key.bias", L + "value.bias"):
                nodecay.remove(n)
            nodecay.extend([L + "query.bias", L + "key.bias", L + "value.bias"])
        missing = names - set(decay) - set(nodecay)
        extra = (set(decay) | set(nodecay)) - names
        if missing or extra:
            raise RuntimeError("vlp_amd.Engine: unexpected parameter set (missing %s, unknown %s)" % (sorted(missing), sorted(extra)))
        return decay, nodecay, buckets

    def plan_layout(self, model=None):
        """Pure function of the parameter shapes (runs on CPU, no device needed): names per flat buffer, element offsets (every
        parameter on a 128-byte boundary), buffer sizes, and the gradient buckets = contiguous slices of the decay buffer in
        backward-completion order (head, layer N-1 .. 0, embedding tables, region projections)."""
        model = model if model is not None else self._model()
        numel = {n: p.numel() for n, p in model.named_parameters()}
        decay, nodecay, bucket_idx = self._ordered_names(model)
        names = {"decay": decay, "nodecay": nodecay}
        offsets, sizes = {}, {}
        for grp, ns in names.items():
            off, offs = 0, {}
            for n in ns:
                offs[n] = off
                off += _ru(numel[n], ALIGN)
            offsets[grp], sizes[grp] = offs, _ru(off, 8)
        buckets = []
        for s_, e_ in bucket_idx:
            lo = offsets["decay"][decay[s_]]
            hi = offsets["decay"][decay[e_ - 1]] + _ru(numel[decay[e_ - 1]], ALIGN)
            buckets.append((lo, min(hi, sizes["decay"])))
        return {"names": names, "offsets": offsets, "sizes": sizes, "buckets": buckets}

    def pack(self):
        """Move every parameter into the flat buffers (idempotent).  Needs fp16 parameters on a GPU:
        this is the `model.half(); model.to(device)` state of run_img2txt_dist.py:370-377."""
        if self.packed:
            return
        model = self._model()
        params = dict(model.named_parameters())
        dev = next(iter(params.values())).device
        if dev.type != "cuda":
            raise RuntimeError("vlp_amd: the model must be on an MI355X (`model.to('cuda')`); there is no CPU path")
        for n, p in params.items():
            if p.dtype != torch.float16:
                raise RuntimeError("vlp_amd: parameters must be fp16 (`model.half()`, i.e. --fp16): %s is %s. "
                                   "The fp32 path of the reference is not implemented (DESIGN.md, out of scope)." % (n, p.dtype))
        K.load()
        lay = self.plan_layout(model)
        self.names, self.offsets, self.sizes, self.buckets = lay["names"], lay["offsets"], lay["sizes"], lay["buckets"]
        self.flat, self.gflat = {}, {}
        for grp, names in self.names.items():
            offs, total = self.offsets[grp], self.sizes[grp]
            flat = torch.zeros(total, device=dev, dtype=torch.float16)
            gflat = torch.zeros(total, device=dev, dtype=torch.float16)
            for n in names:
                p = params[n]
                view = flat[offs[n]:offs[n] + p.numel()].view(p.shape)
                view.copy_(p.data)
                p.data = view
                p.grad = gflat[offs[n]:offs[n] + p.numel()].view(p.shape)
                p._vlp_engine = self
            self.flat[grp], self.gflat[grp] = flat, gflat
        self._params = params
        self.device = dev
        self.packed = True
        self.grads_dirty = False
        self._anchor = torch.zeros(1, device=dev, requires_grad=True)
        self._unused = set(["bert.pooler.dense.weight", "bert.pooler.dense.bias"])
        if model.tasks == "vqa2":
            self._unused |= {"cls.predictions.bias", "cls.predictions.transform.dense.weight", "cls.predictions.transform.dense.bias",
                             "cls.predictions.transform.LayerNorm.weight", "cls.predictions.transform.LayerNorm.bias"}

    def invalidate(self):
        """Called when nn.Module._apply() replaced parameter storage (.half()/.to()/.cpu())."""
        self.packed = False
        self._ws = {}
        self._shadow = None
        self._shadow_ev = None
        self._ln_tab = None
        self._layer_tab = None

    def P(self, name):
        return self._params[name].data

    def G(self, name):
        return self._params[name].grad

    def _layers(self):
        """The layer handle table: [(parameter views, gradient views)] per encoder layer, slices of the flat buffers under the fields of
        layer_param_names (pack() binds every .data / .grad to the same storage once; built on first use, dropped by invalidate())."""
        if self._layer_tab is None:
            tab = []
            for i in range(self._model().config.num_hidden_layers):
                w, g = _LayerViews(), _LayerViews()
                for f, ns in layer_param_names(i).items():
                    grp = "nodecay" if is_no_decay(ns[0]) else "decay"
                    off, shape = self.offsets[grp], self._params[ns[0]].shape
                    if any(off[b] - off[a] != shape.numel() for a, b in zip(ns, ns[1:])):
                        raise RuntimeError("vlp_amd.Engine: %s do not lie back to back in the flat buffer" % (ns,))
                    lo, hi, packed = off[ns[0]], off[ns[0]] + len(ns) * shape.numel(), (len(ns) * shape[0],) + tuple(shape[1:])
                    setattr(w, f, self.flat[grp][lo:hi].view(packed))
                    setattr(g, f, self.gflat[grp][lo:hi].view(packed))
                tab.append((w, g))
            self._layer_tab = tab
        return self._layer_tab

    def unused_parameter_names(self):
        """Parameters that receive no gradient (static per task).  The pooler is used by the vis_pretext branch only:
        it leaves the set while the latest forward ran with mask_image_regions."""
        if self._pretext_on:
            return set(self._unused) - {"bert.pooler.dense.weight", "bert.pooler.dense.bias"}
        return set(self._unused)

    # ------------------------------------------------------------------------------------------
    # pipelined optimizer step: parameter chunks become valid one by one (events on the optimizer stream)
    # ------------------------------------------------------------------------------------------
    def optimizer_stream(self):
        if self._opt_stream is None:
            self._opt_stream = torch.cuda.Stream(device=self.device)
        return self._opt_stream

    def set_param_events(self, events, done):
        self._param_events, self._params_done = events, done

    def wait_params(self, key=None, host=False, consume=True):
        """Make the current stream (host=True: the calling thread) wait until the optimizer stream has written parameter chunk `key`
        ("nodecay" or a bucket index); key=None: all of them (also orders the optimizer's reads of the gradient buffers before later work)."""
        if self._param_works is not None:          # sharded step: parameter chunks arrive by all-gather, one collective per bucket
            works = self._param_works
            prof = self.param_gather_stamps            # bench.py comm profile: how long the forward stood still for its parameters
            if prof is not None:
                e0 = torch.cuda.Event(enable_timing=True)
                e0.record()
            if key is None:
                for w in works.values():
                    if w is not None:
                        w.wait()                   # (RCCL: the current stream waits; no host sync)
                self._param_works = None
            else:
                k = key if key == "nodecay" else self.shard_plan.bucket_of_slice[key]
                w = works.get(k)
                if w is not None:
                    w.wait()
                    if consume:                    # (consume=False: a wait on ANOTHER stream -- the main stream still has to wait for this bucket itself)
                        works[k] = None
            if prof is not None:
                e1 = torch.cuda.Event(enable_timing=True)
                e1.record()
                prof.append((e0, e1))
        if self._params_done is None:
            return
        if key is not None:          # one chunk: the current stream waits for that chunk's event (no event: nothing was written to it)
            ev = self._param_events.get(key) if self._param_events else None
            if ev is not None:
                torch.cuda.current_stream().wait_event(ev)
        elif host:                   # everything, on the calling thread: the step is over and its events are spent
            self._params_done.synchronize()
            self._param_events, self._params_done = None, None
        else:                        # everything, on the current stream: the events stay for the other streams' waits
            torch.cuda.current_stream().wait_event(self._params_done)

    def zero_placeholder(self, device):
        """The shared read-only [1] fp32 zero that stands for a loss the task does not have (modeling.py:1096-1098, 1133)."""
        z = self._zero1
        if z is None or z.device != device:
            z = self._zero1 = torch.zeros(1, device=device, dtype=torch.float32)
        return z

    def is_zero_placeholder(self, t):
        """True when `t` is the shared zero a forward hands out for a loss the task does not have (train loops skip it instead of
        launching `+ 0`).  The placeholder is shared by every forward of this engine: do not modify it in place."""
        return t is self._zero1

    def zero_grad(self):
        """optimizer.zero_grad() of the train loop (run_img2txt_dist.py:585): no memset -- the next
        backward simply overwrites (beta = 0) instead of accumulating."""
        self.grads_dirty = False

    # ------------------------------------------------------------------------------------------
    # workspaces
    # ------------------------------------------------------------------------------------------
    def _workspace(self, B, L, P):
        key = (B, L, P)
        ws = self._ws.get(key)
        if ws is not None:
            return ws
        model = self._model()
        cfg = model.config
        H, I, A, NL, Nv, V = cfg.hidden_size, cfg.intermediate_size, cfg.num_attention_heads, cfg.num_hidden_layers, model.len_vis_input, cfg.vocab_size
        M, Mv = B * L, B * Nv
        dev = self.device

        def h(*s):
            return torch.empty(*s, device=dev, dtype=torch.float16)

        def f(*s):
            return torch.empty(*s, device=dev, dtype=torch.float32)

        ws = {"Lp": _ru(L, 32)}
        ws["maskb"] = torch.empty(B, L, ws["Lp"], device=dev, dtype=torch.uint8)
        ws["maskt"] = torch.empty(B, ws["Lp"], ws["Lp"], device=dev, dtype=torch.uint8)
        # kept rows of the dense step (vlp_kept_rows_build): per-sample lengths, the compact map of dense row indices, its length M'
        ws["kept_lens"], ws["kept_map"], ws["kept_n"] = (torch.empty(n, device=dev, dtype=torch.int32) for n in (B, M, 1))
        ws["img16"], ws["vpe_in"], ws["wpe_pad"] = h(Mv, 2048), h(Mv, PE_PAD), h(H, PE_PAD)
        ws["h1"], ws["vis_h"], ws["vispe_h"] = h(Mv, 2048), h(Mv, H), h(Mv, H)
        ws["emb_pre"], ws["x0"] = h(M, H), h(M, H)
        ws["stat0"] = (f(M), f(M))
        lay = []
        for _ in range(NL):
            lay.append({"qkv": h(M, 3 * H), "ctx": h(M, H), "lse": f(B, A, L), "pre1": h(M, H), "x1": h(M, H),
                        "st1": (f(M), f(M)), "z": h(M, I), "g": h(M, I), "pre2": h(M, H), "x2": h(M, H), "st2": (f(M), f(M))})
        ws["layers"] = lay
        # heads
        Vp = _ru(V, 64)
        ws["Vp"] = Vp
        if P > 0:
            R = B * P
            ws.update(sel=h(R, H), tz=h(R, H), tg=h(R, H), tln=h(R, H), tstat=(f(R), f(R)), logits=h(R, Vp), dlogits=h(R, Vp),
                      dlT=h(Vp, _ru(R, 64)),
                      lse_ce=f(R), coef=f(R), row_loss=f(R), dtln=h(R, H), dtg=h(R, H), dtz=h(R, H), dsel=h(R, H))
            # listed-row backward of the last layer (Engine.backward): the row list (<= R distinct masked rows, -1 padded), its length, and
            # the compact [R, *] gradients between the kernels that walk the list
            ws.update(lv_rows=torch.empty(R, device=dev, dtype=torch.int32), lv_n=torch.zeros(1, device=dev, dtype=torch.int32),
                      lv_dpre2=h(R, H), lv_dpre2_d=h(R, H), lv_dz=h(R, I), lv_dx1=h(R, H), lv_dpre1_d=h(R, H))
        ws["loss"] = f(260)
        if model.tasks == "vqa2":
            NA = model.num_answers
            NAp = _ru(NA, 64)
            ws.update(NAp=NAp, vq_e=h(B, H), vq_a1=h(B, 2 * H), vq_logits=h(B, NAp), vq_dlogits=h(B, NAp), vq_dz1=h(B, 2 * H), vq_de=h(B, H))
        # backward scratch (shared by all layers)
        ws.update(dx=h(M, H), dx_alt=h(M, H), dpre=h(M, H), dctx=h(M, H),
                  delta=f(B, A, L), d_vis_h=h(Mv, H), d_vispe_h=h(Mv, H), dz1v=h(Mv, 2048), dwpe_pad=h(H, PE_PAD), acc32=f(K.embed_bwd_workspace_floats(B, L, Nv, H)))
        # dY operands of the weight-gradient GEMMs, double-buffered by layer parity: the wgrads of layer i run on a side stream
        # while the main stream already works on layer i-1
        ws["dyset"] = [{"dpre2": h(M, H), "dpre2_d": h(M, H), "dpre1": h(M, H), "dpre1_d": h(M, H), "dz": h(M, I), "dqkv": h(M, 3 * H)}
                       for _ in range(2)]
        tn_bytes = max(K.gemm_tn_workspace_bytes(M, I, H), K.gemm_tn_workspace_bytes(Mv, 2048, 2048), K.gemm_tn_workspace_bytes(M, 3 * H, H))
        ws["tn_ws"] = torch.empty(tn_bytes, device=dev, dtype=torch.uint8)
        ws["tn_ws_main"] = torch.empty(max(K.gemm_tn_workspace_bytes(V, _ru(B * max(P, 1), 64), H), 1 << 20), device=dev, dtype=torch.uint8)
        ws["cs_ws"] = torch.empty(max(K.colsum_workspace_bytes(M, I), K.colsum_workspace_bytes(B * max(P, 1), Vp)), device=dev, dtype=torch.uint8)
        ws["ln_ws"] = torch.empty(K.layernorm_bwd_workspace_bytes(max(H, 8)), device=dev, dtype=torch.uint8)
        # one private partials slot per encoder / embedding LayerNorm: their dgamma / dbeta second stages run as ONE launch at the
        # end of backward (vlp_layernorm_bwd_reduce_batched) instead of 2 * layers + 1 tiny reduce kernels
        ws["ln_slot_bytes"] = K.layernorm_bwd_workspace_bytes(max(H, 8))
        ws["ln_slots"] = torch.empty((2 * NL + 1) * ws["ln_slot_bytes"], device=dev, dtype=torch.uint8)
        self._ws[key] = ws
        return ws

    def _shadows(self):
        """Transposed weight copies W^T (zero padded so that every dgrad K is a multiple of 64)."""
        if self._shadow is not None:
            return self._shadow
        model = self._model()
        cfg = model.config
        H, I, V = cfg.hidden_size, cfg.intermediate_size, cfg.vocab_size
        dev = self.device

        def h(*s):
            return torch.zeros(*s, device=dev, dtype=torch.float16)

        sh = {"layers": [{"qkvT": h(H, 3 * H), "oT": h(H, H), "w1T": h(H, I), "w2T": h(I, H)} for _ in range(cfg.num_hidden_layers)],
              "v2T": h(2048, H)}
        if model.tasks == "vqa2":
            NAp = _ru(model.num_answers, 64)
            sh.update(a2T=h(2 * H, NAp), a0T=h(H, 2 * H))
        else:
            sh.update(tT=h(H, H))
        self._shadow = sh
        return sh

    def _ln_table(self):
        """Device table [2 * layers + 1, 2] of (dgamma, dbeta) addresses: slot 2i = attention.output.LayerNorm of layer i, 2i + 1 =
        output.LayerNorm of layer i, last = embeddings.LayerNorm (addresses of the flat gradient buffer are stable)."""
        if self._ln_tab is None:
            rows = []
            for _, g in self._layers():
                rows += [[g.ln1_w.data_ptr(), g.ln1_b.data_ptr()], [g.ln2_w.data_ptr(), g.ln2_b.data_ptr()]]
            rows.append([self.G("bert.embeddings.LayerNorm.weight").data_ptr(), self.G("bert.embeddings.LayerNorm.bias").data_ptr()])
            self._ln_tab = torch.tensor(rows, dtype=torch.int64, device=self.device)
        return self._ln_tab

    def _refresh_shadows(self):
        """All W^T shadows of the step in one batched launch (descriptor table cached: buffer addresses are stable)."""
        sh = self._shadows()
        if "batch" not in sh:
            model = self._model()
            cfg = model.config
            H, I, V = cfg.hidden_size, cfg.intermediate_size, cfg.vocab_size
            items = []
            for s, (w, _) in zip(sh["layers"], self._layers()):
                items.append((w.qkv_w, H, s["qkvT"], 3 * H, 3 * H, H, 3 * H))   # packed [3H, H] -> [H, 3H]
                items.append((w.o_w, H, s["oT"], H, H, H, H))
                items.append((w.fc1_w, H, s["w1T"], I, I, H, I))
                items.append((w.fc2_w, I, s["w2T"], H, H, I, H))
            items.append((self.P("vis_embed.2.weight"), 2048, sh["v2T"], H, H, 2048, H))
            if model.tasks == "vqa2":
                NA = model.num_answers
                items.append((self.P("ans_classifier.2.weight"), 2 * H, sh["a2T"], _ru(NA, 64), NA, 2 * H, _ru(NA, 64)))
                items.append((self.P("ans_classifier.0.weight"), H, sh["a0T"], 2 * H, 2 * H, H, 2 * H))
            else:
                items.append((self.P("cls.predictions.transform.dense.weight"), H, sh["tT"], H, H, H, H))
            sh["batch"] = K.make_transpose_batch(items, self.device)
        K.transpose_batched(sh["batch"])

    # ------------------------------------------------------------------------------------------
    # forward
    # ------------------------------------------------------------------------------------------
    def _nt_variant(self, x, w, y, M, N, Kd, kw):
        """Staging/tiling variant for this problem size.  Deterministic (vlp_amd.tuning: committed table, else a shape
        heuristic) so that every box runs the same kernels and produces the same bits; with VLP_AUTOTUNE=1 every candidate
        (all compute the same contraction) is timed on the real call the first time a shape is seen."""
        if self.GEMM_NT_VARIANT is not None:
            return self.GEMM_NT_VARIANT
        key = (M, N, Kd)
        v = Engine._nt_choice.get(key)
        if v is not None:
            return v
        if not tuning.AUTOTUNE:
            v = Engine._nt_choice[key] = tuning.nt_variant(M, N, Kd)
            return v
        best = self.NT_CANDIDATES[0]
        if M * N >= 128 * 128 * 4:          # tiny problems: not worth timing
            # (256-wide n tiles leave most CUs idle on narrow outputs: not candidates there)
            cands = [c for c in (self.NT_CANDIDATES_SKINNY if M <= 1024 else self.NT_CANDIDATES)
                     if not ((c & 7 == 5 and c < 64 or c == 73) and N < 1024)]
            torch.cuda.synchronize()        # nothing else (e.g. side-stream wgrads) may run while candidates are timed
            best = tuning.best_of(cands, lambda c, i: K.gemm_nt(x, w, y, M, N, Kd, variant=c, **kw), rounds=2, reps=4 if M > 1024 else 12)
        Engine._nt_choice[key] = best
        tuning.remember("nt", M, N, Kd, best)
        return best

    def _nt(self, x, w, y, M, N, Kd, **kw):
        v = self._nt_variant(x, w, y, M, N, Kd, kw)
        if self.prof is not None:
            self._prof_ctr += 1
        if self.prof is None or self._prof_ctr % self.PROF_EVERY:
            K.gemm_nt(x, w, y, M, N, Kd, variant=v, **kw)
            return
        # events are recorded on torch's current stream == the stream handed to the C ABI.  While backward has weight-gradient GEMMs
        # in flight on the side stream, a sampled launch waits for them (and they for it), so that the bracket times ONE kernel.
        side = self._side if self._side_busy else None
        main = torch.cuda.current_stream()
        if side is not None:
            main.wait_stream(side)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        K.gemm_nt(x, w, y, M, N, Kd, variant=v, **kw)
        e1.record()
        if side is not None:
            side.wait_stream(main)
        self.prof.append((e0, e1, 2.0 * M * N * Kd))

    def _nt_skinny(self, x, w, y, M, N, Kd, skws, tune_ws=None, **kw):
        """NT GEMM of the incremental decoder (M = sequences x 2 rows): the ordinary kernels have only N/128 workgroups to run, so the
        split-K form (vlp_gemm_nt_splitk) and every ordinary variant are timed once per shape.  `tune_ws()` returns same-shaped weight
        tensors (the same projection in all layers) to cycle through while timing: in a real token step every weight is read once, i.e.
        from HBM / Infinity Cache, not from a warm L2 -- timing one weight back to back would rank the candidates for the wrong regime."""
        if M > 1024 or N > 4096 or Kd < 256:
            return self._nt(x, w, y, M, N, Kd, **kw)
        key = (M, N, Kd)
        ch = Engine._skinny_choice.get(key)
        if ch is None and not tuning.AUTOTUNE:
            ch = Engine._skinny_choice[key] = tuning.skinny_choice(M, N, Kd)
        if ch is None:
            wl = list(tune_ws()) if tune_ws is not None else [w]
            cands = [("v", v) for v in self.NT_CANDIDATES_SKINNY] + [("s", sp) for sp in tuning.SKINNY_SPLITS if Kd // 64 >= sp]

            def launch(c, i):
                ww = wl[i % len(wl)]
                if c[0] == "v":
                    K.gemm_nt(x, ww, y, M, N, Kd, variant=c[1], **kw)
                else:
                    K.gemm_nt_splitk(x, ww, y, M, N, Kd, c[1], skws, **kw)
            torch.cuda.synchronize()
            # three rounds: these are 5-40 us kernels, one noisy sample would otherwise pin a bad choice for the life of the process
            ch = tuning.best_of(cands, launch, rounds=3, reps=max(12, len(wl)))
            K.gemm_nt(x, w, y, M, N, Kd, variant=1, **kw)        # leave y as computed from the caller's weight
            Engine._skinny_choice[key] = ch
            tuning.remember("sk", M, N, Kd, ch)
        if ch[0] == "v":
            K.gemm_nt(x, w, y, M, N, Kd, variant=ch[1], **kw)
        else:
            K.gemm_nt_splitk(x, w, y, M, N, Kd, ch[1], skws, **kw)

    def _pretext_workspace(self, ws, B, Pm):
        """Buffers of the mask_image_regions / vis_pretext branch (modeling.py:1049-1056, 1113-1131), created on first use."""
        key = ("pt", Pm)
        if key not in ws:
            model = self._model()
            H, Nv, dev = model.config.hidden_size, model.len_vis_input, self.device
            ws[key] = dict(rmask=torch.empty(B * Nv, device=dev, dtype=torch.uint8), pos0=torch.zeros(B, 1, device=dev, dtype=torch.long),
                           sel0=torch.empty(B, H, device=dev, dtype=torch.float16), pooled=torch.empty(B, H, device=dev, dtype=torch.float16),
                           probs=torch.empty(B, Pm, Pm, device=dev, dtype=torch.float32), sample=torch.empty(B, device=dev, dtype=torch.float32),
                           loss=torch.empty(1, device=dev, dtype=torch.float32), dpool=torch.empty(B, H, device=dev, dtype=torch.float16),
                           dsel0=torch.empty(B, H, device=dev, dtype=torch.float16), pT=torch.empty(H, H, device=dev, dtype=torch.float16))
        return ws[key]

    def _kept_lengths(self, attention_mask, masked_pos, B, L, Nv):
        """Per-sample number of leading positions the packed step keeps (host ints): 1 + the last key column ANY query attends, and at
        least what the heads read (masked_pos, position Nv+1).  Every dropped position is therefore attended by no query at all.
        MaskSpec carries the lengths on the host (lens_host = second_end, the loader knows them); a dense int64 mask is reduced on the
        device and read back ONCE per tensor object (the result is remembered while that tensor is alive and unmodified -- a device-
        resident batch pool, bench.py / --synthetic, pays the read-back in its first pass only)."""
        if isinstance(attention_mask, MaskSpec):
            # (lens_host is the loader's promise that nothing past it is attended OR read: masked_pos lies inside the tokens by construction,
            # seq2seq_loader.py:256-265; the gather clamps a position past the kept rows to the last kept row, as the dense kernel clamps to L - 1)
            if attention_mask.lens_host is None:
                return None
            lens = [max(int(n), Nv + 2) for n in attention_mask.lens_host]
            return lens if len(lens) == B and max(lens) <= L else None
        if attention_mask is None or attention_mask.dim() != 3:
            return None
        key = id(attention_mask)
        hit = self._pk_lens.get(key)
        if hit is not None and hit[0]() is attention_mask and hit[1] == attention_mask._version and \
                (hit[2] is None) == (masked_pos is None) and (masked_pos is None or (hit[2]() is masked_pos and hit[4] == masked_pos._version)):
            self._rb_streak = 0
            return hit[3]           # the SAME tensor objects, unmodified (weak references: a recycled id() cannot alias)
        # a fresh dense mask: its lengths cost a reduction + a device -> host read-back in front of this forward
        if self.varlen == "auto":
            if self.varlen_readback_budget <= 0:
                self._warn_readback("the padding-free step is OFF for this batch: its dense [B, L, L] attention mask is a new tensor, and deriving the kept "
                                    "lengths from it would stall the launch queue once per step")
                return None
            self.varlen_readback_budget -= 1
        else:
            self._rb_streak += 1
            if self._rb_streak > 8:
                self._warn_readback("the padding-free step derives the kept lengths of a NEW dense [B, L, L] attention mask every step: one device -> host "
                                    "read-back (a launch-queue stall) per step")
        cols = (attention_mask != 0).any(dim=1)                                            # [B, L]: key column attended by some query
        idx = torch.arange(1, L + 1, device=cols.device, dtype=torch.int32)
        n = (cols.to(torch.int32) * idx).amax(dim=1)
        n = torch.clamp(n, min=Nv + 2)
        if masked_pos is not None and masked_pos.numel() > 0:
            n = torch.maximum(n, (masked_pos.to(torch.int32).amax(dim=1) + 1).clamp(max=L))
        lens = [int(v) for v in n.tolist()]                                              # the one host read-back
        if len(self._pk_lens) > 64:
            self._pk_lens = {k: v for k, v in self._pk_lens.items() if v[0]() is not None}
            if len(self._pk_lens) > 64:
                self._pk_lens.clear()
        self._pk_lens[key] = (weakref.ref(attention_mask), attention_mask._version, weakref.ref(masked_pos) if masked_pos is not None else None, lens,
                              masked_pos._version if masked_pos is not None else 0)
        return lens

    def _warn_readback(self, what):
        if self._rb_warned:
            return
        self._rb_warned = True
        import warnings
        warnings.warn("vlp_amd: " + what + ".  Hand the engine vlp_amd.input_prep.MaskSpec (three int32 per sample + the lengths on the host: what "
                      "vlp_amd.data.BatchPrefetcher delivers) in place of the dense mask, or keep the mask tensors resident and reuse them; "
                      "VLP_VARLEN=0 silences this, VLP_VARLEN=1 accepts the read-back.", VlpPerformanceWarning, stacklevel=3)

    PK_STAGE_SLOTS = 8

    def _packing(self, lens, B, L):
        """(row_off int32 [B+1], row_map int32 [M'], M') on the device for the kept lengths `lens`.  Batches of a resident pool / an epoch
        replay hit the cache; a real loader produces a new length tuple every step: its offsets go through a small RING of pinned staging
        buffers (no hipHostMalloc per step, nothing pinned kept per cache entry -- ADVICE r5), one async H2D copy + one rowmap_build launch."""
        key = (L,) + tuple(lens)
        ent = self._pk_cache.get(key)
        if ent is None:
            if self._pk_stage is None or self._pk_stage[0][0].numel() < B + 1:
                self._pk_stage = [[torch.empty(max(B + 1, 257), dtype=torch.int32).pin_memory(), torch.cuda.Event()] for _ in range(self.PK_STAGE_SLOTS)]
                self._pk_stage_i = 0
            host, ev = self._pk_stage[self._pk_stage_i]
            self._pk_stage_i = (self._pk_stage_i + 1) % self.PK_STAGE_SLOTS
            ev.synchronize()                       # the copy issued from this buffer PK_STAGE_SLOTS misses ago (long done; never-recorded: returns at once)
            off = np.zeros(B + 1, dtype=np.int32)
            np.cumsum(np.asarray(lens, dtype=np.int32), out=off[1:])
            host.numpy()[:B + 1] = off
            row_off = torch.empty(B + 1, dtype=torch.int32, device=self.device)
            row_off.copy_(host[:B + 1], non_blocking=True)
            ev.record()
            Mp = int(off[-1])
            row_map = torch.empty(Mp, dtype=torch.int32, device=self.device)
            K.rowmap_build(row_off, B, L, row_map)
            if len(self._pk_cache) >= 64:
                self._pk_cache.clear()
            ent = self._pk_cache[key] = (row_off, row_map, Mp)
        return ent[0], ent[1], ent[2]

    def _check_regions(self, vis_feats, vis_pe):
        model = self._model()
        H, A, Nv = model.config.hidden_size, model.config.num_attention_heads, model.len_vis_input
        if H != A * 64:
            raise RuntimeError("vlp_amd: attention kernels need head_dim == 64 (hidden %d, heads %d)" % (H, A))
        if vis_feats.shape[1] != Nv or vis_feats.shape[2] != 2048 or vis_pe.shape[2] != PE_DIM:
            raise RuntimeError("vlp_amd: expected vis_feats [B,%d,2048] and vis_pe [B,%d,%d]" % (Nv, Nv, PE_DIM))

    def _region_inputs(self, ws, vis_feats, vis_pe):
        """Operands of the three region GEMMs.  Launches the fp16 cast of fp32 image features and returns (img, prep_pe): prep_pe() launches
        the K-padded box / class encoding into ws["vpe_in"] and the K-padded copy of its weight into ws["wpe_pad"] (a training forward
        runs it on its side stream)."""
        B, Nv, H = vis_feats.shape[0], vis_feats.shape[1], self._model().config.hidden_size
        Mv = B * Nv
        vf = vis_feats.reshape(Mv, 2048)
        if vf.dtype == torch.float32:
            K.copy2d(vf.contiguous(), 2048, True, ws["img16"], 2048, Mv, 2048, 2048)
            img = ws["img16"]
        else:
            img = vf.contiguous()

        def prep_pe():
            if isinstance(vis_pe, RawRegions):  # raw boxes + class probabilities -> K-padded encoding (seq2seq_loader.py:338-351)
                vis_pe.check(B, Nv)
                K.vis_pe_prep(vis_pe.bbox, vis_pe.cls_prob.reshape(Mv, PE_DIM - 6), ws["vpe_in"], B, Nv, PE_DIM - 6, PE_PAD)
            else:
                vp = vis_pe.reshape(Mv, PE_DIM).contiguous()
                K.copy2d(vp, PE_DIM, vp.dtype == torch.float32, ws["vpe_in"], PE_PAD, Mv, PE_DIM, PE_PAD)
            # parameters written by a pipelined optimizer step become readable chunk by chunk (wait_params is a no-op otherwise)
            # (reads a parameter of the embeddings bucket: AFTER the wait, or a pipelined step would project with last step's weight)
            self.wait_params(len(self.buckets) - 1, consume=False)      # region projections (this may run on the side stream)
            K.copy2d(self.P("vis_pe_embed.0.weight"), PE_DIM, False, ws["wpe_pad"], PE_PAD, H, PE_DIM, PE_PAD)
        return img, prep_pe

    def _side_stream(self):
        if self._side is None:
            self._side = torch.cuda.Stream(device=self.device)
            self._side_done = [None, None]
        return self._side

    def _prep_mask(self, st, am, want_t):
        """The packed attention masks of this forward (want_t: also the transposed one backward reads) and the map of a dense step's kept rows."""
        ws, B, L, P, Nv = st.ws, st.B, st.L, st.P, self._model().len_vis_input
        pt, mask_spec = st.pretext, isinstance(am, MaskSpec)
        if mask_spec:                       # per-sample lengths -> packed masks on the device (seq2seq_loader.py:292-301)
            am.check(B, L)
            # (BLOCK_MASKED_REGION_KEYS: opt-in, the reference's own loader leaves the masked regions' key columns attendable, see above)
            K.mask_build(am.second_st, am.second_end, am.is_s2s, ws["maskb"], B, L, ws["Lp"], out_t=want_t,
                         region_mask=pt[0]["rmask"] if (pt is not None and self.BLOCK_MASKED_REGION_KEYS) else None, Nv=Nv)
        else:
            if am is None:
                am = torch.ones(B, L, dtype=torch.long, device=st.batch[1].device)
            if am.dim() == 2:       # modeling.py:818-819
                am = am[:, None, :].expand(B, L, L)
            am = am.to(torch.long).contiguous()
            K.mask_pack(am, ws["maskb"], B, L, ws["Lp"], out_t=want_t)
        if st.kept is not None:
            # the rows whose gradient can be non-zero in this dense step, by the rule of _kept_lengths, on the device (no read-back: the
            # host never learns M'): every later position is attended by no query and read by no head, so its dY is an exact zero in
            # every weight gradient of every layer, and the grouped wgrad (backward) contracts over the mapped rows only
            K.kept_rows_build(B, L, Nv, ws["kept_lens"], ws["kept_map"], ws["kept_n"], maskb=None if mask_spec else ws["maskb"], Lp=ws["Lp"],
                              lens_in=am.second_end if mask_spec else None, pos=st.batch[3].to(torch.long).contiguous() if P > 0 else None)

    def _fwd_inputs(self, st, attention_mask, prep_pe, with_grad):
        """Input preparation of a forward.  With gradients and the side stream it runs underneath the forward: (1) the K-padded box / class
        operand of the third region GEMM, (2) the packed attention masks (first read by layer 0's attention, ~190 us into the forward),
        (3) the W^T shadows of this step's dgrad GEMMs (the weights are final once the optimizer has stepped; 78 us, first read at the head
        of backward, behind _shadow_ev).  The main stream starts the region projections at once and waits for the events of (1) / (2),
        returned here, where it first reads them; (None, None): everything was issued on the main stream."""
        self._shadow_ev = None
        want_t = st.ws["maskt"] if with_grad else None
        if not (with_grad and self.WGRAD_SIDE_STREAM):
            self._prep_mask(st, attention_mask, want_t)
            prep_pe()
            return None, None
        side = self._side_stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            prep_pe()
            pe_ev = torch.cuda.Event()
            pe_ev.record(side)
            self._prep_mask(st, attention_mask, want_t)
            mask_ev = torch.cuda.Event()
            mask_ev.record(side)
            if self._params_done is not None:
                side.wait_event(self._params_done)        # the transposes read every weight matrix
            if self._param_works is not None:
                # sharded optimizer step: the parameters arrive by per-bucket all-gathers that may still be in flight; the
                # transposes read EVERY weight matrix, so this stream waits for all of them (the main stream keeps waiting per
                # bucket where the forward first reads it -- Work.wait() may be called again there)
                for w in self._param_works.values():
                    if w is not None:
                        w.wait()
            self._refresh_shadows()
            self._shadow_ev = torch.cuda.Event()
            self._shadow_ev.record(side)
        return pe_ev, mask_ev

    def _fwd_layer(self, st, i, x, mask_ev):
        """Encoder layer i on the hidden states x (modeling.py:268-372); returns its output.  mask_ev: the event behind the packed masks,
        waited for in front of the attention (layer 0 of a forward that prepared them on the side stream)."""
        cfg = self._model().config
        H, I, A = cfg.hidden_size, cfg.intermediate_size, cfg.num_attention_heads
        a, (w, _), seed, (p, pa) = st.ws["layers"][i], self._layers()[i], st.seed, st.p_drop
        ro, rm, M = st.pk if st.pk is not None else (None, None, st.B * st.L)
        self._nt(x, w.qkv_w, a["qkv"], M, 3 * H, H, bias=w.qkv_b)
        if mask_ev is not None:
            torch.cuda.current_stream().wait_event(mask_ev)
        K.attn_fwd(a["qkv"], st.ws["maskb"], a["ctx"], a["lse"], st.B, st.L, A, 1.0 / math.sqrt(H // A), dropout_p=pa, seed=seed,
                   rng_stream=16 * i + 1, row_off=ro)
        self._nt(a["ctx"], w.o_w, a["pre1"], M, H, H, bias=w.o_b, residual=x, dropout_p=p, seed=seed, rng_stream=16 * i + 2, row_map=rm)
        K.layernorm_fwd(a["pre1"], w.ln1_w, w.ln1_b, a["x1"], M, H, a["st1"][0], a["st1"][1])
        # a["z"] receives gelu'(z), not z: the only consumer is the FFN-down dgrad epilogue, which then multiplies by a stored
        # number instead of re-evaluating erf + exp per element
        self._nt(a["x1"], w.fc1_w, a["g"], M, I, H, bias=w.fc1_b, preact=a["z"], act=K.ACT_GELU_SAVE_GRAD)
        self._nt(a["g"], w.fc2_w, a["pre2"], M, H, I, bias=w.fc2_b, residual=a["x1"], dropout_p=p, seed=seed, rng_stream=16 * i + 3, row_map=rm)
        K.layernorm_fwd(a["pre2"], w.ln2_w, w.ln2_b, a["x2"], M, H, a["st2"][0], a["st2"][1])
        return a["x2"]

    def _fwd_heads(self, st, x, want_vqa):
        """The heads' forward up to the logits on the last layer's output x: masked LM (P > 0), the VQA classifier, pooler + pretext loss."""
        model = self._model()
        H, V, Nv = model.config.hidden_size, model.config.vocab_size, model.len_vis_input
        ws, B, L, P, pt = st.ws, st.B, st.L, st.P, st.pretext
        ro = st.pk[0] if st.pk is not None else None
        if P > 0:
            C = "cls.predictions."
            R = B * P
            K.gather_rows(x, H, st.batch[3].contiguous(), ws["sel"], H, B, P, L, H, row_off=ro)
            self._nt(ws["sel"], self.P(C + "transform.dense.weight"), ws["tg"], R, H, H, bias=self.P(C + "transform.dense.bias"),
                     preact=ws["tz"], act=K.ACT_GELU)
            K.layernorm_fwd(ws["tg"], self.P(C + "transform.LayerNorm.weight"), self.P(C + "transform.LayerNorm.bias"), ws["tln"], R, H,
                            ws["tstat"][0], ws["tstat"][1])
            self._nt(ws["tln"], self.P("bert.embeddings.word_embeddings.weight"), ws["logits"], R, V, H, bias=self.P(C + "bias"), ldy=ws["Vp"])
        if want_vqa:
            NA = model.num_answers
            K.vqa_mul_fwd(x, ws["vq_e"], B, L, Nv, H, row_off=ro)
            self._nt(ws["vq_e"], self.P("ans_classifier.0.weight"), ws["vq_a1"], B, 2 * H, H, bias=self.P("ans_classifier.0.bias"), act=K.ACT_RELU)
            self._nt(ws["vq_a1"], self.P("ans_classifier.2.weight"), ws["vq_logits"], B, NA, 2 * H, bias=self.P("ans_classifier.2.bias"), ldy=ws["NAp"])
        if pt is not None:
            # BertPooler (modeling.py:411-417) -- only this branch reads it -- and the pretext loss (:1113-1131)
            ptw, vmp = pt
            K.gather_rows(x, H, ptw["pos0"], ptw["sel0"], H, B, 1, L, H, row_off=ro)
            self._nt(ptw["sel0"], self.P("bert.pooler.dense.weight"), ptw["pooled"], B, H, H, bias=self.P("bert.pooler.dense.bias"), act=K.ACT_TANH)
            K.pretext_fwd(ws["vis_h"], ws["vispe_h"], ptw["pooled"], vmp, ptw["probs"], ptw["sample"], ptw["loss"], B, Nv, vmp.shape[1], H)

    def forward(self, vis_feats, vis_pe, input_ids, token_type_ids, attention_mask, masked_pos, train, want_mlm, want_vqa,
                vis_masked_pos=None, position_ids=None, dropout=True, dense=False):
        """Runs embeddings + encoder (+ heads' forward up to the logits).  Returns the _State.  vis_masked_pos ([B, Pm] int64, values
        1..Nv): the mask_image_regions branch -- those region rows enter the encoder as zeros and the pooled output is computed
        for the pretext loss (pretext_loss()).  position_ids ([B, L] int64): explicit position ids (default 0..L-1); dropout=False: a
        training forward without dropout; dense=True: never the padding-free step (the SCST scoring pass, score_samples)."""
        self.pack()
        model = self._model()
        cfg = model.config
        H, NL, Nv = cfg.hidden_size, cfg.num_hidden_layers, model.len_vis_input
        B, L = input_ids.shape
        self._check_regions(vis_feats, vis_pe)
        if L < Nv + 2:
            raise RuntimeError("vlp_amd: sequence length %d too short for %d regions" % (L, Nv))
        P = masked_pos.shape[1] if (want_mlm and masked_pos is not None and masked_pos.numel() > 0) else 0
        ws = self._workspace(B, L, P)
        self.gen += 1
        p = cfg.hidden_dropout_prob if (train and dropout) else 0.0
        pa = cfg.attention_probs_dropout_prob if (train and dropout) else 0.0
        if train and (p > 0 or pa > 0):
            self.step_seed += 1
        seed = self.base_seed + self.step_seed
        M, Mv = B * L, B * Nv
        # ---- padding-free layout (opt-in): row_off / row_map / M' from the mask's own kept lengths --------------------------------
        ro = rm = None
        if self.varlen and not dense and (train or torch.is_grad_enabled()) and L <= 192 and os.environ.get("VLP_ATTN_BWD") is None:
            lens = self._kept_lengths(attention_mask, masked_pos if P > 0 else None, B, L, Nv)
            if lens is not None and sum(lens) < M:
                ro, rm, M = self._packing(lens, B, L)
        self.last_packed_rows = M if ro is not None else None

        # ---- inputs -----------------------------------------------------------------------------
        pt = None
        if vis_masked_pos is not None and vis_masked_pos.numel() > 0:
            Pm = vis_masked_pos.shape[1]
            pt = self._pretext_workspace(ws, B, Pm)
            st_vmp = vis_masked_pos.to(torch.long).contiguous()
            K.region_mask_build(st_vmp, pt["rmask"], B, Pm, Nv)
        self._pretext_on = pt is not None
        img, prep_pe = self._region_inputs(ws, vis_feats, vis_pe)
        st = _State()
        st.gen, st.B, st.L, st.P, st.ws, st.has_mlm = self.gen, B, L, P, ws, P > 0
        st.seed, st.p_drop, st.pos_ids = seed, (p, pa), position_ids
        st.batch = (img, input_ids.contiguous(), token_type_ids.contiguous(), masked_pos)
        st.pk = (ro, rm, M) if ro is not None else None
        st.pretext = (pt, st_vmp) if pt is not None else None
        # dense training step with a grouped wgrad (backward: M >= 2048): the map of its kept rows rides along (VLP_WGRAD_KEPT=0: off).
        # dense=True (score_samples) stays unmapped by contract: its head reads sampled rows the rule does not cover
        if (ro is None and not dense and (train or torch.is_grad_enabled()) and M >= 2048
                and os.environ.get("VLP_WGRAD_KEPT", "1") != "0"):
            st.kept = (ws["kept_map"], ws["kept_n"])

        pe_ev, mask_ev = self._fwd_inputs(st, attention_mask, prep_pe, train or torch.is_grad_enabled())
        self.wait_params("nodecay")
        self.wait_params(len(self.buckets) - 1)             # region projections
        self.wait_params(len(self.buckets) - 2)             # embedding tables
        # ---- region projections (modeling.py:1003-1018,1035-1036) ---------------------------------
        self._nt(img, self.P("vis_embed.0.weight"), ws["h1"], Mv, 2048, 2048, bias=self.P("vis_embed.0.bias"), act=K.ACT_RELU)
        self._nt(ws["h1"], self.P("vis_embed.2.weight"), ws["vis_h"], Mv, H, 2048, bias=self.P("vis_embed.2.bias"), act=K.ACT_RELU,
                 dropout_p=p, seed=seed, rng_stream=1001)
        if pe_ev is not None:
            torch.cuda.current_stream().wait_event(pe_ev)
        self._nt(ws["vpe_in"], ws["wpe_pad"], ws["vispe_h"], Mv, H, PE_PAD, bias=self.P("vis_pe_embed.0.bias"), act=K.ACT_RELU,
                 dropout_p=p, seed=seed, rng_stream=1002)
        # ---- embeddings (modeling.py:217-241) ------------------------------------------------------
        E = "bert.embeddings."
        K.embed_fwd(st.batch[1], st.batch[2], self.P(E + "word_embeddings.weight"), self.P(E + "position_embeddings.weight"),
                    self.P(E + "token_type_embeddings.weight"), ws["vis_h"], ws["vispe_h"], ws["emb_pre"], B, L, Nv, H,
                    position_ids=position_ids, region_mask=pt["rmask"] if pt is not None else None, row_map=rm, rows=M if rm is not None else 0)
        K.layernorm_fwd(ws["emb_pre"], self.P(E + "LayerNorm.weight"), self.P(E + "LayerNorm.bias"), ws["x0"], M, H, ws["stat0"][0], ws["stat0"][1],
                        dropout_p=p, seed=seed, rng_stream=1000, row_map=rm)
        # ---- encoder, then the heads up to the logits -------------------------------------------------
        x = ws["x0"]
        for i in range(NL):
            self.wait_params(NL - i)                            # bucket of layer i
            x = self._fwd_layer(st, i, x, mask_ev if i == 0 else None)
        self.wait_params(0)
        self._fwd_heads(st, x, want_vqa)
        return st

    def pretext_loss(self, st):
        """[1] f32 view holding the vis_pretext_loss of this forward (modeling.py:1131)."""
        return st.pretext[0]["loss"]

    def pooled_output(self, st):
        return st.pretext[0]["pooled"]

    def mlm_loss(self, st, labels, weights, drop_worst_ratio):
        """modeling.py:1083-1111 on the logits of this forward; returns a [1] f32 view holding the loss."""
        ws = st.ws
        model = self._model()
        V = model.config.vocab_size
        st.task_labels = labels.contiguous()
        crit = getattr(model, "crit_mask_lm_smoothed", None)
        if crit is None:
            K.mlm_loss_fwd(ws["logits"], ws["Vp"], st.task_labels, weights.to(torch.long).contiguous(), ws["loss"], ws["lse_ce"], ws["coef"],
                           ws["row_loss"], st.B, st.P, V, drop_worst_ratio=float(drop_worst_ratio))
        else:
            # label smoothing (modeling.py:1104-1106): the KL kernels; the choice is recorded on st so that backward follows this forward
            s, c, q_sum, q_log_q = crit.kernel_scalars()
            K.mlm_loss_ls_fwd(ws["logits"], ws["Vp"], st.task_labels, weights.to(torch.long).contiguous(), ws["loss"], ws["lse_ce"], ws["coef"],
                              ws["row_loss"], st.B, st.P, V, s, c, q_sum, q_log_q, ignore_index=crit.ignore_index,
                              drop_worst_ratio=float(drop_worst_ratio))
            st.mlm_smooth = (s, c, q_sum, crit.ignore_index)          # the arguments of the matching backward launch
        return ws["loss"][0:1]

    def vqa_loss(self, st, ans_labels):
        """modeling.py:1140: BCEWithLogits(mean) * num_answers.  ans_labels: the dense [B, num_answers] target, or a SparseAnswers -- then the
        kernels read the (index, score) pairs; the choice is recorded on st (task_labels) so that backward follows this forward."""
        ws = st.ws
        NA = self._model().num_answers
        if isinstance(ans_labels, SparseAnswers):
            ans_labels.check(st.B, NA)
            if not (ans_labels.idx.is_cuda and ans_labels.score.is_cuda):
                raise RuntimeError("SparseAnswers must live on the GPU (there is no CPU path)")
            st.task_labels = SparseAnswers(ans_labels.idx.contiguous(), ans_labels.score.contiguous(), ans_labels.verified_for)
            K.bce_sparse_loss_fwd(ws["vq_logits"], ws["NAp"], st.task_labels.idx, st.task_labels.score, st.B, NA, ws["loss"])
            return ws["loss"][0:1]
        st.task_labels = ans_labels.to(torch.float32).contiguous()
        K.bce_loss_fwd(ws["vq_logits"], ws["NAp"], st.task_labels, st.task_labels.stride(0), st.B, NA, ws["loss"])
        return ws["loss"][0:1]

    def mlm_logits(self, st):
        V = self._model().config.vocab_size
        return st.ws["logits"][:, :V].view(st.B, st.P, V)

    def vqa_logits(self, st):
        return st.ws["vq_logits"][:, :self._model().num_answers]

    def sequence_output(self, st):
        """[B, L, H] hidden states of the last layer.  After a packed forward the dropped (padding) positions hold zeros -- the dense
        run computes values there that nothing consumes."""
        cfg = self._model().config
        x = st.ws["layers"][cfg.num_hidden_layers - 1]["x2"]
        if st.pk is not None:
            dense = torch.zeros(st.B * st.L, cfg.hidden_size, device=x.device, dtype=x.dtype)
            K.rows_unpack(x, st.pk[1], st.pk[2], dense, cfg.hidden_size)
            x = dense
        return x.view(st.B, st.L, cfg.hidden_size)

    # ------------------------------------------------------------------------------------------
    # self-critical sequence training: the gradient of the sampled captions' log-probabilities
    # ------------------------------------------------------------------------------------------
    def score_samples(self, vis_feats, vis_pe, input_ids, token_type_ids, position_ids, attention_mask, sample_ids, mask_word_id,
                      temperature=1.0, entropy=False):
        """Teacher-forced scoring of sampled captions (the gradient the reference gets by running its incremental decoder under autograd,
        modeling.py:1210-1251 / run_img2txt_dist.py:506-507).  Takes the decoder's inputs and its sampled ids [B, T]; builds the scoring
        sequence on the device (vlp_scst_layout: every sampled position sees exactly the hidden states the incremental decoder computed),
        runs the training forward on it densely and without dropout, the LM head over the T [MASK] slots and vlp_token_logprob_fwd.
        Returns (state, logp [B, T] f32 -- a workspace view, overwritten by the next call); backward(state, None, "logprob", g_rows=...).
        temperature T != 1 or entropy=True score the policy softmax(logits / T) with vlp_token_policy_fwd instead: logp is that policy's, and
        with entropy=True the return is (state, logp, entropy), entropy [B, T] f32 the policy's entropy at every position (a workspace view
        next to logp; backward(..., h_rows=...) takes its upstream gradient).  (1.0, False) issues the launches of a call without them."""
        temperature, entropy = float(temperature), bool(entropy)
        if not (0.0 < temperature < float("inf")):
            raise RuntimeError("vlp_amd: score_samples needs a finite temperature > 0 (got %r)" % temperature)
        st, sw, B, T, V = self._scoring_forward(vis_feats, vis_pe, input_ids, token_type_ids, position_ids, attention_mask, sample_ids, mask_word_id,
                                                "score_samples expects sampled ids", "SCST scoring sequence", "--max_len_b")
        if temperature == 1.0 and not entropy:
            K.token_logprob_fwd(st.ws["logits"], st.ws["Vp"], st.task_labels, sw["logp"], st.ws["lse_ce"], B * T, V)
            return st, sw["logp"]
        if entropy and "entropy" not in sw:
            sw["entropy"] = torch.empty(B, T, device=self.device, dtype=torch.float32)
        ent = sw["entropy"] if entropy else None
        K.token_policy_fwd(st.ws["logits"], st.ws["Vp"], st.task_labels, sw["logp"], st.ws["lse_ce"], B * T, V, temperature=temperature, entropy=ent)
        st.policy = (temperature, ent)
        return (st, sw["logp"], ent) if entropy else (st, sw["logp"])

    def score_captions(self, vis_feats, vis_pe, input_ids, token_type_ids, position_ids, attention_mask, caption_ids, mask_word_id,
                       return_logits=False, uncounted_fill=0):
        """Inference: how probable given captions are.  Takes the decoder's inputs and caption_ids [R, T] (T = output length - input length; row r
        is scored against image row r); a position holding -1 is not counted.  The pass is score_samples' -- vlp_scst_layout, the dense forward
        without dropout, the LM head over the T [MASK] slots, in the ("scst", B, in_len, T) workspace -- under no_grad, and one vlp_token_score
        launch in place of vlp_token_logprob_fwd: logp holds score_samples' bits.  An uncounted position is fed to the model as id 0 (no later
        counted position of a causal caption attends to it) and its logits row is not read.
        Returns (logp f32, entropy f32, rank int32, top_id int64), each [R, T] and the caller's own (copies); an uncounted position holds
        (0, 0, -1, -1).  Test hooks: return_logits=True appends the fp16 rows that were scored, [R, T, V]; uncounted_fill is the id fed in place
        of a -1.  Refused in train() mode with gradients enabled: nothing here is differentiable (that is score_samples)."""
        model = self._model()
        if model.training and torch.is_grad_enabled():
            raise RuntimeError("vlp_amd: score_captions is an inference entry (no gradient); call it under eval() or torch.no_grad() -- "
                               "differentiable log-probabilities come from sample_mode='sample' in train() mode")
        with torch.no_grad():
            cap = caption_ids.to(torch.long)
            fed = torch.where(cap < 0, torch.full_like(cap, int(uncounted_fill)), cap)
            st, _, B, T, V = self._scoring_forward(vis_feats, vis_pe, input_ids, token_type_ids, position_ids, attention_mask, fed, mask_word_id,
                                                   "score_captions expects caption ids", "scoring sequence", "--max_tgt_length")
            dev = self.device
            logp, lse, ent, top_logit = (torch.empty(B, T, device=dev, dtype=torch.float32) for _ in range(4))
            rank = torch.empty(B, T, device=dev, dtype=torch.int32)
            top_id = torch.empty(B, T, device=dev, dtype=torch.long)
            K.token_score(st.ws["logits"], st.ws["Vp"], cap.contiguous().view(-1), logp, lse, ent, rank, top_id, top_logit, B * T, V)
            out = (logp, ent, rank, top_id)
            if return_logits:
                out += (st.ws["logits"][:B * T, :V].reshape(B, T, V).clone(),)
        return out

    def _scoring_forward(self, vis_feats, vis_pe, input_ids, token_type_ids, position_ids, attention_mask, ids, mask_word_id, expects, what, flag):
        """The pass score_samples and score_captions share: the checks (a refused call leaves no workspace behind), the ("scst", B, in_len, T)
        workspace, vlp_scst_layout of the ids [B, T] and the dense training forward without dropout with the LM head over the T [MASK] slots.
        Returns (state, workspace, B, T, V); state.task_labels are the ids, state.ws["logits"] the B * T rows to score."""
        self.pack()
        model = self._model()
        V = model.config.vocab_size
        B, in_len, out_len = self._decode_check(vis_feats, vis_pe, input_ids, token_type_ids, attention_mask)
        T = out_len - in_len
        if tuple(ids.shape) != (B, T):
            raise RuntimeError("vlp_amd: %s [B, %d] (output length - input length), got %s" % (expects, T, tuple(ids.shape)))
        Lo = in_len + 2 * T - 1
        if Lo > 256:
            raise RuntimeError("vlp_amd: the %s has %d + 2 x %d - 1 = %d positions, more than the attention kernels' 256; "
                               "lower %s" % (what, in_len, T, Lo, flag))
        key = ("scst", B, in_len, T)
        sw = self._ws.get(key)
        if sw is None:
            dev = self.device

            def i64(*sh):
                return torch.empty(*sh, device=dev, dtype=torch.long)
            sw = self._ws[key] = dict(ids=i64(B, Lo), seg=i64(B, Lo), pos=i64(B, Lo), mask=i64(B, Lo, Lo), mpos=i64(B, T), labels=i64(B, T),
                                      logp=torch.empty(B, T, device=dev, dtype=torch.float32))
        am = attention_mask[:, :out_len, :out_len].to(torch.long).contiguous()
        tt = token_type_ids[:, :out_len].to(torch.long).contiguous()
        pid = position_ids[:, :out_len].to(torch.long).contiguous()
        sw["labels"].copy_(ids)
        K.scst_layout(input_ids.to(torch.long).contiguous(), sw["labels"], tt, pid, am, sw["ids"], sw["seg"], sw["pos"], sw["mask"], sw["mpos"],
                      mask_word_id)
        st = self.forward(vis_feats, vis_pe, sw["ids"], sw["seg"], sw["mask"], sw["mpos"], True, True, False, position_ids=sw["pos"],
                          dropout=False, dense=True)
        st.task_labels = sw["labels"].view(-1)
        return st, sw, B, T, V

    # ------------------------------------------------------------------------------------------
    # backward
    # ------------------------------------------------------------------------------------------
    def _tn_splits(self, a, b, c, M, N, Kd, ws):
        if self.TN_SPLITS is not None:
            return (self.GEMM_TN_VARIANT, self.TN_SPLITS)
        key = (M, N, Kd)
        sp = Engine._tn_choice.get(key)
        if sp is not None:
            return sp
        if not tuning.AUTOTUNE:
            sp = Engine._tn_choice[key] = tuning.tn_choice(M, N, Kd)
            return sp
        best = (self.GEMM_TN_VARIANT, 0)
        if M >= 1024:
            cands = [(var, sp) for var in self.TN_VARIANT_CANDIDATES for sp in tuning.TN_SPLIT_CANDIDATES if not (sp > 1 and M // sp < 128)]
            torch.cuda.synchronize()
            scratch = torch.empty(N, Kd, device=c.device, dtype=torch.float16)   # never time into the live gradient buffer
            best = tuning.best_of(cands, lambda vs, i: K.gemm_tn(a, b, scratch, M, N, Kd, beta=0, workspace=ws["tn_ws"], variant=vs[0], splits=vs[1]),
                                  rounds=2, reps=3)
        Engine._tn_choice[key] = best
        tuning.remember("tn", M, N, Kd, best)
        return best

    def _tn(self, a, b, c, M, N, Kd, ws, beta, bias=None, ws_key="tn_ws", **kw):
        """wgrad GEMM; `bias` (the Linear's bias gradient = column sums of dY) is fused into the same launch.  ws_key: the split-M scratch
        (launches on the side stream share "tn_ws"; the one TN launch of the main stream's head dgrad has its own)."""
        var, sp = self._tn_splits(a, b, c, M, N, Kd, ws)
        K.gemm_tn(a, b, c, M, N, Kd, beta=beta, workspace=ws[ws_key], variant=var, bias_out=bias, splits=sp, **kw)

    @property
    def last_live_rows(self):
        """Length of the row list the latest backward ran the last layer over (the distinct masked rows), or None when every row was
        walked.  The length lives on the device (no host read-back inside the step): reading this property synchronises."""
        return None if self._live_n is None else int(self._live_n.item())

    def _bucket_done(self, idx):
        if self.grad_ready_hook is not None:
            self.grad_ready_hook(idx)

    def backward(self, st, gscale, task, g_pretext=None, g_rows=None, h_rows=None):
        """gscale: device f32 tensor [1] = upstream gradient of the task loss (x loss scale); g_pretext: the same for the pretext loss of
        a mask_image_regions forward.  task="logprob" (a score_samples forward): g_rows = device f32 [B*T], the upstream gradient of every
        sampled token's log-probability (x loss scale) in place of the masked-LM loss; h_rows (optional, a score_samples(entropy=True)
        forward): the same for every position's entropy.  A forward scored with a temperature or an entropy runs vlp_token_policy_bwd, any
        other vlp_token_logprob_bwd.  Writes every parameter gradient into the flat gradient buffers."""
        c = _Backward(self, st, task)
        self._bwd_prologue(c)
        self._bwd_live_rows(c, task)
        head_wgrads = self._bwd_head(c, task, gscale, g_rows, h_rows)
        self._bwd_pretext(c, g_pretext)
        self._bwd_head_wgrads(c, head_wgrads)
        self._bwd_layers(c)
        self._bwd_embeddings(c)
        self._bwd_regions(c)
        self._bwd_finish(c)

    def _bwd_prologue(self, c):
        """Refusals, then what every backward starts from: final parameters, this step's W^T shadows, a cleared dx and cleared += tables."""
        if c.st.gen != self.gen:
            raise RuntimeError("vlp_amd: the activations of this forward were overwritten by a later forward "
                               "(one in-flight forward per model; run backward before the next forward)")
        if c.beta and self.shard_plan is not None:
            raise RuntimeError("vlp_amd: VLP_DDP_MODE=sharded keeps only this rank's chunk of the reduced gradient, so gradients cannot be "
                               "accumulated over several backward passes (--gradient_accumulation_steps > 1); use allreduce or rs_ag")
        self.wait_params()           # the optimizer stream has read the previous gradients and written every parameter
        if self._shadow_ev is not None:
            torch.cuda.current_stream().wait_event(self._shadow_ev)     # transposed during the forward (side stream)
            self._shadow_ev = None
        else:
            self._refresh_shadows()
        c.sh = self._shadows()
        c.ws["dx"].zero_()
        if c.beta == 0:
            # tables that are only ever accumulated into (+=) start from zero
            self.G("bert.embeddings.position_embeddings.weight").zero_()
            self.G("bert.embeddings.token_type_embeddings.weight").zero_()
        if c.use_side:
            self._side_busy = True

    def _bwd_live_rows(self, c, task):
        """The gradient that enters the encoder is zero outside the masked rows, and LayerNorm backward and the dgrad GEMMs keep a zero row
        zero: until attention mixes rows, the last layer's backward runs over the list of masked rows only (VLP_LAST_LAYER_LIVE=0: over all
        rows, as every other layer).  Heads whose gradient reaches other rows (vqa2, pretext, per-token log-probabilities) keep the full path."""
        st, ws = c.st, c.ws
        if (task != "vqa2" and task != "logprob" and st.has_mlm and st.P > 0 and st.pretext is None
                and os.environ.get("VLP_LAST_LAYER_LIVE", "1") != "0"):
            c.live, c.R = ws["lv_rows"], st.B * st.P

            def prologue():
                # the list and the two cleared full-size buffers the dense kernels of the last layer read (dctx: attention backward; dpre1: the
                # residual of the QKV dgrad).  None of it depends on the head's gradient: it runs beside the head chain
                K.live_rows_build(st.batch[3].contiguous(), st.B, st.P, st.L, c.live, ws["lv_n"], row_off=c.ro)
                ws["dctx"][:c.M].zero_()
                ws["dyset"][(c.NL - 1) & 1]["dpre1"][:c.M].zero_()
            c.on_side(prologue)
            if c.use_side:
                c.live_ready = torch.cuda.Event()
                c.live_ready.record(c.side)
        self._live_n = ws["lv_n"] if c.live is not None else None

    def _bwd_head(self, c, task, gscale, g_rows, h_rows):
        """The task head down to dx (the gradient entering the last encoder layer).  Returns its weight gradients as callables: they are
        issued on the side stream once the head's dgrad chain and the pretext branch are on the main stream (_bwd_head_wgrads)."""
        st, ws, sh, beta, ro, H, V, Nv = c.st, c.ws, c.sh, c.beta, c.ro, c.H, c.V, c.Nv
        B, L, P, masked_pos = st.B, st.L, st.P, st.batch[3]
        x_last, dx = ws["layers"][c.NL - 1]["x2"], ws["dx"]
        E, C = "bert.embeddings.", "cls.predictions."
        head_wgrads = []
        if task == "vqa2":
            NA, NAp = self._model().num_answers, ws["NAp"]
            if isinstance(st.task_labels, SparseAnswers):
                K.bce_sparse_loss_bwd(ws["vq_logits"], NAp, st.task_labels.idx, st.task_labels.score, B, NA, gscale, ws["vq_dlogits"], NAp)
            else:
                K.bce_loss_bwd(ws["vq_logits"], NAp, st.task_labels, st.task_labels.stride(0), B, NA, gscale, ws["vq_dlogits"], NAp)
            self._tn(ws["vq_dlogits"], ws["vq_a1"], self.G("ans_classifier.2.weight"), B, NA, 2 * H, ws, beta, bias=self.G("ans_classifier.2.bias"))
            self._nt(ws["vq_dlogits"], sh["a2T"], ws["vq_dz1"], B, 2 * H, NAp, mul_src=ws["vq_a1"], mul_mode=K.MUL_RELU_MASK)
            self._tn(ws["vq_dz1"], ws["vq_e"], self.G("ans_classifier.0.weight"), B, 2 * H, H, ws, beta, bias=self.G("ans_classifier.0.bias"))
            self._nt(ws["vq_dz1"], sh["a0T"], ws["vq_de"], B, H, 2 * H)
            K.vqa_mul_bwd(x_last, ws["vq_de"], dx, B, L, Nv, H, row_off=ro)
            if beta == 0:
                self.G(E + "word_embeddings.weight").zero_()     # no tied-decoder wgrad in this task: scatter needs zeros
        elif not st.has_mlm:
            if beta == 0:                                        # empty masked_pos (modeling.py:1096-1098): only the pretext loss is live
                self.G(E + "word_embeddings.weight").zero_()
                for n in ("bias", "transform.dense.weight", "transform.dense.bias", "transform.LayerNorm.weight", "transform.LayerNorm.bias"):
                    self.G(C + n).zero_()
        else:
            R, Vp = B * P, ws["Vp"]
            if task == "logprob":
                if g_rows is None or g_rows.numel() != R:
                    raise RuntimeError("vlp_amd: backward(task='logprob') needs g_rows with %d elements" % R)
                if h_rows is not None and (st.policy is None or st.policy[1] is None or h_rows.numel() != R):
                    raise RuntimeError("vlp_amd: backward(task='logprob', h_rows=...) needs a score_samples(entropy=True) forward and %d elements" % R)
                if st.policy is None or (st.policy[0] == 1.0 and h_rows is None):
                    K.token_logprob_bwd(ws["logits"], Vp, st.task_labels, ws["lse_ce"], g_rows, ws["dlogits"], Vp, R, V)
                else:
                    K.token_policy_bwd(ws["logits"], Vp, st.task_labels, ws["lse_ce"], g_rows, ws["dlogits"], Vp, R, V, temperature=st.policy[0],
                                       h=h_rows, entropy=None if h_rows is None else st.policy[1].view(-1))
            elif st.mlm_smooth is None:
                K.mlm_loss_bwd(ws["logits"], Vp, st.task_labels, ws["lse_ce"], ws["coef"], gscale, ws["dlogits"], Vp, R, V)
            else:
                K.mlm_loss_ls_bwd(ws["logits"], Vp, st.task_labels, ws["lse_ce"], ws["coef"], gscale, ws["dlogits"], Vp, R, V, *st.mlm_smooth)
            # tied decoder (modeling.py:445-448): dE[V,H] = dlogits^T . t ; the embedding scatter adds to it later
            head_wgrads.append(lambda: self._tn(ws["dlogits"], ws["tln"], self.G(E + "word_embeddings.weight"), R, V, H, ws, beta, bias=self.G(C + "bias")))
            # dgrad through the tied decoder: dt[R,H] = dlogits[R,V] . E[V,H].  As an NT GEMM this is 12 workgroups walking
            # K = 29056; instead transpose dlogits (11 MB) and contract over the vocabulary rows with the split-M wgrad kernel,
            # reading E in place (no E^T shadow).
            Rp = _ru(R, 64)
            K.transpose(ws["dlogits"], Vp, ws["dlT"], Rp, R, Vp, Rp)
            self._tn(ws["dlT"], self.P(E + "word_embeddings.weight"), ws["dtln"], V, R, H, ws, 0, ws_key="tn_ws_main")
            K.layernorm_bwd(ws["dtln"], ws["tg"], self.P(C + "transform.LayerNorm.weight"), ws["tstat"][0], ws["tstat"][1], ws["dtg"],
                            self.G(C + "transform.LayerNorm.weight"), self.G(C + "transform.LayerNorm.bias"), R, H, ws["ln_ws"], beta=beta)
            K.gelu_bwd(ws["dtg"], ws["tz"], ws["dtz"], R * H)
            head_wgrads.append(lambda: self._tn(ws["dtz"], ws["sel"], self.G(C + "transform.dense.weight"), R, H, H, ws, beta, bias=self.G(C + "transform.dense.bias")))
            self._nt(ws["dtz"], sh["tT"], ws["dsel"], R, H, H)
            K.scatter_add_rows(ws["dsel"], H, masked_pos.contiguous(), dx, H, B, P, L, H, row_off=ro)
        return head_wgrads

    def _bwd_pretext(self, c, g_pretext):
        """vis_pretext_loss backward (modeling.py:1113-1131): masked rows of d_vis_h / d_vispe_h (embed_bwd leaves them alone), then the
        pooler: tanh' is applied by the kernel, dW = d^T . h[:, 0], dh[:, 0] += d . W.  Without the branch: the pooler's gradient buffer."""
        st, ws, beta, H, Nv = c.st, c.ws, c.beta, c.H, c.Nv
        if st.pretext is not None:
            ptw, vmp = st.pretext
            if g_pretext is None:
                g_pretext = torch.zeros(1, device=self.device, dtype=torch.float32)
            K.pretext_bwd(ws["vis_h"], ws["vispe_h"], ptw["pooled"], vmp, ptw["probs"], g_pretext, ws["d_vis_h"], ws["d_vispe_h"], ptw["dpool"],
                          st.B, Nv, vmp.shape[1], H, drop_p=c.p, seed=c.seed, vis_stream=1001, vispe_stream=1002)
            self._tn(ptw["dpool"], ptw["sel0"], self.G("bert.pooler.dense.weight"), st.B, H, H, ws, beta, bias=self.G("bert.pooler.dense.bias"))
            K.transpose(self.P("bert.pooler.dense.weight"), H, ptw["pT"], H, H, H, H)
            self._nt(ptw["dpool"], ptw["pT"], ptw["dsel0"], st.B, H, H)
            K.scatter_add_rows(ptw["dsel0"], H, ptw["pos0"], ws["dx"], H, st.B, 1, st.L, H, row_off=c.ro)
            self._pooler_dirty = True
        elif beta == 0 and self._pooler_dirty:
            self.G("bert.pooler.dense.weight").zero_()           # a previous pretext step left gradients there; unused now
            self.G("bert.pooler.dense.bias").zero_()
            self._pooler_dirty = False                           # (an accumulating backward without the branch leaves buffer and flag as they are)

    def _bwd_head_wgrads(self, c, head_wgrads):
        """The head's deferred weight gradients on the side stream, then the hand-off of the head's gradient slice."""
        def tail():
            for fn in head_wgrads:
                fn()
            self._bucket_done(0)
        c.on_side(tail)          # (the side stream is ordered behind everything the main stream has issued so far)

    def _bwd_layers(self, c):
        """Encoder layers, last to first.  The dgrad chain (LN-bwd -> dgrad GEMMs -> attention-bwd) is the critical path; the four
        weight-gradient GEMMs of a layer only consume its dY tensors.  They are issued on a side stream (ordered after their producers by
        wait_stream) so that they co-run with the next kernels of the chain; dY buffers alternate by layer parity and the main stream waits
        for the side stream's event before it reuses a set."""
        self.last_wgrad_mapped = c.kept is not None
        for i in reversed(range(c.NL)):
            if c.use_side and self._side_done[i & 1] is not None:
                c.main.wait_event(self._side_done[i & 1])       # wgrads of layer i+2 have finished reading this set
            listed = c.live is not None and i == c.NL - 1
            if listed and c.live_ready is not None:
                c.main.wait_event(c.live_ready)
            self._bwd_layer(c, i, listed)
        if c.use_side and not c.grouped:
            c.main.wait_stream(c.side)      # all layer wgrads (and their bucket hand-offs) precede the rest of backward (split-M wgrads share tn_ws)
            self._side_busy = False
        # (grouped wgrads: the main stream does NOT wait here -- layer 0's weight gradients (170 us, issued a moment ago) and the
        # embedding tables run on the side stream underneath the embedding / region-projection backward, which touches none of their
        # operands; the streams join once, at the end of backward)

    def _bwd_layer(self, c, i, listed):
        """Backward of encoder layer i (modeling.py:268-372, bottom up).  listed: only the rows in c.live (device int32 [R], ascending, -1
        padded) carry gradient into it -- the two LayerNorm backwards, the FFN and attention-output dgrads and their three weight gradients
        walk the list and read the saved activations in place at row live[m]; the gradients between them are compact [R, *].  Attention
        backward and the QKV dgrad / wgrad stay dense either way: with a list they read dctx and the dpre1 residual, which hold exact zeros
        outside the listed rows (cleared by _bwd_live_rows)."""
        st, ws, beta, M, p, H, I = c.st, c.ws, c.beta, c.M, c.p, c.H, c.I
        a, s, (w, g), ds = ws["layers"][i], c.sh["layers"][i], self._layers()[i], ws["dyset"][i & 1]
        x_in = ws["layers"][i - 1]["x2"] if i > 0 else ws["x0"]
        dx, dctx, dpre1, dqkv = ws["dx"], ws["dctx"], ds["dpre1"], ds["dqkv"]
        # the gradients between the kernels: compact [R, *] beside the list, else the dY set's [M, *] (dx1, the gradient of x1: dx itself)
        if listed:
            live, R = c.live, c.R
            dpre2, dpre2_d, dz, dx1, dpre1_d = ws["lv_dpre2"], ws["lv_dpre2_d"], ws["lv_dz"], ws["lv_dx1"], ws["lv_dpre1_d"]
        else:
            live, R = None, M
            dpre2, dpre2_d, dz, dx1, dpre1_d = ds["dpre2"], ds["dpre2_d"], ds["dz"], dx, ds["dpre1_d"]
        dy2 = dpre2_d if p > 0 else dpre2
        # (dy1 of a list without dropout is the undropped dpre1 at its rows of the cleared full buffer: addressed through the list)
        dy1, dy1_fl = (dpre1_d, 0) if p > 0 else (dpre1, K.ROWS_X)
        # the layer's four weight gradients (dY, X, dW, rows, N, K, beta, dbias); the packed [3H, H] QKV gradient is always dense
        wg = [(dy2, a["g"], g.fc2_w, R, H, I, beta, g.fc2_b),
              (dz, a["x1"], g.fc1_w, R, I, H, beta, g.fc1_b),
              (dqkv, x_in, g.qkv_w, M, 3 * H, H, beta, g.qkv_b),
              (dy1, a["ctx"], g.o_w, R, H, H, beta, g.o_b)]
        split = not c.grouped and not listed       # split-M launches, each right behind the kernel that wrote its dY

        def tn(t):
            self._tn(*t[:6], ws, t[6], bias=t[7])
        # BertOutput: LN(dropout(dense(g)) + x1) (modeling.py:353-357); dG * gelu'(z) (stored by the forward); BertIntermediate (:340-343)
        # + the residual path of LN2's input; BertSelfOutput: LN(dropout(dense(ctx)) + x) (:313-317)
        ln2 = dict(dx_drop=dpre2_d if p > 0 else None, out_drop=(p, c.seed, 16 * i + 3), beta=beta, defer_reduce=True, row_map=c.rm)
        ln1 = dict(dx_drop=dpre1_d if p > 0 else None, out_drop=(p, c.seed, 16 * i + 2), beta=beta, defer_reduce=True, row_map=c.rm)
        if listed:
            K.layernorm_bwd_rows(dx, a["pre2"], w.ln2_w, *a["st2"], dpre2, g.ln2_w, g.ln2_b, live, K.ROWS_X, R, H, c.ln_slot(2 * i + 1), M, **ln2)
            K.gemm_nt_rows(dy2, s["w2T"], dz, live, K.ROWS_MUL, R, I, H, mul_src=a["z"], mul_mode=K.MUL_PLAIN)
            K.gemm_nt_rows(dz, s["w1T"], dx1, live, 0, R, H, I, residual=dpre2)
            K.layernorm_bwd_rows(dx1, a["pre1"], w.ln1_w, *a["st1"], dpre1, g.ln1_w, g.ln1_b, live, K.ROWS_Y, R, H, c.ln_slot(2 * i), M, **ln1)
            K.gemm_nt_rows(dy1, s["oT"], dctx, live, dy1_fl | K.ROWS_Y, R, H, H)
        else:
            K.layernorm_bwd(dx, a["pre2"], w.ln2_w, *a["st2"], dpre2, g.ln2_w, g.ln2_b, M, H, c.ln_slot(2 * i + 1), **ln2)
            if split:
                c.on_side(lambda: tn(wg[0]))
            self._nt(dy2, s["w2T"], dz, M, I, H, mul_src=a["z"], mul_mode=K.MUL_PLAIN)
            if split:
                c.on_side(lambda: tn(wg[1]))
            self._nt(dz, s["w1T"], dx1, M, H, I, residual=dpre2)
            K.layernorm_bwd(dx1, a["pre1"], w.ln1_w, *a["st1"], dpre1, g.ln1_w, g.ln1_b, M, H, c.ln_slot(2 * i), **ln1)
            if split:
                c.on_side(lambda: tn(wg[3]))
            self._nt(dy1, s["oT"], dctx, M, H, H)
        # BertSelfAttention (modeling.py:268-303)
        K.attn_bwd(a["qkv"], ws["maskb"], ws["maskt"], a["ctx"], dctx, a["lse"], dqkv, ws["delta"], st.B, st.L, c.A, c.scale, dropout_p=c.pa,
                   seed=c.seed, rng_stream=16 * i + 1, row_off=c.ro)

        def wgrads():           # what is left of the layer's weight gradients, behind its attention backward
            if listed:
                # three walks of the list and the dense QKV problem (in one launch with enough rows, QKV third as in every grouped launch)
                rows = [wg[0] + (live, 0), wg[1] + (live, 0), wg[3] + (live, dy1_fl)]
                K.gemm_tn_grouped_rows(rows[:2] + [wg[2] + (None, 0)] + rows[2:] if c.grouped else rows)
            elif c.kept is not None:
                # dense step: rows past a sample's kept length have dY == 0 in all four problems; the walk skips them (device map)
                K.gemm_tn_grouped_mapped(wg, c.kept[0], c.kept[1])
            elif c.grouped:
                # ONE grid of 36 + 108 + 144 + 144 output tiles, every workgroup walking the whole contraction: no split-M slabs, no
                # reduce launches (csrc/gemm_tn.hip)
                K.gemm_tn_grouped(wg)
            if not c.grouped:
                tn(wg[2])       # split-M (the other three: in the listed launch above, or issued beside the dgrads)
            c.wgrads_issued(i)
        c.on_side(wgrads)
        self._nt(dqkv, s["qkvT"], dx, M, H, 3 * H, residual=dpre1)

    def _embed_bwd(self, c, dpre, parts):
        """parts = 1: the region rows (d_vis_h / d_vispe_h; they do not depend on position ids), 2: the three embedding tables."""
        st, ws, E = c.st, c.ws, "bert.embeddings."
        pt, (_, input_ids, token_type_ids, _) = st.pretext, st.batch
        args = (ws["vis_h"], ws["vispe_h"], self.G(E + "word_embeddings.weight"), self.G(E + "position_embeddings.weight"),
                self.G(E + "token_type_embeddings.weight"), ws["d_vis_h"], ws["d_vispe_h"], ws["acc32"], st.B, st.L, c.Nv,
                c.H, c.V, self._model().config.type_vocab_size)
        kw = dict(drop_p=c.p, seed=c.seed, vis_stream=1001, vispe_stream=1002, region_mask=pt[0]["rmask"] if pt is not None else None, parts=parts)
        if parts == 2 and st.pos_ids is not None:       # explicit position ids (score_samples): the position table follows them
            K.embed_bwd_pos(dpre, input_ids, token_type_ids, st.pos_ids, *args, **kw)
        else:
            K.embed_bwd(dpre, input_ids, token_type_ids, *args, **kw)

    def _bwd_embeddings(self, c):
        """Embedding LayerNorm and the region rows on the main stream; the tables and every LayerNorm's parameter sums on the side stream."""
        ws, beta, M, rm, NL, H, E = c.ws, c.beta, c.M, c.rm, c.NL, c.H, "bert.embeddings."
        dpre = ws["dpre"]
        K.layernorm_bwd(ws["dx"], ws["emb_pre"], self.P(E + "LayerNorm.weight"), ws["stat0"][0], ws["stat0"][1], dpre,
                        self.G(E + "LayerNorm.weight"), self.G(E + "LayerNorm.bias"), M, H, c.ln_slot(2 * NL), beta=beta, dy_drop=(c.p, c.seed, 1000),
                        defer_reduce=True, row_map=rm)
        if rm is not None:
            # the embedding backward sums over (batch, position) in the dense [B, L] geometry (position table: a column of the batch;
            # word table: id chains in row order): hand it the dense gradient -- exact zeros on the dropped positions, as in the dense run
            dense = ws["dx_alt"]
            dense.zero_()
            K.rows_unpack(dpre, rm, M, dense, H)
            dpre = dense

        def tables_and_ln_params():
            # the tail of backward that nothing on the main stream waits for: dgamma / dbeta of the 2 * layers + 1 LayerNorms (one launch,
            # slot order = table order) and the three embedding tables (five launches); their gradient slice is announced from here
            K.layernorm_bwd_reduce_batched(ws["ln_slots"], self._ln_table(), 2 * NL + 1, M, H, beta=beta)
            self._embed_bwd(c, dpre, 2)
            self._bucket_done(NL + 1)           # position / type / word embedding tables (tied decoder wgrad + embedding backward) are final

        # region rows first (the region-projection dgrad / wgrads wait for d_vis_h / d_vispe_h only); the tables and the LayerNorm
        # parameter sums run on the side stream underneath them (round 5: six small launches, ~140 us, off the critical path)
        self._embed_bwd(c, dpre, 1)
        if c.use_side:
            self._side_busy = True
        c.on_side(tables_and_ln_params)

    def _bwd_regions(self, c):
        """Region projections.  vis_pe_embed: Linear(1607, H) -- wgrad into the padded shadow, then crop-accumulate; vis_embed:
        Linear(2048,2048)+ReLU -> Linear(2048,H)+ReLU+Dropout."""
        ws, beta, Mv, H, img = c.ws, c.beta, c.Mv, c.H, c.st.batch[0]
        self._nt(ws["d_vis_h"], c.sh["v2T"], ws["dz1v"], Mv, 2048, H, mul_src=ws["h1"], mul_mode=K.MUL_RELU_MASK)
        if c.grouped and Mv >= 2048:
            # the three region-projection wgrads (78 + 96 + 256 output tiles, contraction over B x 100 region rows) as one grouped launch
            K.gemm_tn_grouped([
                (ws["dz1v"], img, self.G("vis_embed.0.weight"), Mv, 2048, 2048, beta, self.G("vis_embed.0.bias")),
                (ws["d_vis_h"], ws["h1"], self.G("vis_embed.2.weight"), Mv, H, 2048, beta, self.G("vis_embed.2.bias")),
                (ws["d_vispe_h"], ws["vpe_in"], ws["dwpe_pad"], Mv, H, PE_PAD, 0, None)])
        else:
            if c.use_side and self._side_busy:
                # these split-M launches use ws["tn_ws"] on the MAIN stream; the head wgrads deferred to the side stream use the same scratch and
                # with <= 2 layers no per-layer wait orders the two: join first (small batches only -- Mv < 2048)
                c.main.wait_stream(c.side)
            self._tn(ws["d_vispe_h"], ws["vpe_in"], ws["dwpe_pad"], Mv, H, PE_PAD, ws, 0)
            self._tn(ws["d_vis_h"], ws["h1"], self.G("vis_embed.2.weight"), Mv, H, 2048, ws, beta, bias=self.G("vis_embed.2.bias"))
            self._tn(ws["dz1v"], img, self.G("vis_embed.0.weight"), Mv, 2048, 2048, ws, beta, bias=self.G("vis_embed.0.bias"))
        K.copy2d(ws["dwpe_pad"], PE_PAD, False, self.G("vis_pe_embed.0.weight"), PE_DIM, H, PE_DIM, PE_DIM, beta=beta)
        K.colsum(ws["d_vispe_h"], self.G("vis_pe_embed.0.bias"), Mv, H, beta=beta, workspace=ws["cs_ws"])

    def _bwd_finish(self, c):
        """Join the streams, hand off the last gradient slice, mark the gradients as written."""
        if c.use_side and self._side_busy:
            # the streams join HERE, in front of the last hand-off: a reducer may coalesce the embedding tables (written on the side stream)
            # with the region projections into one bucket, and that bucket's collective is ordered behind the stream that announces it
            c.main.wait_stream(c.side)
            self._side_busy = False
        self._bucket_done(c.NL + 2)
        self.grads_dirty = True
        if self.post_backward_hook is not None:
            self.post_backward_hook()
