"""Incremental caption decoding with a K/V cache on the HIP engine (modeling.py:1189-1253, :856-875, :386-394): the base class of
vlp_amd.engine.Engine that holds the decode workspaces, the token step, its capture / replay, and the three decoders (greedy, K samples
per image, beam search).  The three are one program: `_decode_begin` is the call setup, `_decode_steps` the token-step loop; a decoder
adds its limits, its selection launches, its caches and its plan key.

Every kernel is called as K.<name>(...) through the vlp_amd._lib module object at call time.  Parameters, region inputs, the NT GEMM
dispatch and the training forward stay in engine.py and are reached through `self`."""
import collections
import math
import os

import numpy as np
import torch

from . import _lib as K
from . import tuning
from ._common import PE_PAD, VlpPerformanceWarning, _ru


def sample_major(t, B, Ks, n):
    """Rows of a grouped sampled decode, [B*Ks, >= n] with row b*Ks + k, as a NEW [Ks*B, n] tensor with row k*B + b: one permuted copy
    for every Ks.  (At Ks == 1 the permutation is the identity, and a reshape alone would hand the caller the workspace's own rows.)"""
    return t[:, :n].view(B, Ks, n).transpose(0, 1).clone(memory_format=torch.contiguous_format).view(Ks * B, n)


# One decode call after _decode_begin.  R = sequences decoded in parallel from step 1 on; T0 = rows of step 0 (prefix + [MASK]);
# am = the workspace's static copy of the mask (what the token steps s >= 1 read: call-invariant launch arguments); attention_mask =
# the caller's, int64 with a unit last stride (what step 0 reads); token_type_ids / position_ids = the caller's as int64.
_Call = collections.namedtuple("_Call", "ws B R in_len out_len n_steps T0 V am token_type_ids position_ids attention_mask x_first")


class Decoder(object):
    def _decode_workspace(self, B, T0, Lcap, Kb=1, group=False):
        """group: Kb samples per image that never permute (decode_sample_group) instead of Kb beams."""
        key = ("dec", B, T0, Lcap, Kb) + (("group",) if group else ())
        ws = self._ws.get(key)
        if ws is not None:
            return ws
        model = self._model()
        cfg = model.config
        H, I, NL, Nv, V = cfg.hidden_size, cfg.intermediate_size, cfg.num_hidden_layers, model.len_vis_input, cfg.vocab_size
        R = B * Kb                                    # sequences decoded in parallel after the first step
        M, Mv, dev = max(B * T0, R * 2), B * Nv, self.device

        def h(*s):
            return torch.empty(*s, device=dev, dtype=torch.float16)

        def f(*s):
            return torch.empty(*s, device=dev, dtype=torch.float32)

        def i64(*s):
            return torch.empty(*s, device=dev, dtype=torch.long)

        Vp = _ru(V, 64)
        ws = dict(Vp=Vp, maskb=torch.empty(max(B * T0, R * 2) * _ru(Lcap, 32), device=dev, dtype=torch.uint8),
                  img16=h(Mv, 2048), vpe_in=h(Mv, PE_PAD), wpe_pad=h(H, PE_PAD), h1=h(Mv, 2048), vis_h=h(Mv, H), vispe_h=h(Mv, H),
                  emb_pre=h(M, H), xa=h(M, H), xb=h(M, H), qkv=h(M, 3 * H), ctx=h(M, H), pre=h(M, H), x1=h(M, H), g=h(M, I),
                  kv=[h(B, Lcap, 2 * H) for _ in range(NL)],        # per layer: K | V of every position decoded so far
                  sel=h(R, H), tg=h(R, H), tln=h(R, H), logits=h(R, Vp), xids=i64(R, 2),
                  last_first=torch.full((R, 1), T0 - 1, device=dev, dtype=torch.long), last_step=torch.full((R, 1), 1, device=dev, dtype=torch.long),
                  # static copies of the caller's per-position inputs, so that the launches of a token step have call-invariant arguments
                  mask_static=i64(R, Lcap, Lcap), tt_steps=i64(Lcap, R, 2), pid_steps=i64(Lcap, R, 2),
                  out_ids=i64(B, Lcap), out_val=f(B, Lcap), plans={}, calls=0, plan_stream=None, plans_aside={},
                  slab=f(self.DEC_SPLITS, R * 2, H),      # fp32 split-K partial sums of the token-step out-projection / FFN-down (vlp_dec_gemm -> vlp_dec_reduce_ln)
                  sk_ws=torch.empty(K.gemm_nt_splitk_workspace_bytes(min(M, 1024), max(I, 3 * H), max(tuning.SKINNY_SPLITS)), device=dev,
                                    dtype=torch.uint8))
        if group:
            # one cache per row for the generated positions (the prefix stays in `kv`, once per image), the outputs of all R rows, and the
            # device cell the sampling launches read their seed from (uint64 bits)
            ws.update(out_ids=i64(R, Lcap), out_val=f(R, Lcap), seed_cell=torch.zeros(1, device=dev, dtype=torch.long))
            if Kb > 1:
                ws.update(kvS=[h(R, Lcap, 2 * H) for _ in range(NL)])
        elif Kb > 1:
            # beams: two caches per layer (select_beam_items permutes rows: gather from one into the other, then swap)
            ws.update(kvA=[h(R, Lcap, 2 * H) for _ in range(NL)], kvB=[h(R, Lcap, 2 * H) for _ in range(NL)],
                      kk_s=f(R, Kb), kk_i=i64(R, Kb), src_rows=i64(R), tot=f(Lcap, B, Kb), wids=i64(Lcap, B, Kb), ptrs=i64(Lcap, B, Kb),
                      eos=f(Lcap, B, Kb),
                      # device n-gram blocking: per hypothesis the words that would repeat an n-gram (vlp_ngram_candidates -> vlp_logsoftmax_topk_list)
                      # (a hypothesis of frame s lists at most s + 1 <= Lcap - T0 + 1 words)
                      cand_ids=torch.empty(R, Lcap - T0 + 1, device=dev, dtype=torch.int32), cand_cnt=torch.empty(R, device=dev, dtype=torch.int32),
                      ngram_ignore={})
        self._ws[key] = ws
        return ws

    def _decode_check(self, vis_feats, vis_pe, input_ids, token_type_ids, attention_mask):
        Nv = self._model().len_vis_input
        B, in_len = input_ids.shape
        out_len = token_type_ids.shape[1]
        self._check_regions(vis_feats, vis_pe)
        if in_len < Nv + 2 or out_len <= in_len or out_len > 256:
            raise RuntimeError("vlp_amd: decode needs %d <= input length < output length <= 256 (got %d, %d)" % (Nv + 2, in_len, out_len))
        if attention_mask.dim() != 3 or attention_mask.shape[1] < out_len or attention_mask.shape[2] < out_len:
            raise RuntimeError("vlp_amd: decode expects a [B, L, L] attention mask covering the output length")
        return B, in_len, out_len

    def _decode_regions(self, ws, vis_feats, vis_pe):
        """Region projections, once per decode call (:1192-1193)."""
        model = self._model()
        H, Nv = model.config.hidden_size, model.len_vis_input
        Mv = vis_feats.shape[0] * Nv
        img, prep_pe = self._region_inputs(ws, vis_feats, vis_pe)
        prep_pe()           # (the decoders have waited for every parameter already: its wait_params orders nothing new)
        self._nt(img, self.P("vis_embed.0.weight"), ws["h1"], Mv, 2048, 2048, bias=self.P("vis_embed.0.bias"), act=K.ACT_RELU)
        self._nt(ws["h1"], self.P("vis_embed.2.weight"), ws["vis_h"], Mv, H, 2048, bias=self.P("vis_embed.2.bias"), act=K.ACT_RELU)
        self._nt(ws["vpe_in"], ws["wpe_pad"], ws["vispe_h"], Mv, H, PE_PAD, bias=self.P("vis_pe_embed.0.bias"), act=K.ACT_RELU)

    # Token steps on the burst kernels of csrc/decode.hip (round 6): 7 launches per layer instead of 12 (vlp_dec_gemm QKV with the K/V append
    # fused, attention, out-projection as 4 k slices, slab reduce + bias + residual + LayerNorm in one launch, FFN-up + GeLU, FFN-down as 4 k
    # slices, reduce + LayerNorm).  VLP_DECODE_FUSED=0: the round-2 path (split-K skinny GEMMs, separate reduces / kv_append / LayerNorms).
    DECODE_FUSED = os.environ.get("VLP_DECODE_FUSED", "1") == "1"
    DEC_SPLITS = 4

    def _decode_attn(self, ws, kv, i, maskb, R, T, Lk, Lcap, prefix):
        """Attention of the T new rows of R sequences over layer i's cache `kv` (and, under beam search, the per-sample prefix cache)."""
        cfg = self._model().config
        H, A = cfg.hidden_size, cfg.num_attention_heads
        kw = {}
        if prefix is not None:
            pk = prefix[0][i]
            kw = dict(k_prefix=pk, v_prefix=pk[:, :, H:], prefix_rows=Lcap, n_prefix=prefix[1], beams=prefix[2])
        K.attn_decode(ws["qkv"], 3 * H, T, kv, kv[:, :, H:], 2 * H, Lcap, maskb, ws["ctx"], R, T, Lk, A, 1.0 / math.sqrt(H // A), **kw)

    def _decode_layers_fused(self, ws, caches, Lcap, x, alt, maskb, R, T, st, prefix):
        """The 12 BertLayers of a token step (M = R * T <= a few hundred rows) on vlp_dec_gemm / vlp_dec_reduce_ln.  Same arithmetic and
        rounding points as the unfused path (fp16 GEMM outputs, fp16 pre-LayerNorm sums, fp32 LayerNorm statistics); only the fp32
        summation order of the contractions differs."""
        model = self._model()
        cfg = model.config
        H, I, NL = cfg.hidden_size, cfg.intermediate_size, cfg.num_hidden_layers
        Lk, M, S = st + T, R * T, self.DEC_SPLITS
        slab = ws["slab"].view(-1)[:S * M * H].view(S, M, H)        # slab s holds rows [s * M, (s + 1) * M)
        for i in range(NL):
            Ln = "bert.encoder.layer.%d." % i
            kv = caches[i]
            K.dec_gemm(x, self.P(Ln + "attention.self.query.weight"), M, 3 * H, H, y=ws["qkv"], bias=self.P(Ln + "attention.self.query.bias"),
                       kv_cache=kv, kv_col0=H, kv_Lcap=Lcap, kv_T=T, kv_start=st)
            self._decode_attn(ws, kv, i, maskb, R, T, Lk, Lcap, prefix)
            # (this LayerNorm as a prologue of the FFN-up launch, which vlp_dec_gemm can do, measured slower and is not used: 0.645 against
            # 0.559 ms per token step, profiles/r06_decode_ln_prologue_ab.txt)
            K.dec_gemm(ws["ctx"], self.P(Ln + "attention.output.dense.weight"), M, H, H, slab=slab, splits=S)
            K.dec_reduce_ln(slab, S, self.P(Ln + "attention.output.dense.bias"), x, self.P(Ln + "attention.output.LayerNorm.weight"),
                            self.P(Ln + "attention.output.LayerNorm.bias"), ws["x1"], M, H)
            K.dec_gemm(ws["x1"], self.P(Ln + "intermediate.dense.weight"), M, I, H, y=ws["g"], bias=self.P(Ln + "intermediate.dense.bias"), act=K.ACT_GELU)
            K.dec_gemm(ws["g"], self.P(Ln + "output.dense.weight"), M, H, I, slab=slab, splits=S)
            K.dec_reduce_ln(slab, S, self.P(Ln + "output.dense.bias"), ws["x1"], self.P(Ln + "output.LayerNorm.weight"),
                            self.P(Ln + "output.LayerNorm.bias"), alt, M, H)
            x, alt = alt, x
        return x

    def _decode_layers_unfused(self, ws, caches, Lcap, x, alt, maskb, R, T, st, prefix):
        """The same layers on the round-2 path (split-K skinny GEMMs, separate kv_append / LayerNorm launches): the first step of a decode
        call and every shape the fused kernels do not take."""
        cfg = self._model().config
        H, I, NL = cfg.hidden_size, cfg.intermediate_size, cfg.num_hidden_layers
        Lk, M = st + T, R * T

        def same_in_all_layers(suffix):
            return lambda: [self.P("bert.encoder.layer.%d.%s" % (j, suffix)) for j in range(NL)]

        def nt(xin, Ln, name, y, N, Kd, **kw):
            self._nt_skinny(xin, self.P(Ln + name + ".weight"), y, M, N, Kd, ws["sk_ws"], tune_ws=same_in_all_layers(name + ".weight"),
                            bias=self.P(Ln + name + ".bias"), **kw)

        for i in range(NL):
            Ln = "bert.encoder.layer.%d." % i
            kv = caches[i]
            nt(x, Ln, "attention.self.query", ws["qkv"], 3 * H, H)
            K.kv_append(ws["qkv"], 3 * H, kv, Lcap, R, T, st, H)
            self._decode_attn(ws, kv, i, maskb, R, T, Lk, Lcap, prefix)
            nt(ws["ctx"], Ln, "attention.output.dense", ws["pre"], H, H, residual=x)
            K.layernorm_fwd(ws["pre"], self.P(Ln + "attention.output.LayerNorm.weight"), self.P(Ln + "attention.output.LayerNorm.bias"),
                            ws["x1"], M, H)
            nt(ws["x1"], Ln, "intermediate.dense", ws["g"], I, H, act=K.ACT_GELU)
            nt(ws["g"], Ln, "output.dense", ws["pre"], H, I, residual=ws["x1"])
            K.layernorm_fwd(ws["pre"], self.P(Ln + "output.LayerNorm.weight"), self.P(Ln + "output.LayerNorm.bias"), alt, M, H)
            x, alt = alt, x
        return x

    def _decode_model_step(self, ws, caches, Lcap, xids, tt, pid, mask_view, R, T, st, first, prefix=None):
        """One incremental forward of R sequences x T new tokens at absolute positions st..st+T-1: Q/K/V projection of the new
        tokens, K|V appended to the per-layer caches, attention over positions 0..st+T-1, LM head on the last ([MASK]) slot.
        Leaves the logits [R, V] in ws['logits'] (pitch ws['Vp']).  prefix = (per-sample caches, n_prefix, beams): beam search keeps
        the positions < n_prefix (regions + [SEP], identical for all beams of a sample) once per sample; `caches` then hold only
        the generated positions of every beam."""
        model = self._model()
        cfg = model.config
        H, I, Nv, V = cfg.hidden_size, cfg.intermediate_size, model.len_vis_input, cfg.vocab_size
        E, C = "bert.embeddings.", "cls.predictions."
        Lk = st + T
        Lkp = _ru(Lk, 32)
        M = R * T
        maskb = ws["maskb"][:R * T * Lkp]
        K.mask_pack_rect(mask_view, maskb, R, T, Lk, Lkp)
        K.embed_fwd(xids, tt, self.P(E + "word_embeddings.weight"), self.P(E + "position_embeddings.weight"),
                    self.P(E + "token_type_embeddings.weight"), ws["vis_h"], ws["vispe_h"], ws["emb_pre"], R, T, Nv if first else 0, H,
                    position_ids=pid)
        x, alt = ws["xa"], ws["xb"]
        K.layernorm_fwd(ws["emb_pre"], self.P(E + "LayerNorm.weight"), self.P(E + "LayerNorm.bias"), x, M, H)
        fused = (self.DECODE_FUSED and not first and M <= 1024 and H % 256 == 0 and H <= 768 and I % (64 * self.DEC_SPLITS) == 0 and
                 I // self.DEC_SPLITS <= 768 and H % (64 * self.DEC_SPLITS) == 0)
        layers = self._decode_layers_fused if fused else self._decode_layers_unfused
        x = layers(ws, caches, Lcap, x, alt, maskb, R, T, st, prefix)
        # ---- LM head on the [MASK] slot (:1226-1228 / :1293-1296) ----------------------------------
        if fused:
            # the [MASK] slot is the LAST of the T new rows of every sequence: a strided view of x (row pitch T * H), no gather launch
            sel = x.view(-1)[:R * T * H].view(R, T * H)[:, (T - 1) * H:]
            K.dec_gemm(sel, self.P(C + "transform.dense.weight"), R, H, H, y=ws["tg"], bias=self.P(C + "transform.dense.bias"), act=K.ACT_GELU)
        else:
            K.gather_rows(x, H, ws["last_first"] if first else ws["last_step"], ws["sel"], H, R, 1, T, H)
            self._nt(ws["sel"], self.P(C + "transform.dense.weight"), ws["tg"], R, H, H, bias=self.P(C + "transform.dense.bias"), act=K.ACT_GELU)
        K.layernorm_fwd(ws["tg"], self.P(C + "transform.LayerNorm.weight"), self.P(C + "transform.LayerNorm.bias"), ws["tln"], R, H)
        if fused:
            K.dec_gemm(ws["tln"], self.P("bert.embeddings.word_embeddings.weight"), R, V, H, y=ws["logits"], bias=self.P(C + "bias"))
        else:
            self._nt(ws["tln"], self.P("bert.embeddings.word_embeddings.weight"), ws["logits"], R, V, H, bias=self.P(C + "bias"), ldy=ws["Vp"])

    def _decode_static_inputs(self, ws, token_type_ids, position_ids, attention_mask, in_len, out_len, rep):
        """Copies the caller's per-position inputs of the token steps s >= 1 into workspace buffers (one torch op each), so that the
        launches of those steps take the same arguments on every call (launch plans).  rep = beams per sample (first_expand)."""
        n = out_len - in_len - 1                     # steps 1 .. n_steps-1 use the position window (in_len+s-1, in_len+s)
        if n > 0:
            tt = token_type_ids.unfold(1, 2, 1)[:, in_len:in_len + n].transpose(0, 1)      # [n, B, 2]
            pid = position_ids.unfold(1, 2, 1)[:, in_len:in_len + n].transpose(0, 1)
            if rep > 1:
                tt, pid = tt.repeat_interleave(rep, dim=1), pid.repeat_interleave(rep, dim=1)
            ws["tt_steps"][1:n + 1].copy_(tt)
            ws["pid_steps"][1:n + 1].copy_(pid)
        am = attention_mask[:, :out_len, :out_len]
        ws["mask_static"].copy_(am.repeat_interleave(rep, dim=0) if rep > 1 else am)

    DECODE_GRAPHS = os.environ.get("VLP_DECODE_GRAPHS", "1") == "1"

    def _run_planned(self, ws, key, fn):
        """Token steps s >= 1 launch ~200 small kernels with call-invariant arguments; at ~4.5 us of HIP launch cost each the host, not
        the GPU, bounded decoding.  Call 1 of a workspace runs (and autotunes) normally; call 2 captures each step into a hipGraph
        (torch.cuda.CUDAGraph over the launches our C ABI puts on the capture stream) and replays it; later calls only replay.
        If capture is unavailable the recorded ctypes plan (no Python argument marshalling) is the fallback."""
        stream = torch.cuda.current_stream().cuda_stream
        if ws["plan_stream"] != stream:
            # the plans of a workspace belong to ONE stream (a recorded ctypes plan carries it in the arguments of every launch): on another
            # stream ALL of them are set aside, not only the one that meets the change, and they come back with their stream
            aside = ws["plans_aside"]
            if ws["plan_stream"] is not None:
                aside[ws["plan_stream"]] = ws["plans"]
            ws["plans"], ws["plan_stream"] = aside.pop(stream, {}), stream
        item = ws["plans"].get(key)
        if item is not None:
            if isinstance(item, list):
                K.replay(item)
            else:
                item.replay()
            return
        if ws["calls"] == 0:
            fn()
            return
        if self.DECODE_GRAPHS:
            try:
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    fn()
                g.replay()
                ws["plans"][key] = g
                return
            except Exception as e:               # capture not possible here: fall back to the ctypes plan (host-bound: say so, once)
                torch.cuda.synchronize()
                # off for the process, on the class whose attribute the decoders read (the subclass's, where somebody assigned it there)
                next(c for c in type(self).__mro__ if "DECODE_GRAPHS" in vars(c)).DECODE_GRAPHS = False
                import warnings
                warnings.warn("vlp_amd: hipGraph capture of a decoder token step failed (%r); token steps fall back to replayed ctypes launch plans, "
                              "which are bound by host launch overhead" % (e,), VlpPerformanceWarning)
        with K.record() as plan:
            fn()
        ws["plans"][key] = plan

    def _decode_begin(self, vis_feats, vis_pe, input_ids, token_type_ids, position_ids, attention_mask, mask_word_id, Kb=1, group=False):
        """The call setup of every decoder, once: parameters packed and waited for, the shape check, the workspace of (B, T0, Lcap, Kb),
        the region projections, the static copies the token steps s >= 1 read, the ids of step 0 (prefix + [MASK]) and the [MASK] slot of
        the token steps.  A decoder's own limits are checked in front of this call: a refused call leaves no workspace behind.
        The caller's mask is read as int64 with a unit last stride (vlp_mask_pack_rect takes a row pitch, not an element stride); step 0
        of every decoder reads that tensor, the steps after it read the workspace's copy."""
        self.pack()
        self.wait_params()
        B, in_len, out_len = self._decode_check(vis_feats, vis_pe, input_ids, token_type_ids, attention_mask)
        T0 = in_len + 1
        ws = self._decode_workspace(B, T0, out_len, Kb, group)
        attention_mask = attention_mask.to(torch.long)
        if attention_mask.stride(2) != 1:
            attention_mask = attention_mask.contiguous()
        token_type_ids, position_ids = token_type_ids.to(torch.long), position_ids.to(torch.long)
        self._decode_regions(ws, vis_feats, vis_pe)
        self._decode_static_inputs(ws, token_type_ids, position_ids, attention_mask, in_len, out_len, Kb)     # first_expand (:1361-1365)
        x_first = torch.cat((input_ids.to(torch.long), torch.full((B, 1), int(mask_word_id), device=self.device, dtype=torch.long)),
                            dim=1).contiguous()
        ws["xids"][:, 1] = int(mask_word_id)
        return _Call(ws, B, B * Kb, in_len, out_len, out_len - in_len, T0, self._model().config.vocab_size, ws["mask_static"],
                     token_type_ids, position_ids, attention_mask, x_first)

    def _decode_steps(self, call, select, caches, prefix, plan_key, between=None):
        """The token-step loop of every decoder.  Step 0 runs the B prefixes + [MASK] on the per-image cache ws["kv"]; step s >= 1 feeds
        the token that is new since step s-1 plus one [MASK] slot of R sequences at positions st, st+1 on `caches(s)` (with `prefix`, see
        _decode_model_step).  `select(s, first)` issues the decoder's launches behind the logits of step s; it runs inside the captured
        step.  `between(s)`, if given, runs on the host after step s, outside any capture.
        Run or plan: `plan_key(s)` is None for a step whose launches change from call to call (a seed or a fresh tensor among the
        arguments, a selection on the host) -- it is run -- and else the key under which step s is captured once and replayed
        (_run_planned).  The key carries everything that is baked into the step's launches beyond the workspace's shapes: the decoder
        kind, s, and every scalar or workspace tensor the decoder's `select` passes that another call on this workspace may pass
        differently.  Counts the call on the workspace at the end (call 1 runs, call 2 captures)."""
        c, ws = call, call.ws
        self._decode_model_step(ws, ws["kv"], c.out_len, c.x_first, c.token_type_ids[:, :c.T0].contiguous(),
                                c.position_ids[:, :c.T0].contiguous(), c.attention_mask[:, :c.T0, :c.T0], c.B, c.T0, 0, True)
        select(0, True)
        if between is not None:
            between(0)
        for s in range(1, c.n_steps):
            def step(s=s, st=c.in_len + s - 1, kv=caches(s)):           # (captured by a graph: everything it reads is bound here)
                self._decode_model_step(ws, kv, c.out_len, ws["xids"], ws["tt_steps"][s], ws["pid_steps"][s], c.am[:, st:st + 2, :st + 2],
                                        c.R, 2, st, False, prefix=prefix)
                select(s, False)
            key = plan_key(s)
            if key is None:
                step()
            else:
                self._run_planned(ws, key, step)
            if between is not None:
                between(s)
        ws["calls"] += 1

    def decode_greedy(self, vis_feats, vis_pe, input_ids, token_type_ids, position_ids, attention_mask, mask_word_id, sample=False):
        """Greedy incremental decoding.  Step s feeds the tokens that are new since step s-1 plus one [MASK] slot, projects them
        to Q/K/V, appends K|V to the per-layer cache at their absolute positions (the [MASK] slot's entry is overwritten by the
        real token in the next step, which is exactly what the reference's hidden-state history achieves by dropping the last
        row, :1236-1247) and attends over the cache.  Returns (ids [B, n] int64, max logits [B, n] f32); with sample=True the
        ids are drawn from softmax(logits) (:1229-1235) and the second output holds their log-probabilities."""
        c = self._decode_begin(vis_feats, vis_pe, input_ids, token_type_ids, position_ids, attention_mask, mask_word_id)
        ws, out_ids, out_val = c.ws, c.ws["out_ids"], c.ws["out_val"]

        def select(s, first):
            if sample:
                self.step_seed += 1
                for dst in (out_ids[:, s], ws["xids"][:, 0]):                   # same (seed, stream) -> same draw; 2nd = next input token
                    K.sample_rows(ws["logits"], ws["Vp"], c.B, c.V, self.base_seed + self.step_seed, 7001, dst, out_val[:, s])
            else:
                K.argmax_rows2(ws["logits"], ws["Vp"], c.B, c.V, out_ids[:, s], ws["xids"][:, 0], out_val[:, s])      # + next step's first input token

        # sampling: the seed is a launch argument and changes every step: not plannable (decode_sample_group reads it from a device cell
        # and is)
        self._decode_steps(c, select, lambda s: ws["kv"], None, lambda s: None if sample else ("greedy", s))
        return out_ids[:, :c.n_steps].clone(), out_val[:, :c.n_steps].clone()

    def decode_sample_group(self, vis_feats, vis_pe, input_ids, token_type_ids, position_ids, attention_mask, mask_word_id, n_samples,
                            temperature=1.0, top_k=0, top_p=1.0):
        """K = n_samples sampled captions per image (self-critical training with a leave-one-out baseline).  Step 0 runs the B prefixes as in
        decode_beam and draws K first tokens from each of the B logits rows; steps s >= 1 decode R = B*K rows against the per-image prefix
        cache, each row with a cache of its own for the generated positions -- rows never permute, so nothing is gathered.
        temperature / top_k / top_p other than (1, 0, 1) draw from the tempered, truncated distribution instead
        (vlp_sample_rows_filtered: same seed cell, seed_add and RNG stream; logp is the log-probability under that distribution); the
        values (1, 0, 1) issue the launches of a call without them.
        Returns (ids [K*B, n] int64, logp [K*B, n] f32) sample-major: row k*B + b is sample k of image b.  Both are copies the caller owns,
        for every K (one copy each after the last token step, outside the captured steps): the next call at the same shapes overwrites the
        workspace's rows, not a result somebody still holds -- as decode_greedy and decode_beam clone theirs."""
        Ks, B = int(n_samples), input_ids.shape[0]
        if Ks < 1 or Ks > 16:
            raise RuntimeError("vlp_amd: decode_sample_group draws 1..16 samples per image (got %d)" % Ks)
        filt = (float(temperature), int(top_k), float(top_p))
        if not (0.0 < filt[0] < float("inf")) or filt[1] < 0 or filt[1] >= 1 << 31 or not (0.0 < filt[2] <= 1.0):
            raise RuntimeError("vlp_amd: decode_sample_group needs a finite temperature > 0, top_k >= 0 and 0 < top_p <= 1 (got %r, %r, %r)" %
                               (temperature, top_k, top_p))
        plain = filt == (1.0, 0, 1.0)
        R = B * Ks
        if R > 1024:
            raise RuntimeError("vlp_amd: %d samples of %d images are %d sequences; the sampled decode takes at most 1024" % (Ks, B, R))
        if R > 512 and not self._warned_group_unfused:
            self._warned_group_unfused = True
            import warnings
            warnings.warn("vlp_amd: %d sequences in a sampled decode: the fused token step takes at most 512 (1024 rows), the decode runs on the "
                          "unfused path" % R, VlpPerformanceWarning)
        c = self._decode_begin(vis_feats, vis_pe, input_ids, token_type_ids, position_ids, attention_mask, mask_word_id, Ks, group=True)
        ws, out_ids, out_val, cell = c.ws, c.ws["out_ids"], c.ws["out_val"], c.ws["seed_cell"]
        # The seed of step s is base_seed + step_seed + 1 + s (decode_greedy(sample=True)'s sequence), read by the sampling launches from a
        # device cell the host sets once per call: every launch of a token step has call-invariant arguments and the steps are captured /
        # replayed
        seed = (self.base_seed + self.step_seed + 1) & 0xFFFFFFFFFFFFFFFF
        cell.fill_(seed - (1 << 64) if seed >= (1 << 63) else seed)            # the uint64's bits in an int64 cell
        self.step_seed += c.n_steps
        if not plain and "filter_cutoff" not in ws:
            # the smallest kept logit and the size of the kept set of every draw of the last filtered call, [step, row]: one store each,
            # and what makes the set a call drew from checkable from outside
            ws.update(filter_cutoff=torch.zeros(out_ids.shape[1], R, device=self.device, dtype=torch.float32),
                      filter_kept=torch.zeros(out_ids.shape[1], R, device=self.device, dtype=torch.int32))

        def select(s, first):
            rep = Ks if first else 1
            if plain:
                K.sample_rows_rep(ws["logits"], ws["Vp"], R, c.V, rep, cell, s, 7001, out_ids[:, s], out_val[:, s], ids2=ws["xids"][:, 0])
            else:
                K.sample_rows_filtered(ws["logits"], ws["Vp"], R, c.V, rep, cell, s, 7001, filt[0], filt[1], filt[2], out_ids[:, s], out_val[:, s],
                                       ids2=ws["xids"][:, 0], cutoff=ws["filter_cutoff"][s], kept=ws["filter_kept"][s])

        # one sample per image: the rows are the images, their cache is `kv` itself (decode_greedy's launches)
        caches, prefix = (ws["kvS"], (ws["kv"], c.in_len, Ks)) if Ks > 1 else (ws["kv"], None)
        # a replayed step carries its own call's parameters: they are part of the key (the unfiltered steps keep theirs)
        self._decode_steps(c, select, lambda s: caches, prefix, lambda s: ("sample_group", s) + (() if plain else filt))
        return sample_major(out_ids, B, Ks, c.n_steps), sample_major(out_val, B, Ks, c.n_steps)

    NGRAM_MAX_FRAMES = 256       # csrc/elementwise.hip: NGRAM_MAX_FRAMES frames per hypothesis (and <= TOPK_LIST_MAX = 1024 ids per list)

    def decode_beam(self, vis_feats, vis_pe, input_ids, token_type_ids, position_ids, attention_mask, mask_word_id, beam_size, eos_id,
                    min_len=0, forbid_fn=None, ngram=None, groups=1, diversity=0.0, group_select="device", constraints=None,
                    constrained_select="device"):
        """Beam search frames (modeling.py:1255-1430) on the K/V-cache decoder.  The first step runs B sequences; its cache rows are
        replicated to the B*K beams (first_expand), afterwards every step decodes B*K sequences and the caches follow the back
        pointers (select_beam_items) -- only the generated positions; the prefix is identical for all beams of a sample and is kept,
        and streamed by the attention kernel, once per sample.
        `forbid_fn(step_ids [B,K] list, back_ptrs [B,K] list, first)` -> uint8 [B*K, V] numpy mask or None implements the host-side
        n-gram blocking (:1367-1430); when given, ids / pointers are copied to the host every step exactly as the reference does.
        `ngram=(n, ignore_ids)` (n >= 2; ignore_ids: token ids or None) is the same blocking on the device: after frame s vlp_ngram_candidates
        lists every hypothesis's forbidden words from the resident frames, step s+1 selects with vlp_logsoftmax_topk_list; nothing goes to
        the host before the frames are returned and the token steps are captured / replayed like those of an unblocked search.
        `groups=G > 1` (G divides K) with `diversity=lambda >= 0` is a diverse (group) beam search (vlp_amd.diverse is the rule; not in the
        reference): every frame selects with vlp_beam_select_groups where vlp_beam_select stands otherwise -- one launch for one launch, so the
        steps are captured / replayed as well.  The frames keep the unpenalised scores; back pointers stay inside their group.  groups=1 is
        the search as it is and refuses a diversity.
        `group_select="host"` is the A/B and fallback path of G > 1: every frame copies the top-K lists and the last frame's totals / eos flags
        to the host, runs diverse.beam_select_groups_host and uploads the frame.
        `constraints=(cons_ids [B, C, Lc], cons_len [B, C])` is a constrained beam search (vlp_amd.constrained is the rule; not in the
        reference): up to 8 phrases of up to 8 word pieces per image that its caption must mention.  The pair is checked on the host and
        copied into buffers of the workspace, with the first frame's wanted words, before anything is launched: the captured steps point at
        those buffers, never at the caller's tensors.  A step then launches vlp_logsoftmax_topk_want for the top-K call and
        vlp_beam_select_constrained for vlp_beam_select (the last frame with its `last` flag: a hypothesis cut off by the target length
        unmet is forbidden as an unmet eos is) -- one for one, captured / replayed, ("constrained", C, Lc) in the plan key; ngram=,
        forbid_fn= and min_len work as before, groups > 1 is refused.  `constrained_select="host"` runs
        constrained.beam_select_constrained_host per frame instead (A/B and fallback, not planned).  The call returns a fourth tensor, the
        state frames int32 [frames, B, K].  Without constraints nothing changes, launch for launch.
        Returns (total_scores, step_ids, back_ptrs) as [frames, B, K] tensors on the device."""
        Kb, eos_id = int(beam_size), int(eos_id)
        G, lam = int(groups), float(diversity)
        if group_select not in ("device", "host"):
            raise ValueError("group_select must be 'device' or 'host', got %r" % (group_select,))
        if G == 1:
            if lam != 0.0:
                raise ValueError("vlp_amd: diversity=%r needs groups > 1 (groups=1 is the plain beam search)" % (diversity,))
        else:
            from .diverse import check_limits as check_groups
            check_groups(Kb, G, lam)
        if Kb < 2 or Kb > 64:
            raise RuntimeError("vlp_amd: beam size must be in [2, 64]")
        if constrained_select not in ("device", "host"):
            raise ValueError("constrained_select must be 'device' or 'host', got %r" % (constrained_select,))
        cons = None
        if constraints is not None:
            from . import constrained as CB
            if G > 1:
                raise ValueError("vlp_amd: constraints and groups > 1 (diverse beam search) exclude each other")
            cons = CB.check_constraints(constraints[0], constraints[1], self._model().config.vocab_size, eos_id)
            if cons[0].shape[0] != input_ids.shape[0]:
                raise ValueError("vlp_amd: constraints for %d images, batch of %d" % (cons[0].shape[0], input_ids.shape[0]))
            CB.check_limits(Kb, cons[0].shape[1], cons[0].shape[2])
        if ngram is not None:
            if forbid_fn is not None:
                raise RuntimeError("vlp_amd: decode_beam takes forbid_fn (host blocking) or ngram (device blocking), not both")
            ng_n, ign, n_steps = int(ngram[0]), ngram[1], token_type_ids.shape[1] - input_ids.shape[1]
            if ng_n < 2:
                raise RuntimeError("vlp_amd: device n-gram blocking needs ngram_size >= 2 (got %d)" % ng_n)
            if n_steps > self.NGRAM_MAX_FRAMES:          # the kernels' limits, checked before anything is launched
                raise RuntimeError("vlp_amd: device n-gram blocking handles at most %d generated tokens (vlp_ngram_candidates keeps a hypothesis in LDS), "
                                   "this search asks for %d; shorten the target or use ngram_blocking='host'" % (self.NGRAM_MAX_FRAMES, n_steps))
            ign = tuple(sorted(set(int(t) for t in (ign.tolist() if torch.is_tensor(ign) else ign)))) if ign is not None else ()
        c = self._decode_begin(vis_feats, vis_pe, input_ids, token_type_ids, position_ids, attention_mask, mask_word_id, Kb)
        ws, B, V, n_steps, NL, H = c.ws, c.B, c.V, c.n_steps, self._model().config.num_hidden_layers, self._model().config.hidden_size
        tot, wids, ptrs, eos = ws["tot"], ws["wids"], ws["ptrs"], ws["eos"]
        bufs = (ws["kvA"], ws["kvB"])
        host = {"forbid": None}          # forbid_fn's mask for the next frame
        on_host = (G > 1 and group_select == "host") or (cons is not None and constrained_select == "host")
        # what the selection bakes into a captured step beyond (s, eos_id, block_eos): the blocking's size and ignore list, and (G, lambda)
        plan_tag = ()
        if ngram is not None:
            ng_ignore = None
            if ign:                      # one device copy per distinct ignore list, owned by the workspace (the captured launches point at it)
                ng_ignore = ws["ngram_ignore"].get(ign)
                if ng_ignore is None:
                    ng_ignore = ws["ngram_ignore"][ign] = torch.tensor(ign, device=self.device, dtype=torch.long)
            plan_tag = ("ngram", ng_n, ign)
        if G > 1:
            plan_tag += ("groups", G, lam)
        if cons is not None:
            Cc, Lc = cons[0].shape[1], cons[0].shape[2]
            cw = ws.setdefault("constrained", {}).get((Cc, Lc))
            if cw is None:       # owned by the workspace, one set per (C, Lc): what the captured launches of that plan key point at
                i32 = dict(device=self.device, dtype=torch.int32)
                cw = ws["constrained"][(Cc, Lc)] = dict(
                    ids=torch.empty(B, Cc, Lc, **i32), len=torch.empty(B, Cc, **i32), want=torch.empty(2, c.R, Cc, **i32),
                    want_val=torch.empty(c.R, Cc, device=self.device, dtype=torch.float32), state=torch.empty(c.out_len, B, Kb, **i32))
            cw["ids"].copy_(torch.from_numpy(cons[0]))
            cw["len"].copy_(torch.from_numpy(cons[1]))
            # frame 0's wanted words: the first piece of every phrase, -1 for an unused slot (wanted(0))
            # (two want buffers: frame s reads want[s & 1] and writes the next frame's words to the other one)
            cw["want"][0, :B].copy_(torch.from_numpy(np.where(cons[1] > 0, cons[0][:, :, 0], -1).astype(np.int32)))
            cstate = cw["state"]
            plan_tag += ("constrained", Cc, Lc)

        def block_eos(s):
            return bool(min_len) and (s + 1 <= min_len)

        def select_constrained_on_host(s, first):
            kk_s, kk_i = (ws["kk_s"][:B], ws["kk_i"][:B]) if first else (ws["kk_s"].view(B, Kb, Kb), ws["kk_i"].view(B, Kb, Kb))
            rows = B if first else c.R
            out = CB.beam_select_constrained_host(kk_s, kk_i, cw["want"][s & 1, :rows], cw["want_val"][:rows], None if first else tot[s - 1],
                                                  None if first else eos[s - 1], None if first else cstate[s - 1], cons[0], cons[1], first, eos_id,
                                                  last=s + 1 == n_steps)
            for dst, src in ((tot[s], out[0]), (wids[s], out[1]), (ptrs[s], out[2]), (eos[s], out[3]), (ws["src_rows"], out[4]),
                             (ws["xids"][:, 0], out[1].reshape(-1)), (cstate[s], out[6]), (cw["want"][(s + 1) & 1], out[7])):
                dst.copy_(torch.from_numpy(src))

        def select_on_host(s, first):
            from .diverse import beam_select_groups_host
            kk_s, kk_i = (ws["kk_s"][:B], ws["kk_i"][:B]) if first else (ws["kk_s"].view(B, Kb, Kb), ws["kk_i"].view(B, Kb, Kb))
            o_tot, o_ids, o_ptr, o_eos, o_src, _ = beam_select_groups_host(kk_s, kk_i, None if first else tot[s - 1], None if first else eos[s - 1],
                                                                           first, eos_id, G, lam)
            for dst, src in ((tot[s], o_tot), (wids[s], o_ids), (ptrs[s], o_ptr), (eos[s], o_eos), (ws["src_rows"], o_src),
                             (ws["xids"][:, 0], o_ids.reshape(-1))):
                dst.copy_(torch.from_numpy(src))

        def select(s, first):
            # step 0: B sequences.  first_expand (:1325-1332) is implicit: the prefix K|V of a sample stays in its per-sample cache and is
            # shared by its beams inside the attention kernel; the per-beam caches only ever hold generated positions
            rows, prev_tot, prev_eos = (B, None, None) if first else (c.R, tot[s - 1], eos[s - 1])
            if cons is not None:
                listed = ngram is not None and not first
                K.logsoftmax_topk_want(ws["logits"], ws["Vp"], rows, V, Kb, ws["kk_s"], ws["kk_i"], cw["want"][s & 1], cw["want_val"],
                                       forbid=None if listed else host["forbid"], cand_ids=ws["cand_ids"] if listed else None,
                                       cand_cnt=ws["cand_cnt"] if listed else None, eos_id=eos_id, block_eos=block_eos(s))
            elif ngram is not None and not first:
                K.logsoftmax_topk_list(ws["logits"], ws["Vp"], rows, V, Kb, ws["kk_s"], ws["kk_i"], ws["cand_ids"], ws["cand_cnt"], eos_id=eos_id,
                                       block_eos=block_eos(s))
            else:
                K.logsoftmax_topk(ws["logits"], ws["Vp"], rows, V, Kb, ws["kk_s"], ws["kk_i"], forbid=host["forbid"], eos_id=eos_id,
                                  block_eos=block_eos(s))
            if cons is not None:
                if on_host:
                    select_constrained_on_host(s, first)
                else:
                    K.beam_select_constrained(ws["kk_s"], ws["kk_i"], prev_tot, prev_eos, tot[s], wids[s], ptrs[s], eos[s], ws["src_rows"],
                                              ws["xids"][:, 0], B, Kb, first, eos_id, cw["want"][s & 1], cw["want_val"],
                                              None if first else cstate[s - 1], cw["ids"], cw["len"], Cc, Lc, cstate[s], cw["want"][(s + 1) & 1],
                                              last=s + 1 == n_steps)
            elif G == 1:
                K.beam_select(ws["kk_s"], ws["kk_i"], prev_tot, prev_eos, tot[s], wids[s], ptrs[s], eos[s], ws["src_rows"], ws["xids"][:, 0],
                              B, Kb, first, eos_id)
            elif on_host:
                select_on_host(s, first)
            else:
                K.beam_select_groups(ws["kk_s"], ws["kk_i"], prev_tot, prev_eos, tot[s], wids[s], ptrs[s], eos[s], ws["src_rows"],
                                     ws["xids"][:, 0], B, Kb, first, eos_id, G, lam)
            if ngram is not None and s + 1 < n_steps:        # the next step's forbidden words (frame 0: s + 1 < n, every count becomes 0)
                K.ngram_candidates(wids, ptrs, B, Kb, s, ng_n, ws["cand_ids"], ws["cand_cnt"], ignore_ids=ng_ignore)
            if not first and s + 1 < n_steps:      # select_beam_items (:1334-1359): generated positions in_len .. st follow their beam
                cur, other = bufs[(s - 1) & 1], bufs[s & 1]            # the caches swap after every step >= 1
                for i in range(NL):
                    K.kv_gather(cur[i], c.out_len, other[i], c.out_len, ws["src_rows"], c.R, c.in_len, c.in_len + s, 2 * H)

        def plan_key(s):
            if forbid_fn is not None or on_host:     # the forbid mask is a fresh tensor every step / the selection runs on the host
                return None
            return ("beam", s, eos_id, block_eos(s)) + plan_tag

        def ask_forbid_fn(s):
            fm = forbid_fn(wids[s].tolist(), ptrs[s].tolist(), s == 0)
            host["forbid"] = None if fm is None else torch.from_numpy(fm).to(self.device)

        self._decode_steps(c, select, lambda s: bufs[(s - 1) & 1], (ws["kv"], c.in_len, Kb), plan_key,
                           between=ask_forbid_fn if forbid_fn is not None else None)
        if cons is not None:
            return tot[:n_steps].clone(), wids[:n_steps].clone(), ptrs[:n_steps].clone(), cstate[:n_steps].clone()
        return tot[:n_steps].clone(), wids[:n_steps].clone(), ptrs[:n_steps].clone()

    def beam_nbest(self, tot, wids, ptrs, n_best, eos_id, length_penalty, out_len):
        """The n_best best finished hypotheses of the frames decode_beam returned ([frames, B, K]), ranked and back-tracked on the device
        (vlp_beam_nbest; the rule is vlp_amd.nbest.beam_nbest_host's): one launch on the current stream, nothing goes to the host.
        Returns (seq int64 [n_best*B, out_len], score f32, value f64, len int32, ok uint8, each [n_best*B]), sample-major (rank n of image b
        is row n*B + b).  The outputs belong to the decode workspace of that search: the next call with the same shapes overwrites them."""
        from .nbest import check_limits
        if tot.dim() != 3 or wids.shape != tot.shape or ptrs.shape != tot.shape:
            raise ValueError("beam_nbest takes the three [frames, B, K] tensors of decode_beam")
        F, B, Kb = (int(v) for v in tot.shape)
        N, out_len = int(n_best), int(out_len)
        check_limits(F, B, Kb, N, out_len)
        ws = self._ws.get(("dec", B, out_len - F + 1, out_len, Kb))
        if ws is None:
            raise RuntimeError("vlp_amd: beam_nbest ranks the frames of a decode_beam call of this engine; there was none with batch %d, beam %d, "
                               "%d frames and output length %d" % (B, Kb, F, out_len))
        out = ws.setdefault("nbest", {}).get(N)
        if out is None:
            dev = self.device
            out = ws["nbest"][N] = (torch.empty(N * B, out_len, device=dev, dtype=torch.long), torch.empty(N * B, device=dev, dtype=torch.float32),
                                    torch.empty(N * B, device=dev, dtype=torch.float64), torch.empty(N * B, device=dev, dtype=torch.int32),
                                    torch.empty(N * B, device=dev, dtype=torch.uint8))
        K.beam_nbest(tot.contiguous(), wids.contiguous(), ptrs.contiguous(), N, int(eos_id), float(length_penalty), *out)
        return out
