"""Drop-in for `pytorch_pretrained_bert.modeling` of LuoweiZhou/VLP on MI355X.

Same public surface as the reference file (class names, constructor / forward signatures, submodule
tree and therefore state_dict keys, `from_pretrained` keyword handling -- citations below are into
pytorch_pretrained_bert/modeling.py), but the module tree is only a *container of parameters*: all
arithmetic of `BertForPreTrainingLossMask.forward` runs as hand-written HIP kernels through
libvlp_hip.so, sequenced by vlp_amd.engine.Engine (one fused forward/backward, no per-op autograd graph).

Not implemented (raise loudly; see DESIGN.md "out of scope"): fp32 execution, `enable_butd=False`
(the reference asserts it is True, run_img2txt_dist.py:199), `relax_projection`, and the dead HF heads
(:878-978, :1497-1966).  Label smoothing (`config.label_smoothing`, loss.py) runs on its own HIP loss kernels.  `mask_image_regions` / `vis_pretext_loss` (:1049-1056, 1113-1131) and the pooler they use are built.
"""
import copy
import json
import logging
import math
import os
import pickle

import torch
from torch import nn

from . import _lib as K
from .engine import Engine
from .input_prep import MaskSpec, SparseAnswers
from .loss import LabelSmoothingLoss

logger = logging.getLogger(__name__)

CONFIG_NAME = "bert_config.json"
WEIGHTS_NAME = "pytorch_model.bin"
PRETRAINED_MODEL_ARCHIVE_MAP = {   # names the reference resolves over the network (:49-57); offline they must be local dirs
    "bert-base-uncased": None, "bert-large-uncased": None, "bert-base-cased": None, "bert-large-cased": None,
    "bert-base-multilingual-uncased": None, "bert-base-multilingual-cased": None, "bert-base-chinese": None,
}


class BertConfig(object):
    """Same fields and helpers as the reference BertConfig (:77-171)."""

    def __init__(self, vocab_size_or_config_json_file, hidden_size=768, num_hidden_layers=12, num_attention_heads=12,
                 intermediate_size=3072, hidden_act="gelu", hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1,
                 max_position_embeddings=512, type_vocab_size=2, relax_projection=0, initializer_range=0.02, task_idx=None,
                 fp32_embedding=False, label_smoothing=None):
        if isinstance(vocab_size_or_config_json_file, str):
            with open(vocab_size_or_config_json_file, "r", encoding="utf-8") as reader:
                for key, value in json.loads(reader.read()).items():
                    self.__dict__[key] = value
        elif isinstance(vocab_size_or_config_json_file, int):
            self.vocab_size = vocab_size_or_config_json_file
            self.hidden_size = hidden_size
            self.num_hidden_layers = num_hidden_layers
            self.num_attention_heads = num_attention_heads
            self.hidden_act = hidden_act
            self.intermediate_size = intermediate_size
            self.hidden_dropout_prob = hidden_dropout_prob
            self.attention_probs_dropout_prob = attention_probs_dropout_prob
            self.max_position_embeddings = max_position_embeddings
            self.type_vocab_size = type_vocab_size
            self.relax_projection = relax_projection
            self.initializer_range = initializer_range
            self.task_idx = task_idx
            self.fp32_embedding = fp32_embedding
            self.label_smoothing = label_smoothing
        else:
            raise ValueError("First argument must be either a vocabulary size (int) or the path to a pretrained model config file (str)")

    @classmethod
    def from_dict(cls, json_object):
        config = BertConfig(vocab_size_or_config_json_file=-1)
        for key, value in json_object.items():
            config.__dict__[key] = value
        return config

    @classmethod
    def from_json_file(cls, json_file):
        with open(json_file, "r", encoding="utf-8") as reader:
            return cls.from_dict(json.loads(reader.read()))

    def __repr__(self):
        return str(self.to_json_string())

    def to_dict(self):
        return copy.deepcopy(self.__dict__)

    def to_json_string(self):
        return json.dumps(self.to_dict(), indent=2, sort_keys=True) + "\n"


def _no_direct_forward(self, *a, **k):
    raise NotImplementedError("%s is a parameter container in vlp_amd: the fused HIP path is entered through "
                              "BertForPreTrainingLossMask.forward / BertForSeq2SeqDecoder.forward" % type(self).__name__)


class BertLayerNorm(nn.Module):
    """Parameters of the TF-style LayerNorm (:174-192); evaluated by vlp_layernorm_fwd/bwd."""

    def __init__(self, hidden_size, eps=1e-5):
        super(BertLayerNorm, self).__init__()
        self.weight = nn.Parameter(torch.ones(hidden_size))
        self.bias = nn.Parameter(torch.zeros(hidden_size))
        self.variance_epsilon = eps

    def forward(self, x):
        """Stand-alone use (any [*, H] fp16 device tensor) through the C ABI."""
        H = x.shape[-1]
        x2 = x.reshape(-1, H).contiguous()
        y = torch.empty_like(x2)
        K.layernorm_fwd(x2, self.weight.data, self.bias.data, y, x2.shape[0], H, eps=self.variance_epsilon)
        return y.view(x.shape)


class BertEmbeddings(nn.Module):   # :195-241
    def __init__(self, config):
        super(BertEmbeddings, self).__init__()
        self.word_embeddings = nn.Embedding(config.vocab_size, config.hidden_size)
        self.position_embeddings = nn.Embedding(config.max_position_embeddings, config.hidden_size)
        self.token_type_embeddings = nn.Embedding(config.type_vocab_size, config.hidden_size)
        self.fp32_embedding = getattr(config, "fp32_embedding", False)
        self.LayerNorm = BertLayerNorm(config.hidden_size, eps=1e-5)
        self.dropout = nn.Dropout(config.hidden_dropout_prob)
    forward = _no_direct_forward


class BertSelfAttention(nn.Module):   # :244-303
    def __init__(self, config):
        super(BertSelfAttention, self).__init__()
        if config.hidden_size % config.num_attention_heads != 0:
            raise ValueError("The hidden size (%d) is not a multiple of the number of attention heads (%d)"
                             % (config.hidden_size, config.num_attention_heads))
        self.num_attention_heads = config.num_attention_heads
        self.attention_head_size = int(config.hidden_size / config.num_attention_heads)
        self.all_head_size = self.num_attention_heads * self.attention_head_size
        self.query = nn.Linear(config.hidden_size, self.all_head_size)
        self.key = nn.Linear(config.hidden_size, self.all_head_size)
        self.value = nn.Linear(config.hidden_size, self.all_head_size)
        self.dropout = nn.Dropout(config.attention_probs_dropout_prob)
    forward = _no_direct_forward


class BertSelfOutput(nn.Module):   # :306-317
    def __init__(self, config):
        super(BertSelfOutput, self).__init__()
        self.dense = nn.Linear(config.hidden_size, config.hidden_size)
        self.LayerNorm = BertLayerNorm(config.hidden_size, eps=1e-5)
        self.dropout = nn.Dropout(config.hidden_dropout_prob)
    forward = _no_direct_forward


class BertAttention(nn.Module):   # :320-330
    def __init__(self, config):
        super(BertAttention, self).__init__()
        self.self = BertSelfAttention(config)
        self.output = BertSelfOutput(config)
    forward = _no_direct_forward


class BertIntermediate(nn.Module):   # :333-343
    def __init__(self, config):
        super(BertIntermediate, self).__init__()
        if config.hidden_act != "gelu":
            raise NotImplementedError("vlp_amd fuses the erf-GELU of the reference configs; hidden_act=%r is not supported" % (config.hidden_act,))
        self.dense = nn.Linear(config.hidden_size, config.intermediate_size)
    forward = _no_direct_forward


class BertOutput(nn.Module):   # :346-357
    def __init__(self, config):
        super(BertOutput, self).__init__()
        self.dense = nn.Linear(config.intermediate_size, config.hidden_size)
        self.LayerNorm = BertLayerNorm(config.hidden_size, eps=1e-5)
        self.dropout = nn.Dropout(config.hidden_dropout_prob)
    forward = _no_direct_forward


class BertLayer(nn.Module):   # :360-372
    def __init__(self, config):
        super(BertLayer, self).__init__()
        self.attention = BertAttention(config)
        self.intermediate = BertIntermediate(config)
        self.output = BertOutput(config)
    forward = _no_direct_forward


class BertEncoder(nn.Module):   # :375-402
    def __init__(self, config):
        super(BertEncoder, self).__init__()
        self.layer = nn.ModuleList([BertLayer(config) for _ in range(config.num_hidden_layers)])
    forward = _no_direct_forward


class BertPooler(nn.Module):   # :405-417
    def __init__(self, config):
        super(BertPooler, self).__init__()
        self.dense = nn.Linear(config.hidden_size, config.hidden_size)
        self.activation = nn.Tanh()
    forward = _no_direct_forward


class BertPredictionHeadTransform(nn.Module):   # :420-435
    def __init__(self, config):
        super(BertPredictionHeadTransform, self).__init__()
        if getattr(config, "relax_projection", 0) > 1:
            raise NotImplementedError("relax_projection > 1 is not supported by vlp_amd (off in every reference config)")
        self.dense = nn.Linear(config.hidden_size, config.hidden_size)
        self.LayerNorm = BertLayerNorm(config.hidden_size, eps=1e-5)
    forward = _no_direct_forward


class BertLMPredictionHead(nn.Module):   # :438-482
    def __init__(self, config, bert_model_embedding_weights):
        super(BertLMPredictionHead, self).__init__()
        self.transform = BertPredictionHeadTransform(config)
        self.decoder = nn.Linear(bert_model_embedding_weights.size(1), bert_model_embedding_weights.size(0), bias=False)
        self.decoder.weight = bert_model_embedding_weights      # tied (:445-448)
        self.bias = nn.Parameter(torch.zeros(bert_model_embedding_weights.size(0)))
        self.relax_projection = 0
        self.fp32_embedding = getattr(config, "fp32_embedding", False)
    forward = _no_direct_forward


class BertPreTrainingHeads(nn.Module):   # :506-520
    def __init__(self, config, bert_model_embedding_weights, num_labels=2):
        super(BertPreTrainingHeads, self).__init__()
        self.predictions = BertLMPredictionHead(config, bert_model_embedding_weights)
    forward = _no_direct_forward


def load_checkpoint_state(model, state_dict):
    """The checkpoint remapping of the reference's from_pretrained (:651-752), shared by `from_pretrained` and the train
    script: TF-era gamma/beta names, segment table 2 -> 6 rows, position-table tiling, size-mismatch errors; sets
    `model.missing_keys`.  Anything whose shape does not fit after the remapping raises (never silently skipped)."""
    config = model.config
    state_dict = dict(state_dict)
    # TF-era names (:651-663)
    for key in list(state_dict.keys()):
        new_key = key.replace("gamma", "weight").replace("beta", "bias")
        if new_key != key:
            state_dict[new_key] = state_dict.pop(key)
    H = config.hidden_size
    # segment table 2 -> 6 rows: rows 2,3,4 start from row 0 and row 5 from row 1 (:665-683)
    k = "bert.embeddings.token_type_embeddings.weight"
    if k in state_dict and state_dict[k].shape[0] != config.type_vocab_size:
        old = state_dict[k]
        if config.type_vocab_size > old.shape[0]:
            new = old.new_zeros(config.type_vocab_size, H)
            new.normal_(mean=0.0, std=config.initializer_range)
            new[:old.shape[0]] = old
            if config.type_vocab_size >= 6:
                new[2], new[3], new[4], new[5] = old[0], old[0], old[0], old[1]
            state_dict[k] = new
        else:
            state_dict[k] = old[:config.type_vocab_size]
    # position table: tile the learned rows when it grows (:685-702)
    k = "bert.embeddings.position_embeddings.weight"
    if k in state_dict and state_dict[k].shape[0] != config.max_position_embeddings:
        old = state_dict[k]
        n_old, n_new = old.shape[0], config.max_position_embeddings
        if n_new > n_old:
            reps = int(math.ceil(n_new / float(n_old)))
            state_dict[k] = old.repeat(reps, 1)[:n_new].clone()
        else:
            state_dict[k] = old[:n_new]
    k = "cls.predictions.transform.dense.weight"
    if k in state_dict and state_dict[k].shape[0] != H:
        raise NotImplementedError("checkpoint uses relax_projection; not supported by vlp_amd")
    own = model.state_dict()
    # a bare BertModel reads the 'bert.'-prefixed entries of a task checkpoint (:751)
    strip = "" if hasattr(model, "bert") else "bert."
    missing, unexpected, load = [], [], {}
    for key, value in state_dict.items():
        if strip and not key.startswith(strip):
            unexpected.append(key)
            continue
        full = key[len(strip):]
        if full in own:
            if tuple(own[full].shape) != tuple(value.shape):
                raise RuntimeError("size mismatch for %s: checkpoint %s vs model %s" % (full, tuple(value.shape), tuple(own[full].shape)))
            load[full] = value
        else:
            unexpected.append(key)
    for key in own:
        if key not in load:
            missing.append(key)
    nn.Module.load_state_dict(model, load, strict=False)
    model.missing_keys = missing
    if missing:
        logger.info("Weights of {} not initialized from pretrained model: {}".format(model.__class__.__name__, missing))
    if unexpected:
        logger.info("Weights from pretrained model not used in {}: {}".format(model.__class__.__name__, unexpected))
    return model


class PreTrainedBertModel(nn.Module):
    """Weight init and `from_pretrained` (:523-764)."""

    def __init__(self, config, *inputs, **kwargs):
        super(PreTrainedBertModel, self).__init__()
        if not isinstance(config, BertConfig):
            raise ValueError("Parameter config in `{}(config)` should be an instance of class `BertConfig`.".format(self.__class__.__name__))
        self.config = config

    def init_bert_weights(self, module):   # :539-551
        if isinstance(module, (nn.Linear, nn.Embedding)):
            module.weight.data.normal_(mean=0.0, std=self.config.initializer_range)
        elif isinstance(module, BertLayerNorm):
            module.bias.data.zero_()
            module.weight.data.fill_(1.0)
        if isinstance(module, nn.Linear) and module.bias is not None:
            module.bias.data.zero_()

    # parameters live in flat device buffers once packed: any storage-changing _apply must unlink them
    def _apply(self, fn, *a, **k):
        eng = self.__dict__.get("_engine")
        out = super(PreTrainedBertModel, self)._apply(fn, *a, **k)
        if eng is not None:
            eng.invalidate()
        return out

    def __deepcopy__(self, memo):
        # deepcopy (run_img2txt_dist.py:598 `copy.deepcopy(model_to_save).cpu()`) must not clone workspaces
        cls = self.__class__
        new = cls.__new__(cls)
        memo[id(self)] = new
        for k, v in self.__dict__.items():
            if k == "_engine":
                continue
            new.__dict__[k] = copy.deepcopy(v, memo)
        new.__dict__["_engine"] = Engine(new) if "_engine" in self.__dict__ else None
        for p in new.parameters():
            p.grad = None
            if hasattr(p, "_vlp_engine"):
                del p._vlp_engine
            if new.__dict__["_engine"] is not None:
                p._vlp_owner = new.__dict__["_engine"]
        return new

    def state_dict(self, *args, **kwargs):
        """Same keys as the reference; tensors are detached clones so a checkpoint never drags the flat
        parameter buffer along."""
        eng = self.__dict__.get("engine") or getattr(self, "engine", None)
        if eng is not None and getattr(eng, "packed", False):
            eng.wait_params()            # a pipelined optimizer step may still be writing the flat parameter buffers
        sd = super(PreTrainedBertModel, self).state_dict(*args, **kwargs)
        if args or kwargs.get("destination") is not None:
            return sd            # nested call from a parent module: the top-level call clones once
        for k in list(sd.keys()):
            sd[k] = sd[k].detach().clone()
        return sd

    @classmethod
    def from_pretrained(cls, pretrained_model_name, state_dict=None, cache_dir=None, *inputs, **kwargs):
        """Same contract as the reference (:554-764): `pretrained_model_name` is a directory holding
        bert_config.json (+ pytorch_model.bin unless `state_dict` is given; `state_dict={}` means random
        init, run_img2txt_dist.py:320-323).  Model *names* need the network in the reference and are
        rejected here."""
        if pretrained_model_name in PRETRAINED_MODEL_ARCHIVE_MAP and not os.path.isdir(pretrained_model_name):
            config_path = kwargs.get("config_path")
            if not config_path:
                raise EnvironmentError("'%s' would be downloaded by the reference; offline, pass a local model directory "
                                       "(bert_config.json [+ pytorch_model.bin]) or config_path=..." % pretrained_model_name)
            serialization_dir = None
        else:
            serialization_dir = pretrained_model_name
            if not os.path.isdir(serialization_dir):
                logger.error("Model directory '%s' not found", pretrained_model_name)
                return None
        config_file = kwargs.get("config_path") or os.path.join(serialization_dir, CONFIG_NAME)
        config = BertConfig.from_json_file(config_file)
        # keyword overrides (:615-636)
        if "type_vocab_size" in kwargs:
            config.type_vocab_size = kwargs["type_vocab_size"]
        for key in ("relax_projection", "task_idx", "max_position_embeddings", "fp32_embedding", "label_smoothing"):
            if kwargs.get(key):
                setattr(config, key, kwargs[key])
        if "drop_prob" in kwargs:
            config.attention_probs_dropout_prob = kwargs["drop_prob"]
            config.hidden_dropout_prob = kwargs["drop_prob"]
        for key in ("config_path", "type_vocab_size", "relax_projection", "task_idx", "max_position_embeddings", "fp32_embedding",
                    "label_smoothing", "drop_prob"):
            kwargs.pop(key, None)
        for key in ("relax_projection", "task_idx", "fp32_embedding", "label_smoothing"):
            if not hasattr(config, key):
                setattr(config, key, None if key in ("task_idx", "label_smoothing") else 0)
        logger.info("Model config {}".format(config))
        model = cls(config, *inputs, **kwargs)
        if state_dict is None:
            if serialization_dir is None:
                raise EnvironmentError("no weights: pass state_dict (or {} for random init)")
            state_dict = torch.load(os.path.join(serialization_dir, WEIGHTS_NAME), map_location="cpu")
        load_checkpoint_state(model, state_dict)
        return model


class BertModel(PreTrainedBertModel):
    """Embeddings + encoder + pooler parameters (:767-849).  As a sub-module of the task models it is a
    container; the fused path owns its arithmetic."""

    def __init__(self, config):
        super(BertModel, self).__init__(config)
        self.embeddings = BertEmbeddings(config)
        self.encoder = BertEncoder(config)
        self.pooler = BertPooler(config)
        self.apply(self.init_bert_weights)
    forward = _no_direct_forward


class BertModelIncr(BertModel):   # :852-875
    def __init__(self, config):
        super(BertModelIncr, self).__init__(config)


def _region_embedders(module, config, enable_butd, allow_random_fc7):
    """vis_embed / vis_pe_embed exactly as the reference builds them (:1002-1018)."""
    if not enable_butd:
        raise NotImplementedError("vlp_amd supports region features only (enable_butd=True); the reference itself asserts this "
                                  "(run_img2txt_dist.py:199 'featmap attn deprecated')")
    module.vis_embed = nn.Sequential(nn.Linear(2048, 2048), nn.ReLU(), nn.Linear(2048, config.hidden_size), nn.ReLU(),
                                     nn.Dropout(config.hidden_dropout_prob))
    module.vis_pe_embed = nn.Sequential(nn.Linear(6 + 1601, config.hidden_size), nn.ReLU(), nn.Dropout(config.hidden_dropout_prob))
    return allow_random_fc7


def _load_fc7(module, allow_random):
    """Detectron fc7 weights are read relative to the CWD like the reference (:1008-1014)."""
    try:
        with open("detectron_weights/fc7_w.pkl", "rb") as f:
            w = torch.from_numpy(pickle.load(f))
        with open("detectron_weights/fc7_b.pkl", "rb") as f:
            b = torch.from_numpy(pickle.load(f))
        module.vis_embed[0].weight.data.copy_(w)
        module.vis_embed[0].bias.data.copy_(b)
    except Exception:
        if allow_random or os.environ.get("VLP_ALLOW_RANDOM_FC7") == "1":
            return
        raise Exception("Cannot find Detectron fc7 weights! Download from https://dl.fbaipublicfiles.com/ActivityNet-Entities/"
                        "ActivityNet-Entities/detectron_weights.tar.gz and uncompress under the code root directory "
                        "(or pass allow_random_fc7=True / VLP_ALLOW_RANDOM_FC7=1 for synthetic runs).")


class _LossFn(torch.autograd.Function):
    """Hands the fused backward to autograd: `loss.backward()` (run_img2txt_dist.py:571-575) reaches
    Engine.backward with the upstream scalar gradient (which carries the fp16 loss scale).  With mask_image_regions the forward has two
    live losses (task loss, vis_pretext_loss; the train loop sums them, :531): both are outputs of ONE node, so a single backward call
    receives both upstream gradients."""

    @staticmethod
    def forward(ctx, anchor, loss, pretext, engine, state, task):
        ctx.engine, ctx.state, ctx.task = engine, state, task
        ctx.has_pretext = pretext is not None
        if pretext is None:
            return loss.clone()
        return loss.clone(), pretext.clone()

    @staticmethod
    def backward(ctx, grad, grad_pt=None):
        g = grad.detach().to(torch.float32).reshape(1).contiguous()
        gp = grad_pt.detach().to(torch.float32).reshape(1).contiguous() if ctx.has_pretext else None
        ctx.engine.backward(ctx.state, g, ctx.task, g_pretext=gp)
        return None, None, None, None, None, None


class _LogprobFn(torch.autograd.Function):
    """The sampled captions' log-probabilities [B, T] of a train-mode `sample_mode='sample'` forward as an autograd output: any torch loss
    on them (RewardCriterion, scst_utils.py:66-78) reaches Engine.backward(task="logprob") with dL/dlogp, which carries the fp16 loss scale.
    With `entropy` (the policy's entropy rows of the same scoring pass, return_entropy=True) there is a second differentiable output, and
    the backward hands dL/dlogp and dL/dentropy to the engine in one call."""

    @staticmethod
    def forward(ctx, anchor, logp, engine, state, entropy=None):
        ctx.engine, ctx.state, ctx.has_entropy = engine, state, entropy is not None
        if entropy is None:
            return logp.clone()
        return logp.clone(), entropy.clone()

    @staticmethod
    def backward(ctx, grad, grad_h=None):
        g = grad.detach().to(torch.float32).contiguous().reshape(-1)
        if not ctx.has_entropy:
            ctx.engine.backward(ctx.state, None, "logprob", g_rows=g)
            return None, None, None, None
        h = grad_h.detach().to(torch.float32).contiguous().reshape(-1)
        ctx.engine.backward(ctx.state, None, "logprob", g_rows=g, h_rows=h)
        return None, None, None, None, None


class BertForPreTrainingLossMask(PreTrainedBertModel):
    """The VLP training / VQA model (:982-1143) on the fused HIP path."""

    def __init__(self, config, num_labels=2, enable_butd=False, len_vis_input=49, tasks="img2txt", allow_random_fc7=False):
        super(BertForPreTrainingLossMask, self).__init__(config)
        self.bert = BertModel(config)
        self.cls = BertPreTrainingHeads(config, self.bert.embeddings.word_embeddings.weight, num_labels=num_labels)
        self.apply(self.init_bert_weights)
        self.num_labels = num_labels
        self.len_vis_input = len_vis_input
        self.enable_butd = enable_butd
        if getattr(config, "label_smoothing", None):                   # :995-999; a buffer, never a parameter of the engine's flat layout
            self.crit_mask_lm_smoothed = LabelSmoothingLoss(config.label_smoothing, config.vocab_size, ignore_index=0, reduction="none")
        else:
            self.crit_mask_lm_smoothed = None
        _region_embedders(self, config, enable_butd, allow_random_fc7)
        _load_fc7(self, allow_random_fc7)
        self.tasks = tasks
        self.num_answers = 3129          # hard-coded in the reference (:1029)
        if tasks == "vqa2":
            self.ans_classifier = nn.Sequential(nn.Linear(config.hidden_size, config.hidden_size * 2), nn.ReLU(),
                                                nn.Linear(config.hidden_size * 2, self.num_answers))
        self.__dict__["_engine"] = Engine(self)
        for prm in self.parameters():          # lets optimizers / DDP find the engine before the first forward packs
            prm._vlp_owner = self.__dict__["_engine"]

    @property
    def engine(self):
        return self.__dict__["_engine"]

    def forward(self, vis_feats, vis_pe, input_ids, token_type_ids=None, attention_mask=None, masked_lm_labels=None, ans_labels=None,
                next_sentence_label=None, masked_pos=None, masked_weights=None, task_idx=None, vis_masked_pos=[],
                mask_image_regions=False, drop_worst_ratio=0.2, vqa_inference=False):
        eng = self.engine
        if token_type_ids is None:
            token_type_ids = torch.zeros_like(input_ids)
        train = self.training

        if vqa_inference:                                              # :1039-1047 (returns before the region masking of :1049)
            assert ans_labels is None
            st = eng.forward(vis_feats, vis_pe, input_ids, token_type_ids, attention_mask, None, False, False, True)
            logits = eng.vqa_logits(st)
            self.last_vqa_logits = logits
            return torch.max(logits[:, 1:].float(), -1)[1] + 1
        if masked_lm_labels is None or next_sentence_label is None:    # :1062-1063
            raise NotImplementedError
        vmp = None
        if mask_image_regions:                                         # :1049-1056, 1113-1131
            if not torch.is_tensor(vis_masked_pos) or vis_masked_pos.dim() != 2 or vis_masked_pos.shape[1] == 0:
                raise ValueError("mask_image_regions=True needs vis_masked_pos [B, n_masked] (seq2seq_loader.py:267-269)")
            vmp = vis_masked_pos
        is_vqa = self.tasks == "vqa2"
        if is_vqa:
            assert ans_labels is not None
        want_mlm = (not is_vqa) and masked_pos is not None and masked_pos.numel() > 0
        st = eng.forward(vis_feats, vis_pe, input_ids, token_type_ids, attention_mask, masked_pos, train, want_mlm, is_vqa, vis_masked_pos=vmp)
        # the reference's `.new(1).fill_(0)` placeholders of the losses a task does not have (:1096-1098, 1133): ONE read-only [1] zero per engine,
        # handed out by identity (no fill / clone launches per step; vlp_amd.run_img2txt_dist.train_step skips adding it) -- do not modify it in place
        zero1 = eng.zero_placeholder(input_ids.device)
        need_grad = torch.is_grad_enabled()
        raw_pt = eng.pretext_loss(st) if vmp is not None else None
        if vmp is not None:
            self.last_pooled_output = eng.pooled_output(st)

        def live(raw, task):
            """(task loss, pretext loss) as autograd outputs of one node; the pretext placeholder is the reference's [1] zero (:1133)."""
            if not need_grad:
                return raw.clone(), (raw_pt.clone().reshape(()) if raw_pt is not None else zero1)
            if raw_pt is None:
                return _LossFn.apply(eng._anchor, raw, None, eng, st, task), zero1
            a, b = _LossFn.apply(eng._anchor, raw, raw_pt, eng, st, task)
            return a, b.reshape(())                                     # :1131: a 0-dim mean

        if is_vqa:
            raw = eng.vqa_loss(st, ans_labels)
            self.last_vqa_logits = eng.vqa_logits(st)
            loss, pt_loss = live(raw, "vqa2")
            return zero1, pt_loss, loss.reshape(())                     # :1141 shapes ([1], [1] | [], [])
        if not want_mlm:
            if raw_pt is None:
                return zero1, zero1, zero1                              # :1096-1098
            loss, pt_loss = live(zero1.clone(), "img2txt")              # empty masked_pos: only the pretext loss is live
            return loss, pt_loss, zero1
        raw = eng.mlm_loss(st, masked_lm_labels, masked_weights, drop_worst_ratio)
        self.last_mlm_logits = eng.mlm_logits(st)
        loss, pt_loss = live(raw, "img2txt")
        return loss.reshape(()), pt_loss, zero1                         # :1143 shapes ([], [1] | [], [1])

    def answer(self, vis_feats, vis_pe, input_ids, token_type_ids=None, attention_mask=None, answers=None):
        """VQA prediction (:1039-1047, eval_vqa2.py:237-244) for a batch of questions: (ans_idx int64 [B], ans_logit f32 [B], ans_score f32 [B]
        or None).  ans_idx = argmax(logits[:, 1:]) + 1 (first maximum; index 0, the unknown answer, is never predicted), ans_logit its logit;
        with `answers` (a SparseAnswers on the GPU: the questions' human answers) ans_score is the soft accuracy of each prediction -- the
        score the question lists for it, 0 when it lists none.  One engine forward without dropout, then ONE vlp_vqa_answer_rows launch
        (no fp32 copy of the logits, no read-back).  The forward is padding-free when attention_mask is a MaskSpec that carries the lengths
        on the host: the packed step is defined for gradient-enabled forwards (Engine.VARLEN), so that is the forward taken then -- what it
        adds (the transposed mask, the W^T shadows) runs on the side stream.  Sets last_vqa_logits."""
        if self.tasks != "vqa2":
            raise RuntimeError("answer() needs a model built with tasks='vqa2'")
        eng = self.engine
        if token_type_ids is None:
            token_type_ids = torch.zeros_like(input_ids)
        B, NA = input_ids.shape[0], self.num_answers
        packed = isinstance(attention_mask, MaskSpec) and attention_mask.lens_host is not None
        with torch.enable_grad() if packed else torch.no_grad():
            st = eng.forward(vis_feats, vis_pe, input_ids, token_type_ids, attention_mask, None, False, False, True)
        self.last_vqa_logits = eng.vqa_logits(st)
        dev = input_ids.device
        ans_idx = torch.empty(B, dtype=torch.long, device=dev)
        ans_logit = torch.empty(B, dtype=torch.float32, device=dev)
        ans_score = None
        if answers is not None:
            if not isinstance(answers, SparseAnswers):
                raise TypeError("answer(answers=...) takes a vlp_amd.input_prep.SparseAnswers")
            answers.check(B, NA)
            ans_score = torch.empty(B, dtype=torch.float32, device=dev)
            K.vqa_answer_rows(st.ws["vq_logits"], st.ws["NAp"], B, NA, 1, ans_idx, ans_logit, answers.idx.contiguous(), answers.score.contiguous(), ans_score)
        else:
            K.vqa_answer_rows(st.ws["vq_logits"], st.ws["NAp"], B, NA, 1, ans_idx, ans_logit)
        return ans_idx, ans_logit, ans_score


class BertForSeq2SeqDecoder(PreTrainedBertModel):
    """Incremental caption decoder (:1147-1494): same parameter tree as BertForPreTrainingLossMask (checkpoint compatible);
    greedy decoding (:1189-1253) and beam search (:1255-1494) run on the HIP engine with per-layer K/V caches
    (Engine.decode_greedy / Engine.decode_beam); the host keeps only the back-tracking of the frames (n-gram blocking runs on the
    device; the reference's host loop over python lists remains as ngram_blocking="host").  sample_mode='sample' draws with the library's counter-based RNG; in train() mode with gradients enabled
    it also returns differentiable log-probabilities (SCST, run_img2txt_dist.py:506-507): a teacher-forced scoring pass of the sampled ids on
    the training engine (Engine.score_samples), without dropout."""
    tasks = "img2txt"
    # forbid_duplicate_ngrams with ngram_size >= 2: "device" = Engine.decode_beam(ngram=...) (vlp_ngram_candidates / vlp_logsoftmax_topk_list, no
    # host round trip, token steps replayed from captured graphs); "host" = the _ngram_blocker closure (A/B and fallback).  Same results.
    ngram_blocking = "device"
    # where beam_search turns the frames into hypotheses: "host" = _backtrack_batch (numpy, one device -> host copy of the frames, the best
    # hypothesis only); "device" = Engine.beam_nbest (vlp_beam_nbest: ranked n-best list, no copy).  n_best > 1 always takes the device.
    backtrack = "host"
    # beam_groups > 1 (diverse beam search): "device" = vlp_beam_select_groups in every frame, steps captured / replayed; "host" =
    # vlp_amd.diverse.beam_select_groups_host with a round trip per frame (A/B and fallback).  Same results.
    group_select = "device"
    # constraints= (constrained beam search): "device" = vlp_logsoftmax_topk_want + vlp_beam_select_constrained in every frame, steps captured /
    # replayed; "host" = vlp_amd.constrained.beam_select_constrained_host with a round trip per frame (A/B and fallback).  Same results.
    constrained_select = "device"

    def __init__(self, config, mask_word_id=0, num_labels=2, search_beam_size=1, length_penalty=1.0, eos_id=0,
                 forbid_duplicate_ngrams=False, forbid_ignore_set=None, ngram_size=3, min_len=0, enable_butd=False, len_vis_input=49,
                 allow_random_fc7=True, n_best=1, beam_groups=1, diversity_penalty=0.0):
        super(BertForSeq2SeqDecoder, self).__init__(config)
        self.bert = BertModelIncr(config)
        self.cls = BertPreTrainingHeads(config, self.bert.embeddings.word_embeddings.weight, num_labels=num_labels)
        self.apply(self.init_bert_weights)
        self.mask_word_id, self.num_labels, self.len_vis_input = mask_word_id, num_labels, len_vis_input
        self.search_beam_size, self.length_penalty, self.eos_id = search_beam_size, length_penalty, eos_id
        self.forbid_duplicate_ngrams, self.forbid_ignore_set, self.ngram_size, self.min_len = forbid_duplicate_ngrams, forbid_ignore_set, ngram_size, min_len
        self.n_best = int(n_best)
        if self.n_best < 1 or self.n_best > max(int(search_beam_size), 1):
            raise ValueError("n_best=%d: the n-best list of a beam search holds 1..search_beam_size (%d) hypotheses" % (self.n_best, search_beam_size))
        self.beam_groups, self.diversity_penalty = int(beam_groups), float(diversity_penalty)
        self._check_groups(int(search_beam_size))
        _region_embedders(self, config, enable_butd, allow_random_fc7)
        self.__dict__["_engine"] = Engine(self)
        for prm in self.parameters():
            prm._vlp_owner = self.__dict__["_engine"]

    @property
    def engine(self):
        return self.__dict__["_engine"]

    def _check_groups(self, K):
        """beam_groups = G / diversity_penalty = lambda of a diverse beam search (vlp_amd.diverse): G = 1 with lambda = 0 is the plain search of
        any beam size; G > 1 needs a beam search whose size G divides, and a finite lambda >= 0."""
        G, lam = self.beam_groups, self.diversity_penalty
        ok = lam == lam and 0.0 <= lam < float("inf") and G >= 1
        if ok and G == 1 and lam == 0.0:
            return
        if not ok or G == 1 or K < 2 or G > K or K % G != 0:
            raise ValueError("beam_groups=%d, diversity_penalty=%r: a diverse beam search needs search_beam_size (%d) >= 2, beam_groups in "
                             "1..search_beam_size and dividing it, and a finite diversity_penalty >= 0 that is 0 unless beam_groups >= 2" % (G, lam, K))

    def forward(self, vis_feats, vis_pe, input_ids, token_type_ids, position_ids, attention_mask, task_idx=None, sample_mode="greedy",
                n_samples=1, temperature=1.0, top_k=0, top_p=1.0, return_entropy=False, constraints=None):
        """Returns (output_ids [B, n], output_probs [B, n]) with n = token_type_ids.shape[1] - input_ids.shape[1], as :1253.
        output_probs are the maximal prediction scores (logits), exactly what the reference returns in greedy mode (:1228).
        n_samples = K > 1 with sample_mode='sample' (not in the reference): K draws per image, returned sample-major as [K*B, n] ids and
        log-probabilities (row k*B + b is sample k of image b; Engine.decode_sample_group); in train() mode with gradients enabled the
        log-probabilities are differentiable, scored as K*B independent sequences.
        temperature / top_k / top_p (not in the reference; sample_mode='sample' without beam search): any value other
        than (1, 0, 1) draws every token from softmax(logits / temperature) restricted to the top_k largest logits (0 = all; ties kept) and
        then to the smallest set of largest logits holding a mass of top_p (vlp_sample_rows_filtered, Engine.decode_sample_group for every
        n_samples >= 1); the second output is the log-probability under that distribution.  (1, 0, 1) changes nothing.  In train() mode
        with gradients enabled a temperature alone (top_k 0, top_p 1) is the tempered policy of SCST: the ids are that decode's and the
        log-probabilities are softmax(logits / temperature)'s, differentiable through the tempered scoring pass (vlp_token_policy_fwd /
        _bwd); top_k / top_p stay refused there.
        return_entropy=True (train() mode with gradients and sample_mode='sample' only): returns (ids, logp, entropy), all [rows, n]; entropy
        is the sampled policy's entropy at every position, a second differentiable output of the same scoring pass.
        constraints (beam search only, see beam_search): phrases every image's caption must mention; per-call data, hence a keyword here."""
        if constraints is not None and (self.search_beam_size < 2 or sample_mode != "greedy" or n_samples != 1 or return_entropy):
            raise ValueError("constraints steer a beam search: they need search_beam_size >= 2 and take no sampling arguments")
        if not input_ids.is_cuda:
            raise RuntimeError("vlp_amd: the decoder runs on the HIP engine only (inputs must be on the GPU); there is no CPU path")
        n_samples = int(n_samples)
        temperature, top_k, top_p = float(temperature), int(top_k), float(top_p)
        if not (0.0 < temperature < float("inf")) or top_k < 0 or top_k >= 1 << 31 or not (0.0 < top_p <= 1.0):
            raise ValueError("temperature must be finite and > 0, top_k >= 0 and 0 < top_p <= 1 (got %r, %r, %r)" % (temperature, top_k, top_p))
        if (temperature, top_k, top_p) != (1.0, 0, 1.0):
            what = "temperature=%g, top_k=%d, top_p=%g" % (temperature, top_k, top_p)
            if sample_mode != "sample":
                raise ValueError("%s shape the distribution sample_mode='sample' draws from; sample_mode is %r" % (what, sample_mode))
            if self.search_beam_size > 1:
                raise ValueError("%s with search_beam_size=%d: beam search is not filtered" % (what, self.search_beam_size))
            if n_samples < 1:
                raise ValueError("n_samples=%d: n_samples >= 1" % n_samples)
            if self.training and torch.is_grad_enabled():
                if (top_k, top_p) != (0, 1.0):
                    raise ValueError("%s in train() mode with gradients enabled: the scoring pass differentiates the unfiltered log-softmax, a "
                                     "policy gradient of the filtered draw would be wrong; call under eval() or torch.no_grad()" % what)
                return self._sample_scored(vis_feats, vis_pe, input_ids, token_type_ids, position_ids, attention_mask, n_samples, temperature,
                                           return_entropy, group=True)
            if return_entropy:
                raise ValueError("return_entropy=True needs train() mode with gradients enabled (the entropy comes from the scoring pass)")
            with torch.no_grad():
                return self.engine.decode_sample_group(vis_feats, vis_pe, input_ids, token_type_ids, position_ids, attention_mask, self.mask_word_id,
                                                       n_samples, temperature=temperature, top_k=top_k, top_p=top_p)
        if return_entropy:
            if sample_mode != "sample" or self.search_beam_size > 1 or not (self.training and torch.is_grad_enabled()):
                raise ValueError("return_entropy=True needs sample_mode='sample' without beam search in train() mode with gradients enabled (the "
                                 "entropy is that of the sampled policy, computed by the scoring pass)")
            if n_samples < 1:
                raise ValueError("n_samples=%d: n_samples >= 1" % n_samples)
            return self._sample_scored(vis_feats, vis_pe, input_ids, token_type_ids, position_ids, attention_mask, n_samples, 1.0, True,
                                       group=n_samples != 1)
        if n_samples != 1:
            if n_samples < 1 or sample_mode != "sample":
                raise ValueError("n_samples=%d needs sample_mode='sample' and n_samples >= 1" % n_samples)
            if self.search_beam_size > 1:
                raise ValueError("n_samples=%d with search_beam_size=%d: several samples per image are drawn, not searched" %
                                 (n_samples, self.search_beam_size))
            if self.training and torch.is_grad_enabled():
                return self._sample_scored(vis_feats, vis_pe, input_ids, token_type_ids, position_ids, attention_mask, n_samples, 1.0, False,
                                           group=True)
            with torch.no_grad():
                return self.engine.decode_sample_group(vis_feats, vis_pe, input_ids, token_type_ids, position_ids, attention_mask,
                                                       self.mask_word_id, n_samples)
        if self.search_beam_size > 1:
            with torch.no_grad():
                return self.beam_search(vis_feats, vis_pe, input_ids, token_type_ids, position_ids, attention_mask, task_idx=task_idx,
                                        constraints=constraints)
        if sample_mode not in ("greedy", "sample"):
            raise NotImplementedError("sample_mode=%r (the reference knows 'greedy' and 'sample', modeling.py:1227-1237)" % (sample_mode,))
        if sample_mode == "sample" and self.training and torch.is_grad_enabled():
            # SCST (run_img2txt_dist.py:505-507): draw on the K/V-cache decoder, then score the drawn ids with one training forward whose
            # [MASK] slots see exactly the decoder's hidden states; the log-probs' backward is that forward's backward
            return self._sample_scored(vis_feats, vis_pe, input_ids, token_type_ids, position_ids, attention_mask, 1, 1.0, False, group=False)
        with torch.no_grad():
            return self.engine.decode_greedy(vis_feats, vis_pe, input_ids, token_type_ids, position_ids, attention_mask, self.mask_word_id,
                                             sample=(sample_mode == "sample"))

    def _sample_scored(self, vis_feats, vis_pe, input_ids, token_type_ids, position_ids, attention_mask, n_samples, temperature, entropy, group):
        """SCST, every form of it (temperature 1 and entropy False: the plain one): draw n_samples captions per image from softmax(logits / temperature)
        (group: Engine.decode_sample_group, the captured path; else decode_greedy(sample=True), the draw of a plain one-sample call), then
        score them under the same policy.  Returns (ids, logp) or (ids, logp, entropy), the last two differentiable."""
        eng = self.engine
        with torch.no_grad():
            if group:
                ids, _ = eng.decode_sample_group(vis_feats, vis_pe, input_ids, token_type_ids, position_ids, attention_mask, self.mask_word_id,
                                                 n_samples, temperature=temperature)
            else:
                ids, _ = eng.decode_greedy(vis_feats, vis_pe, input_ids, token_type_ids, position_ids, attention_mask, self.mask_word_id, sample=True)

        def tiled(t):                        # row k*B + b of the scoring batch is image b
            return t if n_samples == 1 else t.repeat(n_samples, *([1] * (t.dim() - 1)))
        out = eng.score_samples(tiled(vis_feats), tiled(vis_pe), tiled(input_ids), tiled(token_type_ids), tiled(position_ids),
                                tiled(attention_mask), ids, self.mask_word_id, temperature=temperature, entropy=entropy)
        if not entropy:
            return ids, _LogprobFn.apply(eng._anchor, out[1], eng, out[0])
        logp, ent = _LogprobFn.apply(eng._anchor, out[1], eng, out[0], out[2])
        return ids, logp, ent

    def score(self, vis_feats, vis_pe, input_ids, token_type_ids, position_ids, attention_mask, caption_ids, lengths=None):
        """How probable given captions are under this checkpoint (not in the reference): caption r is scored against image row r, teacher
        forced, in one pass over all positions (Engine.score_captions).  caption_ids: R token id lists, or a padded [R, W] tensor with
        lengths [R]; vlp_amd.caption_score.counted_positions says which of the n = token_type_ids.shape[1] - input_ids.shape[1] positions
        count (the caption's tokens and its closing [SEP], eos_id; a caption of >= n tokens is cut and has none).
        Returns (logp f32, entropy f32, rank int32, top_id int64, counted bool), each [R, n]: the log-probability of the caption's token,
        the entropy of the model's distribution, the token's rank in it (0: the model's first choice) and that first choice; (0, 0, -1, -1)
        where counted is False.  Inference only: refused in train() mode with gradients enabled."""
        from .caption_score import counted_positions
        if not input_ids.is_cuda:
            raise RuntimeError("vlp_amd: the decoder runs on the HIP engine only (inputs must be on the GPU); there is no CPU path")
        n = token_type_ids.shape[1] - input_ids.shape[1]
        ids, counted, _ = counted_positions(caption_ids, n, self.eos_id, lengths, vocab_size=self.config.vocab_size)
        dev = input_ids.device
        out = self.engine.score_captions(vis_feats, vis_pe, input_ids, token_type_ids, position_ids, attention_mask, ids.to(dev), self.mask_word_id)
        return out + (counted.to(dev),)

    # ---- beam search: host side (what the reference also does on the host) -------------------------------
    def _ngram_blocker(self, batch_size, vocab_size):
        """Stateful callback for Engine.decode_beam: tracks the partial hypotheses (:1367-1384) and returns the uint8 [B*K, V] mask
        of words that would repeat an n-gram (:1386-1430), or None."""
        import numpy as np
        K, n, ignore = self.search_beam_size, self.ngram_size, self.forbid_ignore_set
        state = {"seqs": None}

        def repeats(seq):
            if len(seq) < n:
                return ()
            tail = seq[len(seq) - (n - 1):]
            if ignore and any(t in ignore for t in tail):
                return ()
            hits = set()
            for i in range(len(seq) - (n - 1)):
                if seq[i:i + n - 1] == tail:
                    nxt = seq[i + n - 1]
                    if not (ignore and nxt in ignore):
                        hits.add(nxt)
            return hits

        def step(ids, back, first):
            if first:
                state["seqs"] = [[ids[b][k]] for b in range(batch_size) for k in range(K)]
            else:
                old = state["seqs"]
                state["seqs"] = [old[b * K + back[b][k]] + [ids[b][k]] for b in range(batch_size) for k in range(K)]
            seqs = state["seqs"]
            if len(seqs[0]) < n:
                return None
            hits = [repeats(sq) for sq in seqs]
            if not any(hits):
                return None
            mask = np.zeros((batch_size * K, vocab_size), dtype=np.uint8)
            for r, hs in enumerate(hits):
                for w in hs:
                    mask[r, w] = 1
            return mask
        return step

    def beam_search(self, vis_feats, vis_pe, input_ids, token_type_ids, position_ids, attention_mask, task_idx=None, constraints=None):
        """Returns the reference's traces dict (:1436-1494): 'pred_seq' [B, L] (0 padded), 'scores' f32 / 'wids' / 'ptrs' [B, L, K]
        (frames padded with zeros to the output length L), on the input device.
        With n_best = N > 1 or backtrack = "device" the hypotheses come from vlp_beam_nbest (Engine.beam_nbest; the rule is
        vlp_amd.nbest.beam_nbest_host's, rank 0 the hypothesis of the host path) and nothing is copied to the host; the dict then also carries
        the ranked list of every image: 'nbest_seq' [B, N, L], 'nbest_score' f32 (cumulative log-probability) / 'nbest_value' f64 (score +
        length_penalty * length) / 'nbest_len' int32 / 'nbest_ok' uint8 [B, N] (0: a hypothesis that went on after its eos, or an empty one).
        With beam_groups = G > 1 the frames are those of a diverse beam search (vlp_amd.diverse: G groups of K / G beams, diversity_penalty per
        earlier pick of the same word in a frame); the scores stay unpenalised log-probabilities, so everything above keeps its meaning.
        constraints (not in the reference; vlp_amd.constrained is the rule): phrases the caption of every image must mention, as a
        (cons_ids [B, C, Lc], cons_len [B, C]) pair or a list, one entry per image, of lists of word-piece id lists (<= 8 phrases of <= 8
        pieces).  The frames are then those of a constrained beam search and the dict also carries 'cons_state' int32 [B, L, K] (every beam's
        constraint state, zero padded like the frames), 'pred_met' int32 [B] (the met mask of pred_seq; bit c: phrase c is mentioned) and,
        with n_best > 1, 'nbest_met' int32 [B, N]: constrained.constraints_met of the returned sequences, computed on the host.
        beam_groups > 1 is refused.  constraints=None is the search as it is."""
        B, out_len = input_ids.shape[0], token_type_ids.shape[1]
        K = self.search_beam_size
        cons = None
        if constraints is not None:
            from . import constrained as CB
            if self.constrained_select not in ("device", "host"):
                raise ValueError("constrained_select must be 'device' or 'host', got %r" % (self.constrained_select,))
            if self.beam_groups > 1:
                raise ValueError("constraints and beam_groups=%d (diverse beam search) exclude each other" % self.beam_groups)
            if isinstance(constraints, (tuple, list)) and len(constraints) == 2 and all(hasattr(t, "shape") for t in constraints):
                cons = constraints
            else:
                cons = CB.pack_constraints(constraints, B)
            cons = CB.check_constraints(cons[0], cons[1], self.config.vocab_size, self.eos_id)
        if self.backtrack not in ("device", "host"):
            raise ValueError("backtrack must be 'device' or 'host', got %r" % (self.backtrack,))
        if not 1 <= self.n_best <= K:
            raise ValueError("n_best=%d: the n-best list of a beam search holds 1..search_beam_size (%d) hypotheses" % (self.n_best, K))
        self._check_groups(K)
        if self.group_select not in ("device", "host"):
            raise ValueError("group_select must be 'device' or 'host', got %r" % (self.group_select,))
        forbid_fn = ngram = None
        if self.forbid_duplicate_ngrams:
            if self.ngram_blocking not in ("device", "host"):
                raise ValueError("ngram_blocking must be 'device' or 'host', got %r" % (self.ngram_blocking,))
            if self.ngram_blocking == "device" and self.ngram_size >= 2:
                ngram = (self.ngram_size, self.forbid_ignore_set)
            else:                    # ngram_size == 1 (the reference's seq[-0:] quirk) stays on the host
                forbid_fn = self._ngram_blocker(B, self.config.vocab_size)
        kw = dict(groups=self.beam_groups, diversity=self.diversity_penalty, group_select=self.group_select) if self.beam_groups > 1 else {}
        if cons is not None:
            kw = dict(constraints=cons, constrained_select=self.constrained_select)
        res = self.engine.decode_beam(vis_feats, vis_pe, input_ids, token_type_ids, position_ids, attention_mask, self.mask_word_id,
                                      K, self.eos_id, min_len=self.min_len, forbid_fn=forbid_fn, ngram=ngram, **kw)
        tot, wids, ptrs = res[:3]
        frames = tot.shape[0]
        dev = input_ids.device

        def with_constraints(out):
            """The constrained search's extra entries: the state frames, and the met masks of the returned sequences (host)."""
            if cons is None:
                return out
            st = torch.zeros(B, out_len, K, dtype=torch.int32, device=dev)
            st[:, :frames] = res[3].permute(1, 0, 2)
            out["cons_state"] = st

            def met(seqs):                   # [B, n, L] -> int32 [B, n]
                a = seqs.cpu().numpy()
                return torch.tensor([[CB.constraints_met(a[b, n], cons[0][b], cons[1][b], eos_id=self.eos_id) for n in range(a.shape[1])]
                                     for b in range(B)], dtype=torch.int32, device=dev)
            out["pred_met"] = met(out["pred_seq"][:, None])[:, 0]
            if "nbest_seq" in out and self.n_best > 1:
                out["nbest_met"] = met(out["nbest_seq"])
            return out
        # frames stay on the device: [frames, B, K] -> [B, out_len, K], zero padded (three small launches; no per-sample host loop)
        scores = torch.zeros(B, out_len, K, dtype=torch.float32, device=dev)
        wid_o = torch.zeros(B, out_len, K, dtype=torch.long, device=dev)
        ptr_o = torch.zeros(B, out_len, K, dtype=torch.long, device=dev)
        scores[:, :frames] = tot.permute(1, 0, 2)
        wid_o[:, :frames] = wids.permute(1, 0, 2)
        ptr_o[:, :frames] = ptrs.permute(1, 0, 2)
        if self.n_best > 1 or self.backtrack == "device":
            from .nbest import by_image
            N = self.n_best
            seq, score, value, length, ok = self.engine.beam_nbest(tot, wids, ptrs, N, self.eos_id, self.length_penalty, out_len)
            out = {"pred_seq": seq[:B].clone(), "scores": scores, "wids": wid_o, "ptrs": ptr_o}     # (copies: the workspace keeps the kernel's rows)
            for name, t in (("nbest_seq", seq), ("nbest_score", score), ("nbest_value", value), ("nbest_len", length), ("nbest_ok", ok)):
                out[name] = by_image(t, N).clone(memory_format=torch.contiguous_format)
            return with_constraints(out)
        # best hypothesis of every sample (:1446-1474), vectorised over the batch on the host: ONE device -> host copy of the three frame tensors
        pred = self._backtrack_batch(tot.cpu().numpy(), wids.cpu().numpy(), ptrs.cpu().numpy(), out_len)
        return with_constraints({"pred_seq": torch.from_numpy(pred).to(dev), "scores": scores, "wids": wid_o, "ptrs": ptr_o})

    def _backtrack_batch(self, scores, words, back, out_len):
        """The best hypothesis (:1446-1474) of all samples at once (numpy; arrays [frames, B, K]) -> int64 [B, out_len], 0 padded: candidates are the
        hypotheses that emitted eos, or any hypothesis of the last valid frame (the first frame whose K words are all eos, else the final one);
        rank by cumulative log-probability + length_penalty * (frame + 1), first maximum in (frame, beam) order; follow the back pointers."""
        import numpy as np
        F, B, K = scores.shape
        eos, lp = self.eos_id, self.length_penalty
        all_eos = (words == eos).all(axis=2)                                   # [F, B]
        last = np.where(all_eos.any(axis=0), all_eos.argmax(axis=0), F - 1)    # [B]
        f_idx = np.arange(F)[:, None, None]
        cand = (f_idx <= last[None, :, None]) & ((words == eos) | (f_idx == last[None, :, None]))
        val = np.where(cand, scores.astype(np.float64) + lp * (f_idx + 1), -np.inf)      # [F, B, K]
        flat = val.transpose(1, 0, 2).reshape(B, F * K)
        best = flat.argmax(axis=1)                                             # first maximum in (frame, beam) order, as the reference's strict `>` scan
        ok = np.isfinite(flat[np.arange(B), best])
        bf, bk = best // K, best % K
        out = np.zeros((B, out_len), dtype=np.int64)
        rows = np.arange(B)
        k = bk.copy()
        for t in range(F - 1, -1, -1):
            live = ok & (t <= bf)
            out[live, t] = words[t, rows, k][live]
            if t > 0:
                k = np.where(live, back[t, rows, k], k)
        return out
