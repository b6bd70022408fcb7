"""What the training step launches and computes, as a text listing two trees can be diffed on: an A/B of host-code changes under the same
libvlp_hip.so (VLP_HIP_LIB).  The training-step sibling of tools/decode_trace.py.

    python tools/step_trace.py [--tree DIR] [--digest]  >  listing   (DIR: the checkout whose vlp_amd / oracle / tests are imported; default: this one)

2 layers, hidden 768, vocabulary 1024, 100 regions, label smoothing on for img2txt: the smallest shapes at which each path of the step is
taken.  max_len_b 21 gives L = 21 + 100 + 3 = 124 (synthetic.seq_len), so B = 24 has M = 24 x 124 = 2976 >= 2048 rows (grouped and mapped
layer wgrads, grouped region wgrads) and B = 4 keeps split-M.
Every case runs TWO consecutive steps (forward, loss, backward; zero_grad between them unless the case accumulates; another batch each
step) on a fresh model with step_seed fixed, and prints
  * every C call of the two steps (_lib.record()): function name and every integer / float argument and structure field in order; pointers
    and the stream are numbered by first appearance within the case, so the listing shows which launches share a buffer or a stream, not
    where the allocator put them (the tensors of these calls are kept alive to the end of the case, so that no number stands for two);
  * after each step the SHA-256 of the losses, the logits and every param.grad.
--digest prints, in place of the call lines of a case, their number, the SHA-256 of exactly those lines and the number of calls per
function, and in place of a step's gradient lines their number and the SHA-256 of exactly those lines: the form that is kept as a record
(the full listings of two trees are what gets diffed).
Only interfaces that older trees have as well are used: the models' forward, Engine.score_samples / backward(task="logprob"), zero_grad,
_lib.record(), engine._ws."""
import argparse
import ctypes as C
import gc
import hashlib
import os
import sys

ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("--tree", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
ap.add_argument("--digest", action="store_true")
ARGS = ap.parse_args()
sys.path.insert(0, os.path.abspath(ARGS.tree))

import torch  # noqa: E402

from oracle import vlp_oracle as O  # noqa: E402
from tests.decode_seq_util import varied_inputs  # noqa: E402
from vlp_amd import _lib as K  # noqa: E402
from vlp_amd import synthetic as S  # noqa: E402
from vlp_amd.modeling import BertConfig, BertForPreTrainingLossMask, BertForSeq2SeqDecoder  # noqa: E402

DEV = torch.device("cuda:0")
V, NV, NL, T = 1024, 100, 2, 6
SWITCHES = ("VLP_LAST_LAYER_LIVE", "VLP_WGRAD_KEPT")


def train_cases():
    """(name, tasks, packed, mask_image_regions, B, dropout, environment, accumulate)"""
    for tasks in ("img2txt", "vqa2"):
        for packed in (False, True):
            for mir in (False, True):
                for B in (24, 4):
                    yield ("%s %s%s B=%d" % (tasks, "packed" if packed else "dense", " mask_image_regions" if mir else "", B),
                           tasks, packed, mir, B, 0.0, {}, False)
    for tasks in ("img2txt", "vqa2"):
        for packed in (False, True):
            yield "%s %s B=24 dropout 0.1" % (tasks, "packed" if packed else "dense"), tasks, packed, False, 24, 0.1, {}, False
    for sw in SWITCHES:
        yield "img2txt dense B=24 %s=0" % sw, "img2txt", False, False, 24, 0.0, {sw: "0"}, False
    for B in (24, 4):
        yield "img2txt dense B=%d accumulating" % B, "img2txt", False, False, B, 0.0, {}, True
    yield "img2txt packed B=24 dropout 0.1 accumulating", "img2txt", True, False, 24, 0.1, {}, True


# (name, B, temperature, entropy)
SCST_CASES = [("scst B=3", 3, 1.0, False), ("scst B=24", 24, 1.0, False), ("scst B=3 T=0.7", 3, 0.7, False),
              ("scst B=3 T=0.7 entropy", 3, 0.7, True), ("scst B=3 entropy", 3, 1.0, True)]


class Numbering(object):
    def __init__(self):
        self.seen = {}

    def pointer(self, v):
        v = v.value if isinstance(v, C.c_void_p) else v
        return "null" if not v else "p%d" % self.seen.setdefault(v, len(self.seen))

    def value(self, v, ctype=None):
        if isinstance(v, C.c_void_p) or ctype is C.c_void_p:
            return self.pointer(v)
        if isinstance(v, C.Structure):
            return "{%s}" % ", ".join("%s=%s" % (f[0], self.value(getattr(v, f[0]), f[1])) for f in v._fields_)
        if isinstance(v, C.Array):
            return "[%s]" % ", ".join(self.value(x, v._type_) for x in v)
        if hasattr(v, "_obj"):                       # byref(structure)
            return self.value(v._obj)
        if hasattr(v, "contents"):                   # pointer(structure)
            return self.value(v.contents)
        if isinstance(v, (bool, int, float, bytes)) or v is None:
            return repr(v)
        if hasattr(v, "value"):                      # c_int(...), c_float(...)
            return repr(v.value)
        raise TypeError("step_trace: argument of type %s" % type(v))


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def print_calls(plan):
    num = Numbering()
    lines = ["  %4d %s(%s)" % (i, fn.__name__, ", ".join(num.value(x) for x in a)) for i, (fn, a) in enumerate(plan)]
    if ARGS.digest:
        names = [fn.__name__ for fn, _ in plan]
        lines = ["  launches %d sha256 %s" % (len(lines), hashlib.sha256("\n".join(lines).encode()).hexdigest()),
                 "  functions " + ", ".join("%s x %d" % (n, names.count(n)) for n in sorted(set(names)))]
    print("\n".join(lines))


def traced(name, m, steps):
    """Run steps(step) -> outputs for step 1, 2 with every C call recorded; print the calls, then the outputs of each step."""
    print("==== %s" % name)
    m.engine.step_seed = 1234
    keep, ptr, outs = [], K.ptr, []
    K.ptr = lambda t: (keep.append(t), ptr(t))[1]
    try:
        with K.record() as plan:
            for step in (1, 2):
                out = steps(step)
                torch.cuda.synchronize()
                # (hashed at once: step 2 overwrites the workspace views and, accumulating, the gradients)
                outs.append((step, {k: v.detach().clone() for k, v in out.items()}, {n: None if q.grad is None else q.grad.detach().clone()
                                                                                     for n, q in m.named_parameters()}, m.engine.step_seed))
    finally:
        K.ptr = ptr
    print_calls(plan)
    for step, out, grads, seed in outs:
        for k in sorted(out):
            print("  step %d %s %s %s" % (step, k, tuple(out[k].shape), sha(out[k])))
        lines = ["  step %d grad %s %s" % (step, n, "None" if g is None else sha(g)) for n, g in grads.items()]
        if ARGS.digest:
            lines = ["  step %d grads %d sha256 %s" % (step, len(lines), hashlib.sha256("\n".join(lines).encode()).hexdigest())]
        print("\n".join(lines))
        print("  step %d step_seed %d" % (step, seed))
    del keep, plan, outs
    gc.collect()
    torch.cuda.empty_cache()


def train_case(name, tasks, packed, mir, B, drop, env, accumulate, params):
    cfg = BertConfig(V, num_hidden_layers=NL, type_vocab_size=6, hidden_dropout_prob=drop, attention_probs_dropout_prob=drop,
                     label_smoothing=0.1 if tasks == "img2txt" else None)
    m = BertForPreTrainingLossMask(cfg, enable_butd=True, len_vis_input=NV, tasks=tasks, allow_random_fc7=True)
    sd = dict(params[tasks])
    sd["cls.predictions.decoder.weight"] = sd["bert.embeddings.word_embeddings.weight"]
    if m.crit_mask_lm_smoothed is not None:
        sd["crit_mask_lm_smoothed.one_hot"] = m.crit_mask_lm_smoothed.one_hot
    m.load_state_dict(sd, strict=True)
    m = m.half().to(DEV).train()
    m.engine.varlen = packed
    batches = [S.batch_to(S.make_batch(B, max_len_b=21, len_vis_input=NV, vocab_size=V, max_pred=3, s2s_prob=0.5, tasks=tasks, seed=70 + s,
                                       vis_mask_prob=0.25 if mir else 0.0), DEV, half=True) for s in (1, 2)]

    def steps(step):
        b = batches[step - 1]
        if step == 2 and not accumulate:
            m.engine.zero_grad()
        lt = m(b.img, b.vis_pe, b.input_ids, b.segment_ids, b.input_mask, b.lm_label_ids, b.ans_labels, b.is_next, masked_pos=b.masked_pos,
               masked_weights=b.masked_weights, task_idx=b.task_idx, vis_masked_pos=b.vis_masked_pos, mask_image_regions=mir, drop_worst_ratio=0)
        ((lt[0] + lt[1] + lt[2]).sum() * 256.0).backward()
        out = {"loss": torch.stack([x.detach().float().reshape(()) for x in lt]),
               "logits": m.last_vqa_logits if tasks == "vqa2" else m.last_mlm_logits}
        out["packed_rows"] = torch.tensor(m.engine.last_packed_rows or 0)
        return out

    old = {k: os.environ.get(k) for k in SWITCHES}
    os.environ.update(env)
    try:
        traced(name, m, steps)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def scst_case(name, B, temperature, entropy, params):
    cfg = BertConfig(V, num_hidden_layers=NL, type_vocab_size=6, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    m = BertForSeq2SeqDecoder(cfg, mask_word_id=S.MASK_ID, eos_id=S.SEP_ID, enable_butd=True, len_vis_input=NV)
    sd = dict(params["img2txt"])
    sd["cls.predictions.decoder.weight"] = sd["bert.embeddings.word_embeddings.weight"]
    m.load_state_dict(sd, strict=True)
    m = m.half().to(DEV).train()
    eng = m.engine
    g = torch.Generator().manual_seed(B)
    draws = []
    for s in (1, 2):
        t = varied_inputs(B, T, 200 + s, NV)
        draws.append(((t[0].half().to(DEV), t[1].half().to(DEV)) + tuple(x.to(DEV) for x in t[2:]),
                      torch.randint(5, V, (B, T), generator=g).to(DEV), torch.randn(B * T, generator=g).to(DEV) * 256.0,
                      torch.randn(B * T, generator=g).to(DEV) * 2.56))

    def steps(step):
        inp, ids, g_rows, h_rows = draws[step - 1]
        if step == 2:
            eng.zero_grad()
        res = eng.score_samples(*inp, ids, S.MASK_ID, temperature=temperature, entropy=entropy)
        out = {"logp": res[1].clone()}
        if entropy:
            out["entropy"] = res[2].clone()
        eng.backward(res[0], None, "logprob", g_rows=g_rows, h_rows=h_rows if entropy else None)
        return out

    traced(name, m, steps)


def main():
    params = {t: O.init_params(vocab_size=V, layers=NL, tasks=t, seed=21) for t in ("img2txt", "vqa2")}
    for case in train_cases():
        train_case(*case, params)
    for case in SCST_CASES:
        scst_case(*case, params)


if __name__ == "__main__":
    main()
