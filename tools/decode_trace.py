"""What the caption decoders launch and return, as a text listing two trees can be diffed on: an A/B of host-code changes under the same
libvlp_hip.so (VLP_HIP_LIB).

    python tools/decode_trace.py [--tree DIR] [--digest]  >  listing   (DIR: the checkout whose vlp_amd / oracle / tests are imported; default: this one)

Shapes of tests/test_46_decode_sequence_gpu.py: vocabulary 1024, 2 layers, hidden 768, 100 regions, B = 3 / T = 6, varied_inputs, the "peaked"
weights (the smallest at which the token steps take the fused path and beams meet eos).  Every case runs on a fresh model and prints
  * the C calls of call 1 (_lib.record(): calls 2 and 3 run inside a capture or replay one, and the engine's fallback must stay free to
    record): function name and every integer / float argument and structure field in order; pointers are numbered by first appearance
    within the case, so the listing shows which launches share a buffer, not where the allocator put it (the tensors of these
    calls are kept alive to the end of the call, so that no number stands for two of them);
  * for calls 1, 2, 3 (plain, capture, replay; other inputs each time) the SHA-256 of every returned tensor, of filter_cutoff / filter_kept
    [:T] of a filtered draw, and engine.step_seed.
--digest prints, in place of the ~140 call lines of a case, their number, the SHA-256 of exactly those lines and the number of calls per
function: the form that is kept as a record (the full listings of two trees are what gets diffed).
Only interfaces that older trees have as well are used: BertForSeq2SeqDecoder.forward and its attributes, _lib.record(), engine._ws."""
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
from vlp_amd.modeling import BertConfig, BertForSeq2SeqDecoder  # noqa: E402

DEV = torch.device("cuda:0")
V, NV, EOS, B, T = 1024, 100, S.SEP_ID, 3, 6
SAMPLE = dict(sample_mode="sample")
NGRAM = dict(search_beam_size=4, forbid_duplicate_ngrams=True, ngram_size=2, forbid_ignore_set=[EOS, 301])
GROUPS = dict(search_beam_size=4, beam_groups=2, diversity_penalty=0.5)
# (name, model attributes, forward keywords, samples per image of a filtered draw or None)
CASES = [("greedy", {}, {}, None),
         ("sampling greedy", {}, SAMPLE, None),
         ("samples K=1 T=0.7", {}, dict(SAMPLE, n_samples=1, temperature=0.7), 1),
         ("samples K=3", {}, dict(SAMPLE, n_samples=3), None),
         ("samples K=3 T=0.8 k=20 p=0.9", {}, dict(SAMPLE, n_samples=3, temperature=0.8, top_k=20, top_p=0.9), 3),
         ("beam 3", dict(search_beam_size=3), {}, None),
         ("beam 3 min_len=3", dict(search_beam_size=3, min_len=3), {}, None),
         ("beam 4 ngram 2 + ignore list, device", dict(NGRAM, ngram_blocking="device"), {}, None),
         ("beam 4 ngram 2 + ignore list, host", dict(NGRAM, ngram_blocking="host"), {}, None),
         ("beam 4 groups 2, device", dict(GROUPS, group_select="device"), {}, None),
         ("beam 4 groups 2, host", dict(GROUPS, group_select="host"), {}, None),
         ("beam 3 n_best=3", dict(search_beam_size=3, n_best=3), {}, None)]


def peaked_params():
    p = O.init_params(vocab_size=V, layers=2, tasks="img2txt", seed=46, std=0.05)
    p["cls.predictions.bias"][300:306] = 8.0
    p["cls.predictions.bias"][EOS] = 7.0
    return p


def fresh_model(p, attrs):
    cfg = BertConfig(V, num_hidden_layers=2, type_vocab_size=6, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    m = BertForSeq2SeqDecoder(cfg, mask_word_id=S.MASK_ID, eos_id=EOS, enable_butd=True, len_vis_input=NV)
    sd = dict(p)
    sd["cls.predictions.decoder.weight"] = p["bert.embeddings.word_embeddings.weight"]
    m.load_state_dict(sd, strict=True)
    for k, v in attrs.items():
        setattr(m, k, v)
    return m.half().to(DEV).eval()


def inputs(seed):
    t = varied_inputs(B, T, seed, NV)
    return (t[0].half().to(DEV), t[1].half().to(DEV)) + tuple(x.to(DEV) for x in t[2:])


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
        raise TypeError("decode_trace: argument of type %s" % type(v))


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def main():
    p = peaked_params()
    for name, attrs, kw, filtered in CASES:
        m = fresh_model(p, attrs)
        print("==== %s" % name)
        for call in (1, 2, 3):
            args = inputs(100 + call)
            with torch.no_grad():
                if call == 1:
                    # every tensor a C call of call 1 sees stays alive until the call is over: a pointer number then never stands for two
                    # tensors (which freed temporary a fresh buffer would reuse follows the allocator's free lists, not the host code)
                    keep, ptr = [], K.ptr
                    K.ptr = lambda t: (keep.append(t), ptr(t))[1]
                    try:
                        with K.record() as plan:
                            res = m(*args, task_idx=None, **kw)
                    finally:
                        K.ptr = ptr
                    del keep
                    num = Numbering()
                    lines = ["  %4d %s(%s)" % (i, fn.__name__, ", ".join(num.value(x) for x in a)) for i, (fn, a) in enumerate(plan)]
                    if ARGS.digest:
                        names = [fn.__name__ for fn, _ in plan]
                        lines = ["  call 1 launches %d sha256 %s" % (len(lines), hashlib.sha256("\n".join(lines).encode()).hexdigest()),
                                 "  call 1 functions " + ", ".join("%s x %d" % (n, names.count(n)) for n in sorted(set(names)))]
                    print("\n".join(lines))
                else:
                    res = m(*args, task_idx=None, **kw)
            torch.cuda.synchronize()
            out = dict(res) if isinstance(res, dict) else dict(zip(("ids", "values"), res))
            if filtered is not None:
                ws = m.engine._ws[("dec", B, NV + 3, NV + 2 + T, filtered, "group")]
                out.update(filter_cutoff=ws["filter_cutoff"][:T], filter_kept=ws["filter_kept"][:T])
            for k in sorted(out):
                print("  call %d %s %s %s" % (call, k, tuple(out[k].shape), sha(out[k])))
            print("  call %d step_seed %d" % (call, m.engine.step_seed))
        del m                         # (a model and its engine refer to each other: collected here, not at some later point)
        gc.collect()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
