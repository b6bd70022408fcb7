"""CPU: host logic and the C-ABI boundary (no compute calls -- there is no GPU here)."""
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    from vlp_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "vlp_hip.h")).read()
    declared = set(re.findall(r"\b(vlp_[a-z0-9_]+)\s*\(", header))
    declared -= {"vlp_status"}
    assert declared, "no declarations parsed"
    for name in declared:
        assert hasattr(lib, name), "libvlp_hip.so does not export %s" % name
    assert declared == set(_lib.SYMBOLS.keys()), declared ^ set(_lib.SYMBOLS.keys())
    assert lib.vlp_version() == 5
    # exported symbols visible to a plain dynamic loader (what a cgo/JNI/ctypes binding would see)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (vlp_[a-z0-9_]+)", out))
    assert declared <= exported
    assert exported <= declared, "exported but not declared in include/vlp_hip.h: %s" % sorted(exported - declared)
    assert lib.vlp_lab_build() == 0, "the product library must not be an investigation (-DVLP_LAB_BUILD) build"


def test_ctypes_structs_match_c_layout(tmp_path):
    """sizeof/offsetof of every argument struct, as seen by gcc, equal the ctypes mirror."""
    from vlp_amd import _lib
    structs = {"vlp_gemm_nt_args": _lib.GemmNtArgs, "vlp_gemm_tn_args": _lib.GemmTnArgs, "vlp_colsum_args": _lib.ColsumArgs,
               "vlp_attn_fwd_args": _lib.AttnFwdArgs, "vlp_attn_bwd_args": _lib.AttnBwdArgs, "vlp_layernorm_fwd_args": _lib.LayerNormFwdArgs,
               "vlp_layernorm_bwd_args": _lib.LayerNormBwdArgs, "vlp_embed_fwd_args": _lib.EmbedFwdArgs, "vlp_embed_bwd_args": _lib.EmbedBwdArgs,
               "vlp_mlm_loss_fwd_args": _lib.MlmLossFwdArgs, "vlp_mlm_loss_bwd_args": _lib.MlmLossBwdArgs,
               "vlp_fused_adam_args": _lib.FusedAdamArgs, "vlp_bert_adam_args": _lib.BertAdamArgs,
               "vlp_transpose_desc": _lib.TransposeDesc, "vlp_attn_decode_args": _lib.AttnDecodeArgs, "vlp_beam_select_args": _lib.BeamSelectArgs, "vlp_vis_pe_prep_args": _lib.VisPePrepArgs,
               "vlp_pretext_fwd_args": _lib.PretextFwdArgs, "vlp_pretext_bwd_args": _lib.PretextBwdArgs,
               "vlp_dec_gemm_args": _lib.DecGemmArgs, "vlp_dec_reduce_ln_args": _lib.DecReduceLnArgs}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "vlp_hip.h"', "int main(void) {"]
    for cname, st in structs.items():
        lines.append('printf("%s %%zu", sizeof(%s));' % (cname, cname))
        for fname, _ in st._fields_:
            lines.append('printf(" %%zu", offsetof(%s, %s));' % (cname, fname))
        lines.append('printf("\\n");')
    lines.append("return 0; }")
    src = os.path.join(tmp_path, "layout.c")
    open(src, "w").write("\n".join(lines))
    exe = os.path.join(tmp_path, "layout")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.strip().splitlines()
    for line in out:
        parts = line.split()
        st = structs[parts[0]]
        assert int(parts[1]) == ctypes.sizeof(st), parts[0]
        offs = [int(x) for x in parts[2:]]
        assert offs == [getattr(st, f).offset for f, _ in st._fields_], parts[0]


def test_no_cpu_fallback():
    from vlp_amd import _lib
    x = torch.zeros(8, 64, dtype=torch.half)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _lib.gemm_nt(x, x, x, 8, 8, 64)
    from vlp_amd.modeling import BertConfig, BertForPreTrainingLossMask
    m = BertForPreTrainingLossMask(BertConfig(128, num_hidden_layers=1, type_vocab_size=6), enable_butd=True, len_vis_input=100,
                                   allow_random_fc7=True)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.engine.pack()
    # product code never imports the oracle
    for root, _, files in os.walk(os.path.join(ROOT, "vlp_amd")):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(root, f)).read()
                assert "oracle" not in re.sub(r'""".*?"""', "", src, flags=re.S).replace("# checker", ""), f


def test_model_surface_matches_reference_contract():
    """Class / kwarg / state_dict-key contract of SURVEY.md 8(b)."""
    import inspect
    from oracle import vlp_oracle as O
    from vlp_amd import modeling as M
    cfg = M.BertConfig(512, num_hidden_layers=2, type_vocab_size=6)
    assert M.BertConfig.from_dict(cfg.to_dict()).to_json_string() == cfg.to_json_string()
    for tasks in ("img2txt", "vqa2"):
        m = M.BertForPreTrainingLossMask(cfg, num_labels=2, enable_butd=True, len_vis_input=100, tasks=tasks, allow_random_fc7=True)
        keys = set(m.state_dict().keys())
        assert keys == set(O.init_params(vocab_size=512, layers=2, tasks=tasks).keys()) | {"cls.predictions.decoder.weight"}
        assert m.cls.predictions.decoder.weight is m.bert.embeddings.word_embeddings.weight        # tied
        names = [n for n, _ in m.named_parameters()]
        assert len(names) == 18 + 16 * 2 + (4 if tasks == "vqa2" else 0)
    sig = inspect.signature(M.BertForPreTrainingLossMask.forward)
    assert list(sig.parameters)[1:] == ["vis_feats", "vis_pe", "input_ids", "token_type_ids", "attention_mask", "masked_lm_labels", "ans_labels",
                                        "next_sentence_label", "masked_pos", "masked_weights", "task_idx", "vis_masked_pos",
                                        "mask_image_regions", "drop_worst_ratio", "vqa_inference"]
    with pytest.raises(Exception, match="Cannot find Detectron fc7 weights"):
        M.BertForPreTrainingLossMask(cfg, enable_butd=True, len_vis_input=100)
    with pytest.raises(NotImplementedError):
        M.BertForPreTrainingLossMask(cfg, enable_butd=False, allow_random_fc7=True)


def test_from_pretrained_resizes_tables(tmp_path):
    from vlp_amd import modeling as M
    cfg = M.BertConfig(300, num_hidden_layers=1, type_vocab_size=2, max_position_embeddings=64)
    open(os.path.join(tmp_path, "bert_config.json"), "w").write(cfg.to_json_string())
    src = M.BertForPreTrainingLossMask(cfg, enable_butd=True, len_vis_input=100, allow_random_fc7=True)
    sd = src.state_dict()
    sd["bert.embeddings.LayerNorm.gamma"] = sd.pop("bert.embeddings.LayerNorm.weight")     # TF-era names are renamed
    sd["bert.embeddings.LayerNorm.beta"] = sd.pop("bert.embeddings.LayerNorm.bias")
    torch.save(sd, os.path.join(tmp_path, "pytorch_model.bin"))
    m = M.BertForPreTrainingLossMask.from_pretrained(str(tmp_path), num_labels=2, type_vocab_size=6, max_position_embeddings=100,
                                                     drop_prob=0.2, enable_butd=True, len_vis_input=100, tasks="img2txt", allow_random_fc7=True)
    assert m.config.type_vocab_size == 6 and m.config.hidden_dropout_prob == 0.2
    tt, old = m.bert.embeddings.token_type_embeddings.weight.data, src.bert.embeddings.token_type_embeddings.weight.data
    assert torch.equal(tt[:2], old) and torch.equal(tt[4], old[0]) and torch.equal(tt[5], old[1])
    pe, po = m.bert.embeddings.position_embeddings.weight.data, src.bert.embeddings.position_embeddings.weight.data
    assert pe.shape[0] == 100 and torch.equal(pe[:64], po) and torch.equal(pe[64:100], po[:36])
    assert m.missing_keys == []
    # random init path of the train script: state_dict={}
    m2 = M.BertForPreTrainingLossMask.from_pretrained(str(tmp_path), state_dict={}, enable_butd=True, len_vis_input=100, allow_random_fc7=True)
    assert len(m2.missing_keys) == len(m2.state_dict())


def test_engine_layout_and_buckets():
    from vlp_amd import modeling as M
    from vlp_amd.engine import is_no_decay
    cfg = M.BertConfig(512, num_hidden_layers=3, type_vocab_size=6)
    m = M.BertForPreTrainingLossMask(cfg, enable_butd=True, len_vis_input=100, tasks="img2txt", allow_random_fc7=True)
    decay, nodecay, buckets = m.engine._ordered_names(m)
    names = [n for n, _ in m.named_parameters()]
    assert sorted(decay + nodecay) == sorted(names)
    assert all(not is_no_decay(n) for n in decay) and all(is_no_decay(n) for n in nodecay)
    # same split as the train script's two groups (run_img2txt_dist.py:395-401)
    nd = ["bias", "LayerNorm.bias", "LayerNorm.weight"]
    assert set(nodecay) == {n for n in names if any(x in n for x in nd)}
    # buckets tile the decay list in backward-completion order: head, layers last..first, embeddings/regions
    assert buckets[0][0] == 0 and buckets[-1][1] == len(decay) and all(a[1] == b[0] for a, b in zip(buckets, buckets[1:]))
    assert decay[buckets[1][0]].startswith("bert.encoder.layer.2.") and decay[buckets[3][0]].startswith("bert.encoder.layer.0.")
    i = decay.index("bert.encoder.layer.1.attention.self.query.weight")
    assert decay[i + 1].endswith("key.weight") and decay[i + 2].endswith("value.weight")          # packed QKV


def test_layer_handle_table_names_every_layer_parameter_once():
    """engine.layer_param_names is the one place a layer's parameter names are written down: for a 2-layer model they are exactly the
    bert.encoder.layer.{0,1}.* names of named_parameters(), each once, under the fields of the handle-table row; the engine's source reads
    every field; the names behind one field lie back to back in the flat buffer (a packed view is one slice).  A parameter added to
    the model without a handle fails here."""
    from vlp_amd import engine as E
    from vlp_amd import modeling as M
    cfg = M.BertConfig(512, num_hidden_layers=2, type_vocab_size=6)
    m = M.BertForPreTrainingLossMask(cfg, enable_butd=True, len_vis_input=100, tasks="img2txt", allow_random_fc7=True)
    numel = {n: p.numel() for n, p in m.named_parameters()}
    lay = m.engine.plan_layout(m)
    import ast
    read = {n.attr for n in ast.walk(ast.parse(open(os.path.join(ROOT, "vlp_amd", "engine.py")).read())) if isinstance(n, ast.Attribute)}
    for i in (0, 1):
        table = E.layer_param_names(i)
        assert tuple(table) == E._LayerViews.__slots__ and len(table) == 12
        listed = [n for ns in table.values() for n in ns]
        assert sorted(listed) == sorted(n for n in numel if n.startswith("bert.encoder.layer.%d." % i))
        assert len(set(listed)) == len(listed) == 16
        for f, ns in table.items():
            assert f in read, "no engine code reads the field %s" % f
            assert all(n.endswith(".bias") == f.endswith("_b") and n.endswith(".weight") == f.endswith("_w") for n in ns), (f, ns)
            grp = "nodecay" if E.is_no_decay(ns[0]) else "decay"
            assert lay["names"][grp].count(ns[0]) == 1
            for a, b in zip(ns, ns[1:]):
                assert lay["offsets"][grp][b] - lay["offsets"][grp][a] == numel[a], (a, b)
    assert not set(E.layer_param_names(0).values()) & set(E.layer_param_names(1).values())


def test_entry_script_arguments_match_reference():
    from vlp_amd import run_img2txt_dist as R
    ours = {a.dest: a.default for a in R.build_parser()._actions if a.dest != "help"}
    from oracle.make_golden import load_contract
    flags = set(str(f) for f in load_contract()["entry_flags"])     # the reference entry script's flags (tests/golden/reference_contract.npz)
    assert flags and flags <= set(ours), flags - set(ours)
    args = R.derive_args(R.build_parser().parse_args(["--enable_butd", "--fp16", "--max_len_b", "64", "--output_dir", "/tmp/x"]))
    assert args.max_seq_length == 167 and args.dist_url == "file:///tmp/x/nonexistent_file"
    with pytest.raises(AssertionError):
        R.derive_args(R.build_parser().parse_args([]))          # enable_butd is mandatory, as in the reference (:199)


def test_synthetic_batch_contract():
    from vlp_amd import synthetic as S
    b = S.make_batch(6, max_len_b=20, s2s_prob=0.5, seed=3)
    L, Nv = 123, 100
    assert b.input_ids.shape == (6, L) and b.input_mask.shape == (6, L, L) and b.img.shape == (6, 100, 2048) and b.vis_pe.shape == (6, 100, 1607)
    for i in range(6):
        n_tok = int((b.input_ids[i] != 0).sum())
        n_b = n_tok - Nv - 3
        m = b.input_mask[i]
        assert (m[:, :Nv + 2] == 1).all() or int(b.task_idx[i]) == 0
        if int(b.task_idx[i]) == 3:        # seq2seq: lower-triangular text block, padding rows see only the visual block
            blk = m[Nv + 2:Nv + 3 + n_b, Nv + 2:Nv + 3 + n_b]
            assert torch.equal(blk, torch.tril(torch.ones_like(blk)))
            assert int(m[-1, Nv + 2:].sum()) == 0 or n_b == 20
        else:                              # bidirectional: every row sees every non-pad column
            assert torch.equal(m[0], (torch.arange(L) < n_tok).long())
        w = b.masked_weights[i].bool()
        assert ((b.masked_pos[i][w] >= Nv + 2) & (b.masked_pos[i][w] < n_tok)).all()


def test_compat_import_paths():
    """vlp_amd.compat.install(): the reference's import lines (run_img2txt_dist.py:23-30,405-406) resolve to the HIP implementation."""
    import subprocess
    code = (
        "import sys; sys.path.insert(0, %r)\n"
        "import vlp_amd.compat as c; c.install()\n"
        "from pytorch_pretrained_bert.modeling import BertForPreTrainingLossMask, BertForSeq2SeqDecoder, BertConfig\n"
        "from pytorch_pretrained_bert.optimization import BertAdam, warmup_linear\n"
        "from pytorch_pretrained_bert.optimization_fp16 import FP16_Optimizer_State\n"
        "from apex.optimizers import FusedAdam\n"
        "import pytorch_pretrained_bert as P, vlp_amd.modeling as M, vlp_amd.optimization_fp16 as F\n"
        "assert BertForPreTrainingLossMask is M.BertForPreTrainingLossMask and P.BertForSeq2SeqDecoder is M.BertForSeq2SeqDecoder\n"
        "assert FusedAdam is F.FusedAdam and FP16_Optimizer_State is F.FP16_Optimizer_State and warmup_linear(0.05, 0.1) == 0.5\n"
        "c.uninstall(); assert 'pytorch_pretrained_bert' not in sys.modules\n"
        "print('ok')\n") % os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr[-2000:]


def test_launch_plan_record_and_replay(monkeypatch):
    """_lib.record() executes AND collects the C calls of a block; replay() re-issues them and surfaces a failing status."""
    from vlp_amd import _lib
    calls = []

    class FakeLib(object):
        def vlp_a(self, x, y):
            calls.append(("a", x, y))
            return 0

        def vlp_b(self, x):
            calls.append(("b", x))
            return 0 if x != 13 else -2

        def vlp_last_error_string(self):
            return b"boom"

    monkeypatch.setattr(_lib, "_lib", FakeLib())
    with _lib.record() as plan:
        assert _lib.load().vlp_a(1, 2) == 0 and _lib.load().vlp_b(5) == 0
        with pytest.raises(RuntimeError):
            with _lib.record():
                pass                                    # no nesting
    assert calls == [("a", 1, 2), ("b", 5)] and len(plan) == 2
    assert _lib.load() is _lib._lib                     # recording ended
    _lib.replay(plan)
    assert calls == [("a", 1, 2), ("b", 5)] * 2
    with _lib.record() as bad:
        _lib.load().vlp_b(13)
    with pytest.raises(RuntimeError, match="boom"):
        _lib.replay(bad)


def test_header_is_plain_c_and_the_c_consumer_compiles():
    """include/vlp_hip.h stands alone: a C (not C++) translation unit that includes it and calls the entry points compiles with gcc
    (tests/c_abi_smoke.c; it is linked against libvlp_hip.so and run on the GPU box by tests/test_00_kernels_gpu.py)."""
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if shutil.which("gcc") is None or not os.path.isdir("/opt/rocm/include"):
        pytest.skip("needs gcc and the ROCm headers")
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-D_GNU_SOURCE", "-I", os.path.join(root, "include"), "-I", "/opt/rocm/include",
                        "-fsyntax-only", os.path.join(root, "tests", "c_abi_smoke.c")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def _backtrack(self, scores, words, back):
    """The per-sample rule _backtrack_batch is checked against.  One sample's frames (lists [frames][K]) -> best hypothesis
    (:1446-1474): candidates are the hypotheses that emitted eos, or any hypothesis of the last valid frame (the first frame whose words
    are all eos, else the final one); rank by cumulative log-probability + length_penalty * length; follow the back pointers."""
    import math
    eos, lp = self.eos_id, self.length_penalty
    last = next((i for i, w in enumerate(words) if all(x == eos for x in w)), len(scores) - 1)
    best = None
    for f in range(last + 1):
        for k, w in enumerate(words[f]):
            if w == eos or f == last:
                val = scores[f][k] + lp * (f + 1)
                if best is None or val > best[0]:
                    best = (val, f, k)
    if best is None or best[0] == -math.inf:
        return [0]
    _, f, k = best
    out = [words[f][k]]
    while f > 0:
        k = back[f][k]
        f -= 1
        out.append(words[f][k])
    out.reverse()
    return out


def test_beam_backtrack_batch_equals_the_per_sample_rule():
    """BertForSeq2SeqDecoder.beam_search picks every sample's best hypothesis on the host in ONE vectorised pass (round 6: the per-sample Python loop with
    its tensor constructions caused 30 - 110 ms stalls at 320 hypotheses); it must follow the reference's rule (modeling.py:1446-1474) exactly as the
    per-sample _backtrack does: eos candidates or the last valid frame, score + length_penalty * length, FIRST maximum, back pointers."""
    import numpy as np
    from vlp_amd.modeling import BertForSeq2SeqDecoder

    class Dec(object):
        eos_id, length_penalty = 3, 0.3
    d = Dec()
    rng = np.random.RandomState(0)
    for trial in range(200):
        F, B, K = rng.randint(1, 8), rng.randint(1, 6), rng.randint(2, 5)
        sc = rng.randn(F, B, K).astype(np.float32)
        if trial % 5 == 0:
            sc = np.round(sc)                          # ties: the first maximum in (frame, beam) order wins
        ww, pp = rng.randint(0, 6, size=(F, B, K)), rng.randint(0, K, size=(F, B, K))
        if trial % 7 == 0:
            ww[rng.randint(0, F)] = 3                  # a frame whose words are all eos ends the search there
        if trial % 11 == 0:
            sc[:] = -np.inf                            # nothing finite: the reference returns [0]
        out = BertForSeq2SeqDecoder._backtrack_batch(d, sc, ww, pp, F + 2)
        for b in range(B):
            seq = _backtrack(d, [sc[f, b].tolist() for f in range(F)], [ww[f, b].tolist() for f in range(F)], [pp[f, b].tolist() for f in range(F)])
            exp = np.zeros(F + 2, dtype=np.int64)
            exp[:len(seq)] = seq
            assert np.array_equal(out[b], exp), (trial, b, out[b], exp)
