"""GPU: VQA 2.0 on real data -- the answer target as (index, score) pairs (vlp_amd.input_prep.SparseAnswers).

  * vlp_bce_sparse_loss_fwd / _bwd are the dense BCE kernels instantiated with another source of y: loss and dlogits must equal the dense
    entry points' on SparseAnswers.dense(N) BIT FOR BIT (no tolerance), and separately meet test_00's bounds against torch in fp64;
  * vlp_vqa_answer_rows: first maximum over columns [1, N), its value, and the score the row lists for it;
  * the model takes a SparseAnswers wherever it takes dense ans_labels (dense and padding-free step), model.answer();
  * python -m vlp_amd.run_img2txt_dist --tasks vqa2 on a packed store, then python -m vlp_amd.eval_vqa2 on the checkpoint it wrote.
"""
import json
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from oracle import vlp_oracle as O                                      # noqa: E402 (checker: parameter init only)
from tests import guard_util as G                                       # noqa: E402
from tests.kernel_util import h16, rel                                  # noqa: E402
from vlp_amd import _lib as K                                           # noqa: E402
from vlp_amd import eval_vqa2 as E                                      # noqa: E402
from vlp_amd import run_img2txt_dist as R                               # noqa: E402
from vlp_amd import synthetic as S                                      # noqa: E402
from vlp_amd.data import PackedRegionStore, write_packed                # noqa: E402
from vlp_amd.input_prep import MaskSpec, RawRegions, SparseAnswers      # noqa: E402
from vlp_amd.modeling import BertConfig, BertForPreTrainingLossMask     # noqa: E402
from vlp_amd.optimization_fp16 import FP16_Optimizer_State, FusedAdam   # noqa: E402

DEV = torch.device("cuda:0")
F32, I64 = torch.float32, torch.int64
NA = 3129
P3 = float(np.float32(0.3))          # the score of an answer given once among ten, as the f32 the kernels read


@pytest.fixture
def gen():
    return torch.Generator(device=DEV).manual_seed(71)


def answer_rows(B, N, seed):
    """Answer lists of B questions over an N-entry vocabulary: row 0 has no answers (unknown only), row 1 fills all 10 slots (every score
    0.3), row 2 has entries at columns N-1 and (when 0 is not the unknown index: the caller passes unk_index=-1) 0 with scores 1.0 and
    0.3; the rest are random mixtures."""
    rng = np.random.RandomState(seed)
    rows = [[-1] * 10, [1 + (7 * k) % (N - 1) for k in range(10)], [N - 1] * 9 + [0]]
    while len(rows) < B:
        k = rng.randint(1, 5)
        pool = rng.choice(N, size=k, replace=False)
        rows.append([int(pool[rng.randint(k)]) for _ in range(10)])
    return rows[:B]


def sparse_targets(B, N, seed):
    sa = SparseAnswers.from_answer_ids(answer_rows(B, N, seed), unk_index=-1, num_answers=N)
    y = sa.dense(N)
    assert int((sa.idx[0] >= 0).sum()) == 0 and int((sa.idx[1] >= 0).sum()) == 10
    assert float(y[2, N - 1]) == 1.0 and float(y[2, 0]) == P3 and bool((y[1][y[1] > 0] == P3).all())
    return sa.to(DEV), y.to(DEV)


# =====================================================================================================
# loss kernels
# =====================================================================================================
@pytest.mark.parametrize("B,N,ld", [(3, 70, 72), (5, 3129, 3136), (64, 3129, 3136)])
def test_sparse_bce_equals_dense_bce_bit_for_bit(B, N, ld, gen):
    sa, y = sparse_targets(B, N, seed=B)
    logits = torch.full((B, ld), 30.0, device=DEV, dtype=torch.half)              # the pad columns hold 30.0: reading one moves the loss
    logits[:, :N] = h16(B, N, scale=3.0, gen=gen)
    loss_d, loss_s = torch.zeros(257, device=DEV), torch.zeros(257, device=DEV)
    K.bce_loss_fwd(logits, ld, y, N, B, N, loss_d)
    K.bce_sparse_loss_fwd(logits, ld, sa.idx, sa.score, B, N, loss_s)
    print("B %d N %d: loss dense %r sparse %r" % (B, N, float(loss_d[0]), float(loss_s[0])))
    assert math.isfinite(float(loss_s[0])) and torch.equal(loss_s[0].view(torch.int32), loss_d[0].view(torch.int32))
    gs = torch.full((1,), 64.0, device=DEV)
    d_d = torch.full((B, ld), 3.0, device=DEV, dtype=torch.half)
    d_s = torch.full((B, ld), 3.0, device=DEV, dtype=torch.half)
    K.bce_loss_bwd(logits, ld, y, N, B, N, gs, d_d, ld)
    K.bce_sparse_loss_bwd(logits, ld, sa.idx, sa.score, B, N, gs, d_s, ld)
    assert torch.equal(d_s.view(torch.int16), d_d.view(torch.int16))
    assert bool((d_s[:, N:].view(torch.int16) == 0).all())                        # pad columns: +0
    # and against torch in fp64, with the bounds of tests/test_00_kernels_gpu.py::test_bce_loss
    x = logits[:, :N].double().requires_grad_(True)
    ref = torch.nn.functional.binary_cross_entropy_with_logits(x, y.double()) * N
    assert abs(float(loss_s[0]) - float(ref.detach())) < 1e-4 * abs(float(ref.detach()))
    (ref * 64.0).backward()
    assert rel(d_s[:, :N].float(), x.grad) < 2e-3


@pytest.mark.parametrize("B,N", [(5, 3129), (3, 70), (4, 3)])
def test_sparse_bce_guarded(B, N, gen):
    """Both kernels inside guard bands: NaN around the logits and in their padding, sentinels around the outputs, index guards of -1 /
    NaN scores around the pairs; nothing outside the logical extents may be read into the result or written."""
    sa, y = sparse_targets(B, N, seed=11) if N >= 12 else (SparseAnswers.from_answer_ids([[2, 2, 0], [1], [-1], [0, 1, 2]], unk_index=-1, num_answers=N).to(DEV), None)
    if y is None:
        y = sa.dense(N)
    S_ = sa.idx.shape[1]
    logits = G.guarded(B, N, ld=G.roundup8(N) + 8, dtype=torch.float16, fill="nan", device=DEV).set(h16(B, N, scale=3.0, gen=gen))
    idx = G.guarded(B, S_, dtype=torch.int32, fill=-1, device=DEV).set(sa.idx)
    score = G.guarded(B, S_, dtype=F32, fill="nan", device=DEV).set(sa.score)
    loss = G.guarded_vec(257, dtype=F32, fill="sentinel", device=DEV)
    K.bce_sparse_loss_fwd(logits.view, logits.ld, idx.view, score.view, B, N, loss.vec)
    x64 = logits.view.double().requires_grad_(True)
    ref = torch.nn.functional.binary_cross_entropy_with_logits(x64, y.double()) * N
    assert math.isfinite(float(loss.vec[0])) and abs(float(loss.vec[0]) - float(ref.detach())) < 1e-4 * abs(float(ref.detach()))
    G.assert_untouched(loss, written="logical", name="loss")
    gs = G.guarded_vec(1, dtype=F32, fill="nan", device=DEV).set(torch.full((1,), 64.0, device=DEV))
    d = G.guarded(B, N, ld=G.roundup8(N) + 24, dtype=torch.float16, fill="sentinel", device=DEV)
    K.bce_sparse_loss_bwd(logits.view, logits.ld, idx.view, score.view, B, N, gs.vec, d.view, d.ld)
    (ref * 64.0).backward()
    G.assert_written(d, "rows", "dlogits")
    G.assert_finite(d.view, "dlogits")
    assert rel(d.view.float(), x64.grad) < 2e-3
    G.assert_zero_band(d, N, d.ld, "dlogits")
    G.assert_untouched(d, written="rows", name="dlogits")
    for g, name in ((logits, "logits"), (idx, "ans_idx"), (score, "ans_score"), (gs, "grad_scale")):
        G.assert_untouched(g, name=name)


# =====================================================================================================
# answer choice
# =====================================================================================================
def first_max_rule(logits, N):
    """torch.where(row[1:N] == row[1:N].max())[0][0] + 1 per row, and that maximum."""
    ids, vals = [], []
    for row in logits:
        r = row[1:N].float()
        ids.append(int(torch.where(r == r.max())[0][0]) + 1)
        vals.append(float(r.max()))
    return torch.tensor(ids, device=DEV), torch.tensor(vals, device=DEV, dtype=F32)


@pytest.mark.parametrize("B,N,ld", [(6, 3129, 3136), (5, 70, 72), (4, 300, 304)])
def test_vqa_answer_rows(B, N, ld, gen):
    sa, y = sparse_targets(B, N, seed=5)
    logits = torch.full((B, ld), 30.0, device=DEV, dtype=torch.half)              # pad columns above every logit
    logits[:, :N] = h16(B, N, scale=2.0, gen=gen).clamp(-8, 8)
    logits[:, 0] = 20.0                                                           # the global maximum sits in column 0: never an answer
    logits[0, N - 1] = 12.0                                                       # maximum in the last valid column
    logits[2, N - 1] = 12.0                                                       # ... which row 2 lists with score 1.0
    logits[3, [1, N - 1]] = 9.5                                                   # a tie between the first and the last candidate
    listed = int(sa.idx[1, 4])
    logits[1, [N - 2, listed, N // 2 + 7]] = 11.0                                 # exact ties: the first index wins; row 1 lists it (score 0.3)
    want_ids, want_vals = first_max_rule(logits, N)
    assert 1 <= listed < N // 2 and int(want_ids[0]) == N - 1 and int(want_ids[3]) == 1 and int(want_ids[1]) == listed
    ids = G.guarded_vec(B, dtype=I64, fill="sentinel", device=DEV)
    vals = G.guarded_vec(B, dtype=F32, fill="sentinel", device=DEV)
    scores = G.guarded_vec(B, dtype=F32, fill="sentinel", device=DEV)
    K.vqa_answer_rows(logits, ld, B, N, 1, ids.vec, vals.vec, sa.idx, sa.score, scores.vec)
    assert torch.equal(ids.vec, want_ids) and torch.equal(vals.vec, want_vals)
    want_scores = y[torch.arange(B, device=DEV), want_ids]
    assert torch.equal(scores.vec, want_scores)
    assert float(want_scores[2]) == 1.0 and float(want_scores[0]) == 0.0          # a listed answer, an unlisted one
    assert float(want_scores[1]) == P3
    for g, name in ((ids, "out_ids"), (vals, "out_vals"), (scores, "out_scores")):
        G.assert_untouched(g, written="logical", name=name)
    # without targets out_scores is not touched
    ids2 = G.guarded_vec(B, dtype=I64, fill="sentinel", device=DEV)
    vals2 = G.guarded_vec(B, dtype=F32, fill="sentinel", device=DEV)
    scores.seal()
    K.vqa_answer_rows(logits, ld, B, N, 1, ids2.vec, vals2.vec)
    assert torch.equal(ids2.vec, want_ids) and torch.equal(vals2.vec, want_vals)
    G.assert_untouched(scores, written=None, name="out_scores (no targets)")
    # first_col = 0: plain first-maximum argmax over [0, N)
    K.vqa_answer_rows(logits, ld, B, N, 0, ids2.vec, vals2.vec)
    assert bool((ids2.vec == 0).all()) and bool((vals2.vec == 20.0).all())


# =====================================================================================================
# model
# =====================================================================================================
ND = ["bias", "LayerNorm.bias", "LayerNorm.weight"]


def build_model(seed=5):
    p = O.init_params(vocab_size=1024, layers=2, tasks="vqa2", seed=seed)
    cfg = BertConfig(1024, num_hidden_layers=2, type_vocab_size=6, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    m = BertForPreTrainingLossMask(cfg, enable_butd=True, len_vis_input=100, tasks="vqa2", allow_random_fc7=True)
    sd = dict(p)
    sd["cls.predictions.decoder.weight"] = p["bert.embeddings.word_embeddings.weight"]
    m.load_state_dict(sd, strict=True)
    return m.half().to(DEV).train()


def step(model, b, ans):
    named = list(model.named_parameters())
    groups = [{"params": [q for n, q in named if not any(x in n for x in ND)], "weight_decay": 0.01},
              {"params": [q for n, q in named if any(x in n for x in ND)], "weight_decay": 0.0}]
    opt = FP16_Optimizer_State(FusedAdam(groups, lr=1e-3, bias_correction=False, max_grad_norm=1.0), dynamic_loss_scale=True,
                               dynamic_loss_args={"init_scale": 1.0})          # (the VQA loss is ~2 000: BCE x 3 129)
    lt = model(b.img, b.vis_pe, b.input_ids, b.segment_ids, b.input_mask, b.lm_label_ids, ans, b.is_next, masked_pos=b.masked_pos,
               masked_weights=b.masked_weights, task_idx=b.task_idx, drop_worst_ratio=0)
    opt.backward(lt[0] + lt[1] + lt[2])
    torch.cuda.synchronize()
    return float(lt[2].detach()), model.last_vqa_logits.clone(), {n: q.grad.detach().float().clone() for n, q in named}


def worst_difference(a, b):
    return max([abs(a[0] - b[0])] + [float((a[2][n] - b[2][n]).abs().max()) for n in a[2]])


@pytest.fixture(scope="module")
def vqa_batch():
    B = 5
    raw = S.make_batch(B, max_len_b=20, vocab_size=1024, max_pred=1, tasks="vqa2", seed=9)
    nb = [int(raw.input_mask[i].any(dim=0).sum()) - 103 for i in range(B)]
    spec = MaskSpec.from_lengths(100, nb, False, device=DEV)
    assert torch.equal(spec.dense(raw.input_mask.shape[1]).cpu(), raw.input_mask)
    sa = SparseAnswers.from_answer_ids(answer_rows(B, NA, seed=3), unk_index=-1)
    return S.batch_to(raw, DEV, half=True), spec, sa.to(DEV), sa.dense(NA).to(DEV)


@pytest.mark.parametrize("packed", [False, True])
def test_model_step_with_sparse_answers_equals_the_dense_labels_step(vqa_batch, packed):
    b, spec, sa, y = vqa_batch
    if packed:
        b = b._replace(input_mask=spec)                                           # host lengths ride along: the padding-free step
    runs = []
    for ans in (y, y, sa):
        model = build_model()
        runs.append(step(model, b, ans))
        assert (model.engine.last_packed_rows is not None) == packed
    noise = worst_difference(runs[0], runs[1])                                    # dense labels twice: the run-to-run difference (expected 0)
    diff = worst_difference(runs[0], runs[2])
    print("packed=%s: dense-vs-dense repeat %.3e, sparse-vs-dense %.3e, loss %.4f" % (packed, noise, diff, runs[2][0]))
    assert math.isfinite(runs[2][0]) and runs[2][0] > 0
    assert torch.equal(runs[0][1], runs[2][1])
    assert diff <= noise


@pytest.mark.parametrize("packed", [False, True])
def test_model_answer(vqa_batch, packed):
    b, spec, sa, y = vqa_batch
    model = build_model().eval()
    mask = spec if packed else b.input_mask
    with torch.no_grad():
        ids, vals, scores = model.answer(b.img, b.vis_pe, b.input_ids, b.segment_ids, mask, answers=sa)
        logits = model.last_vqa_logits.clone()
        assert (model.engine.last_packed_rows is not None) == packed
        want_ids, want_vals = first_max_rule(logits, NA)
        assert ids.dtype == I64 and vals.dtype == F32 and torch.equal(ids, want_ids) and torch.equal(vals, want_vals)
        host = sa.dense(NA).cpu()
        assert scores.tolist() == [float(host[i, int(ids[i])]) for i in range(len(ids))]
        ids2, vals2, none = model.answer(b.img, b.vis_pe, b.input_ids, b.segment_ids, mask)
        assert none is None and torch.equal(ids2, ids) and torch.equal(vals2, vals)
        # the reference's own inference path picks the same answers (modeling.py:1046)
        ref_ids = model(b.img, b.vis_pe, b.input_ids, b.segment_ids, b.input_mask, vqa_inference=True)
        assert torch.equal(model.last_vqa_logits, logits) or packed
        assert torch.equal(ref_ids, ids)
    assert bool((ids >= 1).all()) and bool((ids < NA).all())


# =====================================================================================================
# entry scripts
# =====================================================================================================
N_IMG, T = 6, 12
# 7 questions over the 6 images: (image, number of question tokens, answer ids, question id)
QUESTIONS = [(0, 5, [7] * 10, 1001), (3, 9, [4, 4, 4, 9, 9, 0, 0, 11, 12, 13], 1002), (5, 3, [0] * 10, 1003), (1, 12, [3128] * 4 + [2] * 6, 1004),
             (2, 7, [5, 6, 5, 6, 5, 6, 5, 6, 5, 6], 1005), (4, 15, [1, 2, 3, 4, 5, 6, 7, 8, 9, 10], 1006), (0, 4, [20, 20, 20, 0, 0, 0, 0, 0, 0, 21], 1007)]


@pytest.fixture(scope="module")
def vqa_files(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("vqa_cli"))
    rng = np.random.RandomState(8)
    keys = ["COCO_val2014_%012d" % (100 + i) for i in range(N_IMG)]
    feats = np.abs(rng.randn(N_IMG, 100, 2048)).astype(np.float16)
    cls = rng.rand(N_IMG, 100, 1601).astype(np.float32)
    cls /= cls.sum(-1, keepdims=True)
    xy = rng.rand(N_IMG, 100, 2, 2) * 400
    boxes = np.concatenate([xy.min(2), xy.max(2) + 1.0, np.zeros((N_IMG, 100, 1)), rng.rand(N_IMG, 100, 1)], axis=-1).astype(np.float32)
    store = os.path.join(root, "store")
    write_packed(store, keys, feats, cls, boxes)
    examples = [[keys[i], rng.randint(1000, 2000, size=n).tolist(), ans, qid] for i, n, ans, qid in QUESTIONS]
    token_file = os.path.join(root, "vqa_tokens.json")
    with open(token_file, "w") as f:
        json.dump(examples, f)
    words = ["answer-%d" % i for i in range(NA)]
    vocab_file = os.path.join(root, "answers_vqa.txt")
    with open(vocab_file, "w") as f:
        f.write("\n".join(words) + "\n")
    out_dir = os.path.join(root, "out")
    # train one epoch (2 steps of 4) from scratch (bert-base-cased's shape cut to 2 layers); the tests below evaluate the checkpoint it wrote.
    # Like the reference (modeling.py:1008-1014) a real-data run insists on detectron_weights/fc7_{w,b}.pkl; the test opts out explicitly.
    mp = pytest.MonkeyPatch()
    mp.setenv("VLP_ALLOW_RANDOM_FC7", "1")
    try:
        train(out_dir, store, token_file)
    finally:
        mp.undo()
    return dict(root=root, store=store, token_file=token_file, vocab_file=vocab_file, out_dir=out_dir, examples=examples, words=words)


def train(out_dir, store, token_file):
    R.main(["--output_dir", out_dir, "--tasks", "vqa2", "--packed_features", store, "--token_file", token_file,
            "--num_train_epochs", "1", "--train_batch_size", "4", "--from_scratch", "--fp16", "--enable_butd", "--new_segment_ids",
            "--num_hidden_layers", "2", "--max_len_b", str(T), "--s2s_prob", "0", "--bi_prob", "1", "--max_pred", "1", "--mask_prob", "0",
            "--num_workers", "2", "--log_every", "1", "--drop_prob", "0.1", "--learning_rate", "1e-4"])


def eval_argv(vf, out, *extra):
    return ["--model_recover_path", os.path.join(vf["out_dir"], "model.*.bin"), "--packed_features", vf["store"],
            "--token_file", vf["token_file"], "--output_file", out, "--batch_size", "4", "--max_tgt_length", str(T), "--new_segment_ids", "--fp16",
            "--enable_butd", "--num_hidden_layers", "2", "--split", "val"] + list(extra)


def test_training_script_trains_vqa_from_a_packed_store(vqa_files):
    vf = vqa_files
    with open(os.path.join(vf["out_dir"], "training.log")) as f:
        losses = [float(line.rsplit("Loss", 1)[1]) for line in f if "Iter" in line and "Loss" in line]
    print("VQA losses logged:", losses)
    assert len(losses) == 2 and all(math.isfinite(v) and v > 0 for v in losses)
    sd = torch.load(os.path.join(vf["out_dir"], "model.1.bin"), map_location="cpu")
    for n in ("ans_classifier.0.weight", "ans_classifier.0.bias", "ans_classifier.2.weight", "ans_classifier.2.bias"):
        assert n in sd and bool(torch.isfinite(sd[n].float()).all())
    assert tuple(sd["ans_classifier.2.weight"].shape) == (NA, 2 * 768)


def test_eval_script_answers_equal_the_model_called_directly(vqa_files):
    vf = vqa_files
    out = os.path.join(vf["root"], "answers.json")
    res = E.main(eval_argv(vf, out))
    ckpt = os.path.join(vf["out_dir"], "model.1.bin")
    with open(out) as f:
        preds = json.load(f)
    assert list(res) == [ckpt] and res[ckpt][0] == preds
    assert [p["question_id"] for p in preds] == [q[3] for q in QUESTIONS]        # 7 questions, batches of 4: the short last batch is cut back
    got = [p["answer"] for p in preds]
    assert all(type(a) is int and 1 <= a < NA for a in got)
    # the model called by the test on the same batches
    args = E.build_parser().parse_args(eval_argv(vf, "unused"))
    E.check_args(args)
    model = E.build_model(args, torch.load(ckpt, map_location="cpu"), DEV)
    store, proc = PackedRegionStore(vf["store"]), E.question_preprocessor(args)
    want, host_scores = [], []
    for i in range(0, len(vf["examples"]), 4):
        chunk = vf["examples"][i:i + 4]
        rows = store.rows([e[0] for e in chunk])
        toks = [proc(e[1]) for e in chunk]
        feat = torch.from_numpy(np.ascontiguousarray(store.feat[rows])).to(DEV)
        regions = RawRegions(torch.from_numpy(np.ascontiguousarray(store.bbox[rows])).to(DEV), torch.from_numpy(np.ascontiguousarray(store.cls[rows])).to(DEV))
        spec = MaskSpec.from_lengths([t["len_a"] for t in toks], [t["len_b"] for t in toks], False, device=DEV)
        with torch.no_grad():
            ids, _, _ = model.answer(feat, regions, torch.tensor([t["input_ids"] for t in toks], device=DEV),
                                     torch.tensor([t["segment_ids"] for t in toks], device=DEV), spec)
        want.extend(ids.tolist())
        dense = SparseAnswers.from_answer_ids([e[2] for e in chunk]).dense(NA)
        host_scores.extend(float(dense[j, a]) for j, a in enumerate(ids.tolist()))
    print("answers %s, host scores %s, accuracy %r" % (got, host_scores, res[ckpt][1]))
    assert got == want
    assert res[ckpt][1] == 100.0 * sum(host_scores) / len(host_scores)
    # a two-step model answers these questions wrongly (scores 0): the same questions with answer lists that contain the predictions 10, 1, 0, 2, ...
    # times give non-trivial scores (1.0, 0.3, 0, 0.6, ...); --answer_vocab_file maps the indices to strings
    counts = [10, 1, 0, 2, 3, 4, 1]
    examples2 = [[e[0], e[1], [a] * c + [(a + 1 + k) % (NA - 1) + 1 for k in range(10 - c)], e[3]] for e, a, c in zip(vf["examples"], got, counts)]
    tok2 = os.path.join(vf["root"], "vqa_tokens_scored.json")
    with open(tok2, "w") as f:
        json.dump(examples2, f)
    out2 = os.path.join(vf["root"], "answers_words.json")
    res2 = E.main(eval_argv(vf, out2, "--answer_vocab_file", vf["vocab_file"], "--token_file", tok2))
    with open(out2) as f:
        preds2 = json.load(f)
    assert [p["answer"] for p in preds2] == [vf["words"][a] for a in got]
    dense2 = SparseAnswers.from_answer_ids([e[2] for e in examples2]).dense(NA)
    scores2 = [float(dense2[j, a]) for j, a in enumerate(got)]
    assert scores2 == [1.0, P3, 0.0, float(np.float32(0.6)), float(np.float32(0.9)), 1.0, P3]
    print("scored run: accuracy %r" % (res2[ckpt][1],))
    assert res2[ckpt][1] == 100.0 * sum(scores2) / len(scores2)
    # test2015 has no public answers: no accuracy
    res3 = E.main(eval_argv(vf, os.path.join(vf["root"], "answers_test.json"), "--split", "test2015"))
    assert res3[ckpt][1] is None and [p["answer"] for p in res3[ckpt][0]] == got
