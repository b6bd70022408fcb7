"""GPU: scoring given captions on the device -- vlp_token_score (csrc/loss.hip), Engine.score_captions, BertForSeq2SeqDecoder.score and
python -m vlp_amd.score_img2txt.

(1) the kernel against tests/scst_policy_util.policy_reference (fp64) and tests/caption_score_util.rank_top_reference (torch, exact) over
    the grid of tests/test_86_scst_policy_gpu.py, on aligned rows and on rows at an odd element offset; bit for bit against
    vlp_token_policy_fwd(T = 1, entropy) where that kernel runs (aligned rows); hand-built rows; uncounted rows; guard bands; repeats;
(2) the model on tests/test_80_scst_gpu.py's small case and once at full size: score() against Engine.score_samples (same bits), the
    decoder's own log-probabilities and the oracle's forced decode (test_80's measured bounds), and against its own logits;
(3) the counting rule: counted positions do not depend on what is fed at uncounted ones; truncation;
(4) call sequences: a decoder that scored equals a fresh one in its next greedy, sampled and beam call; results belong to the caller;
(5) the tool: records equal model.score called directly one row at a time, summary, batch sizes, selection, refusals.
Bounds: logp / entropy 1e-4 absolute and lse 1e-5 relative against fp64 (test_80's and test_86's for the same quantities).
Every test prints what it measured through report() (pytest -s); the figures of an MI355X run are in profiles/caption_score.json."""
import copy
import json
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from oracle import vlp_oracle as O                                   # noqa: E402  (checker only)
from oracle.make_golden import decode_inputs                         # noqa: E402  (pure helper)
from tests import caption_score_util as U                            # noqa: E402
from tests import guard_util as GU                                   # noqa: E402
from tests import scst_policy_util as PU                             # noqa: E402
from tests.decode_seq_util import named_outputs, varied_inputs       # noqa: E402
from tests.step_seq_util import first_difference                     # noqa: E402
from tests.test_scst_cpu import forced_decode_logp, scst_inputs      # noqa: E402
from vlp_amd import _lib as K                                        # noqa: E402
from vlp_amd import caption_score as CS                              # noqa: E402
from vlp_amd import synthetic as S                                   # noqa: E402
from vlp_amd.modeling import BertConfig, BertForSeq2SeqDecoder       # noqa: E402

DEV = torch.device("cuda:0")
REPORT = {}
BAD_ARG = -1                                                         # include/vlp_hip.h VLP_ERR_BAD_ARG
F32_OUT = ("logp", "lse", "entropy", "top_logit")
UNCOUNTED = dict(logp=0.0, lse=0.0, entropy=0.0, top_logit=0.0, rank=-1, top_id=-1)


def report(key, **kw):
    """Prints what a test measured; with VLP_CAPTION_SCORE_RECORD=<json file> (profiles/caption_score.json when the record is taken) the
    figures are also kept under that file's "test_48" key, next to the timing runs tools/caption_score_bench.py writes there."""
    REPORT.setdefault(key, {}).update(kw)
    print("%s: %s" % (key, json.dumps(REPORT[key], sort_keys=True)))
    path = os.environ.get("VLP_CAPTION_SCORE_RECORD")
    if path:
        rec = json.load(open(path)) if os.path.exists(path) else {}
        rec.setdefault("test_48", {})[key] = REPORT[key]
        with open(path, "w") as f:
            json.dump(rec, f, indent=2, sort_keys=True)


def padded(x, ld, fill=30.0, offset=0):
    """[R, V] fp16 -> a device view [R, ld] whose pad columns hold `fill`, large values the kernel must not see; offset: elements between
    the allocation's (16-byte aligned) base and the view's -- an odd one gives rows that are not 16-byte aligned."""
    R, V = x.shape
    buf = torch.full((R * ld + 8,), fill, device=DEV, dtype=torch.half)
    view = buf[offset:offset + R * ld].view(R, ld)
    view[:, :V] = x.to(DEV)
    assert view.data_ptr() % 16 == (2 * offset) % 16
    return view


def run_score(logits, ld, ids, rows, V, R=None):
    """One vlp_token_score launch over `rows` rows into outputs of R >= rows elements that hold a sentinel."""
    R = rows if R is None else R
    out = {n: torch.full((R,), 777.0, device=DEV) for n in F32_OUT}
    out["rank"] = torch.full((R,), 777, device=DEV, dtype=torch.int32)
    out["top_id"] = torch.full((R,), 777, device=DEV, dtype=torch.long)
    K.token_score(logits, ld, ids, out["logp"], out["lse"], out["entropy"], out["rank"], out["top_id"], out["top_logit"], rows, V)
    return out


def same_bits(a, b):
    return all(torch.equal(GU.bits(a[n]), GU.bits(b[n])) for n in a)


# =====================================================================================================================================
# (1) the kernel
# =====================================================================================================================================
@pytest.mark.parametrize("extra_ld", [0, 64])
@pytest.mark.parametrize("V", PU.GRID_V)
def test_kernel_against_fp64_its_sibling_and_torch(V, extra_ld):
    R = 48
    ld = GU.roundup8(V) + extra_ld
    x, ids = PU.grid_rows(V, R, 11 + V)
    ids = ids.clamp(min=0)                                             # (a negative id is an uncounted row here: its own test)
    lse_r, lp_r, H_r, _ = PU.reference_rows(x, ids, 1.0)
    rank_r, top_r, topv_r = U.rank_top_reference(x, ids)
    ids_d = ids.to(DEV)
    worst = dict(logp=0.0, H=0.0, lse=0.0)
    for offset in (0, 1):                                              # 16-byte aligned rows (16-byte loads), rows at an odd element offset
        logits = padded(x, ld, offset=offset)
        for rows in (1, 3, 48):
            out = run_score(logits, ld, ids_d, rows, V, R)
            e_lp = float((out["logp"][:rows].double().cpu() - lp_r[:rows]).abs().max())
            e_H = float((out["entropy"][:rows].double().cpu() - H_r[:rows]).abs().max())
            e_lse = float(((out["lse"][:rows].double().cpu() - lse_r[:rows]).abs() / lse_r[:rows].abs().clamp(min=1.0)).max())
            worst.update(logp=max(worst["logp"], e_lp), H=max(worst["H"], e_H), lse=max(worst["lse"], e_lse))
            assert e_lp <= 1e-4 and e_H <= 1e-4, (V, ld, offset, rows, e_lp, e_H)
            assert e_lse < 1e-5, (V, ld, offset, rows, e_lse)
            assert torch.equal(out["rank"][:rows].cpu(), rank_r[:rows]), (V, ld, offset, rows)
            assert torch.equal(out["top_id"][:rows].cpu(), top_r[:rows]), (V, ld, offset, rows)
            assert torch.equal(out["top_logit"][:rows].cpu(), topv_r[:rows]), (V, ld, offset, rows)
            assert torch.equal(out["rank"][:rows] == 0, out["top_id"][:rows] == ids_d[:rows].clamp(max=V - 1))
            for n in out:                                              # rows past `rows` are not this launch's
                assert bool((out[n][rows:] == 777).all()), (n, V, ld, offset, rows)
            assert same_bits(out, run_score(logits, ld, ids_d, rows, V, R))            # a repeat gives the same bits
            if offset == 0:                                            # the sibling takes aligned rows only
                sib = [torch.full((rows,), float("nan"), device=DEV) for _ in range(3)]
                K.token_policy_fwd(logits, ld, ids_d, sib[0], sib[1], rows, V, temperature=1.0, entropy=sib[2])
                for n, t in zip(("logp", "lse", "entropy"), sib):
                    assert torch.equal(GU.bits(out[n][:rows]), GU.bits(t)), (n, V, ld, rows)
    report("kernel_V%d_ld%d" % (V, ld), logp_abs=worst["logp"], entropy_abs=worst["H"], lse_rel=worst["lse"], bound_abs=1e-4, bound_lse=1e-5,
           sibling_bits_equal=True, integers_exact=True)


def test_kernel_hand_built_rows():
    V, ld = 1000, 1000 + 64
    rows = U.hard_score_rows(V)
    names = list(rows)
    x = torch.stack([rows[n][0] for n in names])
    ids = torch.tensor([rows[n][1] for n in names])
    R = len(names)
    lse_r, lp_r, H_r, _ = PU.reference_rows(x, ids, 1.0)
    rank_r, top_r, topv_r = U.rank_top_reference(x, ids)
    got = {}
    for offset in (0, 1):
        out = run_score(padded(x, ld, offset=offset), ld, ids.to(DEV), R, V)
        got[offset] = out
        for n in F32_OUT:
            assert bool(torch.isfinite(out[n]).all()), (n, offset)
        assert torch.equal(out["rank"].cpu(), rank_r) and torch.equal(out["top_id"].cpu(), top_r) and torch.equal(out["top_logit"].cpu(), topv_r)
        for i, name in enumerate(names):
            _, id, want_rank, want_top = rows[name]
            assert want_rank is None or int(out["rank"][i]) == want_rank, (name, offset)
            assert want_top is None or int(out["top_id"][i]) == want_top, (name, offset)
            assert (int(out["rank"][i]) == 0) == (int(out["top_id"][i]) == id), (name, offset)
        # fp64: 1e-4 where fp32 resolves it; a row holding +-65504 has |logp| up to 2^17, where fp32 steps by 2^-6 -- 4 of its steps there
        for n, ref in (("logp", lp_r), ("entropy", H_r), ("lse", lse_r)):
            err = (out[n].double().cpu() - ref).abs()
            bound = 1e-4 + 4 * 2.0 ** -23 * torch.maximum(ref.abs(), lse_r.abs())
            assert bool((err <= bound).all()), (n, offset, [(names[i], float(err[i])) for i in range(R) if err[i] > bound[i]])
    sib = [torch.full((R,), float("nan"), device=DEV) for _ in range(3)]
    K.token_policy_fwd(padded(x, ld), ld, ids.to(DEV), sib[0], sib[1], R, V, temperature=1.0, entropy=sib[2])
    for n, t in zip(("logp", "lse", "entropy"), sib):
        assert torch.equal(GU.bits(got[0][n]), GU.bits(t)), n
    i = names.index("all_equal")
    assert abs(float(got[0]["entropy"][i]) - math.log(V)) <= 1e-4 and abs(float(got[0]["logp"][i]) + math.log(V)) <= 1e-4
    report("hand_rows", rows=names, ranks=got[0]["rank"].tolist(), top_ids=got[0]["top_id"].tolist())


def test_kernel_uncounted_rows_are_not_read_and_change_nothing_else():
    R, V, ld = 48, 257, 264 + 64
    x, ids = PU.grid_rows(V, R, 5)
    ids = ids.clamp(min=0)
    skip = torch.zeros(R, dtype=torch.bool)
    skip[[0, 2, 3, 17, 47]] = True
    ids_s = torch.where(skip, torch.tensor([-1, -7, -(1 << 40), -1, -2]).repeat(10)[:R], ids)
    for offset in (0, 1):
        logits = padded(x, ld, offset=offset)
        full = run_score(logits, ld, ids.to(DEV), R, V)
        logits[skip.to(DEV)] = float("nan")                                # an uncounted row is not read: its values cannot matter
        rows = R - 8
        out = run_score(logits, ld, ids_s.to(DEV), rows, V, R)
        live = (~skip)[:rows].to(DEV)
        for n in out:
            assert torch.equal(GU.bits(out[n][:rows][live]), GU.bits(full[n][:rows][live])), (n, offset)     # the other rows' bits
            assert bool((out[n][:rows][~live] == UNCOUNTED[n]).all()), (n, offset)
            assert bool((out[n][rows:] == 777).all()), (n, offset)
        assert int((~live).sum()) == 4


@pytest.mark.parametrize("R,V,pad", [(48, 28996, 64), (3, 257, 24), (2, 7, 0)])
def test_kernel_guard_bands(R, V, pad):
    x, ids = PU.grid_rows(V, R, 31 + V)
    ids = ids.clamp(min=0)
    if R > 2:
        ids[2] = -1
    ld = GU.roundup8(V) + pad
    logits = GU.guarded(R, V, ld=ld, dtype=torch.half, fill="nan", device=DEV).set(x.to(DEV))       # NaN padding and guards: never read
    ids_g = GU.guarded_vec(R, torch.long, fill=0, device=DEV).set(ids.to(DEV))
    kinds = dict(logp=torch.float32, lse=torch.float32, entropy=torch.float32, top_logit=torch.float32, rank=torch.int32, top_id=torch.long)
    outs = {n: GU.guarded_vec(R, dt, fill="sentinel", device=DEV) for n, dt in kinds.items()}
    K.token_score(logits.view, ld, ids_g.vec, outs["logp"].vec, outs["lse"].vec, outs["entropy"].vec, outs["rank"].vec, outs["top_id"].vec,
                  outs["top_logit"].vec, R, V)
    for n, gd in outs.items():
        GU.assert_written(gd, "logical", n)
        GU.assert_finite(gd.vec, n)
        GU.assert_untouched(gd, written="logical", name=n)
    GU.assert_untouched(logits, name="logits")
    GU.assert_untouched(ids_g, name="ids")
    rank_r, top_r, _ = U.rank_top_reference(x, ids.clamp(min=0))
    live = ids >= 0
    assert torch.equal(outs["rank"].vec.cpu()[live], rank_r[live]) and torch.equal(outs["top_id"].vec.cpu()[live], top_r[live])


def test_kernel_refuses_by_return_code_and_writes_nothing():
    import ctypes as C
    R, V, ld = 3, 40, 40
    lib = K.load()
    logits = torch.zeros(R, ld + 8, device=DEV, dtype=torch.half)
    ids = torch.zeros(R, dtype=torch.long, device=DEV)
    out = run_score(logits, ld + 8, ids, R, V)
    for t in out.values():
        t.fill_(5)
    p, sp = K.ptr, K.stream_ptr()

    def call(ld_=ld + 8, rows=R, V_=V, **nulls):
        o = dict(out, **nulls)
        a = K.TokenScoreArgs(p(logits), ld_, p(ids), p(o["logp"]), p(o["lse"]), p(o["entropy"]), p(o["rank"]), p(o["top_id"]), p(o["top_logit"]),
                             rows, V_)
        return lib.vlp_token_score(C.byref(a), sp)
    codes = {"ld < V": call(ld_=V - 8), "rows 0": call(rows=0), "V 0": call(V_=0), "V > 2^24": call(ld_=(1 << 24) + 8, V_=(1 << 24) + 1)}
    for n in out:
        codes["null " + n] = call(**{n: None})
    torch.cuda.synchronize()
    report("refusals", codes=codes)
    assert all(c == BAD_ARG for c in codes.values()), codes
    assert all(bool((t == 5).all()) for t in out.values())                              # nothing was written
    assert call() == 0
    torch.cuda.synchronize()


# =====================================================================================================================================
# (2) the model
# =====================================================================================================================================
def _decoder(p, V, layers):
    cfg = BertConfig(V, num_hidden_layers=layers, type_vocab_size=6, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    m = BertForSeq2SeqDecoder(cfg, mask_word_id=S.MASK_ID, eos_id=S.SEP_ID, enable_butd=True, len_vis_input=100)
    sd = dict(p)
    sd["cls.predictions.decoder.weight"] = p["bert.embeddings.word_embeddings.weight"]
    m.load_state_dict(sd, strict=True)
    return m.half().to(DEV).eval()


def _model_case(V, layers, B, max_len_b, seed, std):
    """The decoder draws ids; score() scores them.  Everything the tests of this section compare, computed once."""
    p = O.init_params(vocab_size=V, layers=layers, seed=seed, std=std)
    m = _decoder(p, V, layers)
    img, vis_pe, prefix, seg, pos, am, _, _ = scst_inputs(B, max_len_b, seed, V, short=(1,), ragged=((0, 41),), pos_offset=2)
    dv = [t.to(DEV) for t in (img, vis_pe, prefix, seg, pos, am)]
    inp = (dv[0].half(), dv[1].half()) + tuple(dv[2:])
    eng = m.engine
    with torch.no_grad():
        ids, lp_dec = eng.decode_greedy(*inp, S.MASK_ID, sample=True)
        lp_ss = eng.score_samples(*inp, ids, S.MASK_ID)[1].clone()
        logp, ent, rank, top_id, counted = m.score(*inp, ids)
        again = eng.score_captions(*inp, ids, S.MASK_ID, return_logits=True)
        pd = {k: v.to(DEV).half().float() for k, v in p.items()}
        vf, vp = O.vis_embed(pd, inp[0].float()), O.vis_pe_embed(pd, inp[1].float())
        lp_o = forced_decode_logp(pd, vf, vp, *dv[2:], ids, S.MASK_ID)
    torch.cuda.synchronize()
    return dict(m=m, inp=inp, ids=ids, lp_dec=lp_dec, lp_ss=lp_ss, lp_o=lp_o, out=(logp, ent, rank, top_id), counted=counted, again=again, V=V)


@pytest.fixture(scope="module")
def small():
    return _model_case(1024, 3, 5, 12, 21, 0.05)


def _check_model_case(c, key, bound_dec, bound_oracle):
    logp, ent, rank, top_id = c["out"]
    B, T = c["ids"].shape
    assert logp.shape == (B, T) and bool(c["counted"].all())                   # T tokens: all counted, cut, no [SEP]
    assert (logp.dtype, ent.dtype, rank.dtype, top_id.dtype, c["counted"].dtype) == (torch.float32, torch.float32, torch.int32, torch.long, torch.bool)
    e_dec = float((logp - c["lp_dec"]).abs().max())
    e_o = float((logp - c["lp_o"]).abs().max())
    report(key, logp_vs_decoder=e_dec, bound_decoder=bound_dec, logp_vs_oracle=e_o, bound_oracle=bound_oracle, B=B, T=T,
           top1=float((rank == 0).float().mean()), mean_entropy=float(ent.mean()))
    assert torch.equal(GU.bits(logp), GU.bits(c["lp_ss"]))                     # score_samples' launches, score_samples' bits
    assert e_dec < bound_dec, e_dec
    assert e_o < bound_oracle, e_o
    # against its own logits
    a_logp, a_ent, a_rank, a_top, rows16 = c["again"]
    for a, b in zip(c["out"], (a_logp, a_ent, a_rank, a_top)):
        assert torch.equal(GU.bits(a), GU.bits(b))                             # the second call scored the same bits
    assert rows16.shape == (B, T, c["V"]) and rows16.dtype == torch.half
    rank_r, top_r, _ = U.rank_top_reference(rows16.view(B * T, -1), c["ids"].view(-1))
    assert torch.equal(rank.view(-1).cpu(), rank_r) and torch.equal(top_id.view(-1).cpu(), top_r)
    lp64 = torch.log_softmax(rows16.double(), -1)
    H64 = -(lp64.exp() * lp64).sum(-1)
    e_H = float((ent.double() - H64).abs().max())
    e_own = float((logp.double() - lp64.gather(2, c["ids"].unsqueeze(2)).squeeze(2)).abs().max())
    report(key, entropy_vs_own_logits=e_H, logp_vs_own_logits=e_own)
    assert e_H <= 1e-4 and e_own <= 1e-4


def test_small_model_score_vs_score_samples_decoder_oracle_and_own_logits(small):
    _check_model_case(small, "model_1024_3", 0.0048, 0.0036)                  # test_80's bounds for exactly this case


def test_full_size_score_vs_score_samples_decoder_oracle_and_own_logits():
    _check_model_case(_model_case(28996, 12, 16, 20, 5, 0.02), "model_28996_12", 0.003, 0.003)


def test_refusals_leave_no_workspace(small):
    m, inp, ids = small["m"], small["inp"], small["ids"]
    eng = m.engine
    m.train()
    try:
        with pytest.raises(RuntimeError, match="inference entry"):
            m.score(*inp, ids)
        with torch.no_grad():
            assert torch.equal(m.score(*inp, ids)[0], small["out"][0])         # train() under no_grad is inference
    finally:
        m.eval()
    keys = set(eng._ws)
    with torch.no_grad():
        with pytest.raises(RuntimeError, match=r"caption ids \[B, %d\]" % ids.shape[1]):
            eng.score_captions(*inp, ids[:, :5], S.MASK_ID)
        with pytest.raises(ValueError, match="outside the vocabulary"):
            m.score(*inp, [[small["V"]]] * ids.shape[0])
        B, in_len, T = 2, 102, 78                                              # 102 + 2 x 78 - 1 = 257 positions
        _, _, prefix, seg, pos, am = [t.to(DEV) for t in decode_inputs(B, T, 0, Nv=100)]
        with pytest.raises(RuntimeError, match="256"):
            eng.score_captions(inp[0][:B], inp[1][:B], prefix, seg, pos, am, torch.zeros(B, T, dtype=torch.long, device=DEV), S.MASK_ID)
    assert set(eng._ws) == keys                                                # a refused call leaves no workspace behind


# =====================================================================================================================================
# (3) the counting rule
# =====================================================================================================================================
def test_counted_positions_do_not_depend_on_uncounted_ones_and_truncation(small):
    m, inp, V = small["m"], small["inp"], small["V"]
    B, T = small["ids"].shape
    assert B == 5
    gen = torch.Generator().manual_seed(3)
    caps = [torch.randint(1, V, (n,), generator=gen).tolist() for n in (1, 3, T - 1, T, T + 4)]
    ids, counted, trunc = CS.counted_positions(caps, T, S.SEP_ID, vocab_size=V)
    assert trunc.tolist() == [False, False, False, True, True]
    assert counted.sum(1).tolist() == [2, 4, T, T, T]
    assert [int(ids[r, int(counted[r].sum()) - 1]) == S.SEP_ID for r in range(B)] == [True, True, True, False, False]
    ids_d, c = ids.to(DEV), counted.to(DEV)
    with torch.no_grad():
        a = m.engine.score_captions(*inp, ids_d, S.MASK_ID)                                    # fed as id 0
        b = m.engine.score_captions(*inp, ids_d, S.MASK_ID, uncounted_fill=V - 3)
        via_model = m.score(*inp, caps)
    for n, x, y, z in zip(("logp", "entropy", "rank", "top_id"), a, b, via_model):
        assert torch.equal(GU.bits(x[c]), GU.bits(y[c])), n                    # a masked key has weight exactly 0; rows are independent
        assert torch.equal(GU.bits(x), GU.bits(z)), n
        assert bool((x[~c] == UNCOUNTED[n]).all()) and bool((y[~c] == UNCOUNTED[n]).all()), n
    assert torch.equal(via_model[4], c)
    assert bool(torch.isfinite(a[0]).all()) and bool((a[0][c] < 0).all())
    report("counting_rule", counted=counted.sum(1).tolist(), truncated=trunc.tolist(), independent_of_uncounted=True)


# =====================================================================================================================================
# (4) call sequences
# =====================================================================================================================================
def _decode(model, inputs, seed, beam, **kw):
    model.search_beam_size = beam
    model.engine.step_seed = seed
    with torch.no_grad():
        res = model(*inputs, task_idx=None, **kw)
    torch.cuda.synchronize()
    return named_outputs(res, {"step_seed after the call": model.engine.step_seed})


def test_a_decoder_that_scored_equals_a_fresh_one_and_results_belong_to_the_caller():
    V = 1024
    p = O.init_params(vocab_size=V, layers=2, tasks="img2txt", seed=46, std=0.1)
    template = _decoder(p, V, 2)

    def inputs(B, T, seed):
        t = varied_inputs(B, T, seed, 100)
        return (t[0].half().to(DEV), t[1].half().to(DEV)) + tuple(x.to(DEV) for x in t[2:])

    def new():
        m = copy.deepcopy(template)                                            # (a new Engine each)
        m.engine.pack()
        return m
    used = new()
    gen = torch.Generator().manual_seed(8)
    held = []
    for B, T, seed in ((3, 6, 1), (2, 9, 2), (3, 6, 3)):                       # two shapes, the first one twice
        caps = [torch.randint(1, V, (int(n),), generator=gen).tolist() for n in torch.randint(0, T + 3, (B,), generator=gen)]
        with torch.no_grad():
            out = used.score(*inputs(B, T, seed), caps)
        held.append((out, [t.clone() for t in out]))
    for out, snap in held:                                                     # a later call did not write into an earlier call's results
        for a, b in zip(out, snap):
            assert torch.equal(GU.bits(a), GU.bits(b))
    assert not same_bits(dict(enumerate(held[0][0][:2])), dict(enumerate(held[2][0][:2])))      # (the two calls of one shape did differ)
    calls = (("greedy", 1, {}), ("sample", 1, dict(sample_mode="sample")), ("beam", 3, {}))
    for i, (what, beam, kw) in enumerate(calls):
        inp = inputs(3, 6, 10 + i)
        got = _decode(used, inp, 4800 + i, beam, **kw)
        want = _decode(new(), inp, 4800 + i, beam, **kw)
        d = first_difference(got, want)
        assert d is None, "%s after score(): the used decoder differs from a fresh one -- %s" % (what, d)
    report("call_sequence", calls=[c[0] for c in calls], equal_to_fresh=True)


# =====================================================================================================================================
# (5) the tool
# =====================================================================================================================================
@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    from vlp_amd.data import write_packed
    return U.tool_fixture(str(tmp_path_factory.mktemp("score_cli")), O, S, write_packed, BertConfig)


def argv(su, out, *more, batch_size=2, split=True):
    a = ["--bert_model", su["bert"], "--model_recover_path", su["ckpt"], "--packed_features", su["store"], "--token_file", su["token_file"],
         "--output_file", out, "--batch_size", str(batch_size), "--max_tgt_length", str(U.T), "--new_segment_ids", "--fp16", "--enable_butd"]
    if split:
        a += ["--src_file", su["src"], "--split", "test", "--dataset", "coco"]
    return a + list(more)


@pytest.fixture(scope="module")
def scored(tool):
    """The tool's plain run at --batch_size 2: (records, summary) as read back from the files it wrote."""
    from vlp_amd import score_img2txt as SI
    out, summ = os.path.join(tool["root"], "scores_b2.json"), os.path.join(tool["root"], "summary_b2.json")
    res = SI.main(argv(tool, out, "--summary_file", summ))
    records, summary = json.load(open(out)), json.load(open(summ))
    assert res[tool["ckpt"]]["records"] == records and res[tool["ckpt"]]["summary"] == summary
    return records, summary


def test_tool_records_equal_the_model_called_directly(tool, scored):
    from vlp_amd import decode_img2txt as D
    from vlp_amd import score_img2txt as SI
    from vlp_amd.input_prep import RawRegions
    records, _ = scored
    su = tool
    ex = su["examples"]
    assert len(records) == len(ex)
    args = SI.parse_args(argv(su, "unused"))
    model = D.build_decoder(args, D.Vocab(os.path.join(su["bert"], "vocab.txt")), torch.load(su["ckpt"], map_location="cpu"), DEV)
    _, _, input_ids, seg, pos, am = [t.to(DEV) for t in decode_inputs(1, U.T, 0, Nv=U.NV)]
    seen, worst = {}, 0.0
    for rec, (key, toks) in zip(records, ex):
        feat, box, cls = su["regions"][key]
        with torch.no_grad():
            logp, ent, rank, top_id, counted = model.score(feat.unsqueeze(0).to(DEV), RawRegions(box.unsqueeze(0).to(DEV), cls.unsqueeze(0).to(DEV)),
                                                           input_ids, seg, pos, am, [toks])
        c = counted[0].cpu()
        n = int(c.sum())
        want_lp = float(logp[0].cpu().double()[c].sum())
        image_id = int(key.split("_")[2])
        assert set(rec) == {"image_id", "index", "tokens", "truncated", "logprob", "ppl", "top1", "top5", "entropy", "caption"}
        assert rec["image_id"] == image_id and rec["index"] == seen.get(image_id, 0)
        seen[image_id] = rec["index"] + 1
        assert rec["tokens"] == n == min(len(toks) + 1, U.T) and rec["truncated"] == (len(toks) >= U.T)
        assert rec["top1"] == int((rank[0].cpu()[c] == 0).sum()) and rec["top5"] == int((rank[0].cpu()[c] < 5).sum())       # the integers: exact
        worst = max(worst, abs(rec["logprob"] - want_lp) / n)
        assert abs(rec["logprob"] - want_lp) <= 5e-6 * n, (key, rec["logprob"], want_lp)
        assert abs(rec["ppl"] - math.exp(-rec["logprob"] / n)) <= 1e-12 * rec["ppl"]
        assert abs(rec["entropy"] - float(ent[0].cpu().double()[c].sum()) / n) <= 1e-4
        words = []
        for t in toks[:U.T]:
            tok = su["tokens"][t]
            if tok.startswith("##") and words:
                words[-1] += tok[2:]
            else:
                words.append(tok)
        assert rec["caption"] == " ".join(words)
    assert sum(r["truncated"] for r in records) == 1 and max(seen.values()) == 3 and records[-1]["index"] == 2
    assert len({r["logprob"] for r in records}) == len(records)                # the rows differ: an order or batching mix-up would show
    report("tool_records", captions=len(records), logprob_abs_per_token_vs_direct=worst, bound_per_token=5e-6)


def test_tool_summary_is_the_fp64_reduction_of_the_records(scored):
    records, summary = scored
    tokens = sum(r["tokens"] for r in records)
    logprob = math.fsum(r["logprob"] for r in records)
    assert set(summary) == {"captions", "tokens", "logprob", "ppl", "top1", "top5", "entropy"}
    assert summary["captions"] == len(records) and summary["tokens"] == tokens
    assert summary["logprob"] == logprob and summary["ppl"] == math.exp(-logprob / tokens)
    assert summary["top1"] == sum(r["top1"] for r in records) / tokens and summary["top5"] == sum(r["top5"] for r in records) / tokens
    assert abs(summary["entropy"] - math.fsum(r["entropy"] * r["tokens"] for r in records) / tokens) <= 1e-12
    assert 0.0 <= summary["top1"] <= summary["top5"] <= 1.0 and summary["ppl"] > 1.0
    report("tool_summary", **summary)


def test_tool_batch_sizes_write_the_same_files(tool, scored):
    from vlp_amd import score_img2txt as SI
    out, summ = os.path.join(tool["root"], "scores_b3.json"), os.path.join(tool["root"], "summary_b3.json")
    SI.main(argv(tool, out, "--summary_file", summ, batch_size=3))
    assert json.load(open(out)) == scored[0] and json.load(open(summ)) == scored[1]
    assert open(out).read() == open(os.path.join(tool["root"], "scores_b2.json")).read()


def test_tool_selection_and_length_norm(tool, scored):
    from vlp_amd import score_img2txt as SI
    from vlp_amd.eval_captions import load_predictions
    records, _ = scored
    picks = {}
    for norm in ("none", "mean"):
        out, samples = os.path.join(tool["root"], "pick_%s.json" % norm), os.path.join(tool["root"], "samples_%s.json" % norm)
        SI.main(argv(tool, out, "--select", "likelihood", "--length_norm", norm, "--samples_file", samples))
        assert json.load(open(samples)) == records
        got = json.load(open(out))
        value = (lambda r: r["logprob"] / r["tokens"]) if norm == "mean" else (lambda r: r["logprob"])
        want = []
        for image_id in tool["test_ids"]:                                      # the images in the order of their first caption = list order
            mine = [r for r in records if r["image_id"] == image_id]
            best = max(mine, key=lambda r: (value(r), -r["index"]))
            want.append({"image_id": image_id, "caption": best["caption"], "index": best["index"], "logprob": best["logprob"]})
        assert got == want
        picks[norm] = [r["index"] for r in got]
        refs = {i: [["x"]] for i in tool["test_ids"]}
        ids, hyps = load_predictions(out, refs)[:2]
        assert list(ids) == tool["test_ids"] and len(hyps) == 5
    # a case in which the two rules disagree, built from what the first run wrote: two captions of one image, the first with the larger
    # total, the second with the larger log-probability per token
    pair = None
    for a in records:
        for b in records:
            if (pair is None and a["image_id"] == b["image_id"] and a["logprob"] > b["logprob"]
                    and a["logprob"] / a["tokens"] < b["logprob"] / b["tokens"]):
                pair = (a, b)
    assert pair is not None, [(r["image_id"], r["index"], r["tokens"], r["logprob"]) for r in records]
    of_image = [e for e in tool["examples"] if int(e[0].split("_")[2]) == pair[0]["image_id"]]
    two = os.path.join(tool["root"], "two.json")
    json.dump([of_image[pair[0]["index"]], of_image[pair[1]["index"]]], open(two, "w"))
    chosen = {}
    for norm in ("none", "mean"):
        out = os.path.join(tool["root"], "two_%s.json" % norm)
        args = argv(tool, out, "--select", "likelihood", "--length_norm", norm)
        args[args.index("--token_file") + 1] = two
        SI.main(args)
        got = json.load(open(out))
        assert len(got) == 1 and got[0]["image_id"] == pair[0]["image_id"]
        chosen[norm] = got[0]["index"]
        assert got[0]["caption"] == pair[chosen[norm]]["caption"] and got[0]["logprob"] == pair[chosen[norm]]["logprob"]
    assert chosen == {"none": 0, "mean": 1}, chosen
    report("tool_selection", picks=picks, built_pair=[(r["index"], r["tokens"], r["logprob"]) for r in pair])


def test_tool_without_a_split_scores_every_example_under_its_key(tool, scored):
    from vlp_amd import score_img2txt as SI
    out = os.path.join(tool["root"], "scores_nosplit.json")
    SI.main(argv(tool, out, batch_size=3, split=False))
    got = json.load(open(out))
    assert [r["image_id"] for r in got] == [k for k, _ in tool["examples"]]
    strip = lambda rs: [{k: v for k, v in r.items() if k != "image_id"} for r in rs]
    assert strip(got) == strip(scored[0])


def test_tool_refusals(tool, capsys):
    from vlp_amd import score_img2txt as SI
    su = tool
    never = os.path.join(su["root"], "never.json")
    base = argv(su, never)

    def drop(flag, n=2):
        i = base.index(flag)
        return base[:i] + base[i + n:]
    for args, message in ((drop("--fp16", 1), "add --fp16"), (drop("--packed_features"), "--packed_features DIR is required"),
                          (drop("--token_file"), "--token_file FILE is required"),
                          (base + ["--length_norm", "mean"], "--length_norm mean says how --select likelihood compares"),
                          (base + ["--samples_file", "s.json"], "--samples_file s.json receives the per-caption records")):
        with pytest.raises(SystemExit):
            SI.main(args)
        assert message in capsys.readouterr().err
    vqa = os.path.join(su["root"], "vqa.json")
    json.dump([[k, t, [1], n] for n, (k, t) in enumerate(su["examples"])], open(vqa, "w"))
    with pytest.raises(ValueError, match="holds VQA examples"):
        SI.main(drop("--token_file") + ["--token_file", vqa])
    stray = os.path.join(su["root"], "stray.json")
    json.dump(su["examples"] + [["COCO_val2014_000000000001", [5, 6]]], open(stray, "w"))
    with pytest.raises(KeyError, match="COCO_val2014_000000000001.*is not in the packed store"):
        SI.main([stray if a == su["token_file"] else a for a in argv(su, never, split=False)])
    assert not os.path.exists(never)
