"""GPU: the SCST policy controls -- sampling temperature and entropy bonus (vlp_token_policy_fwd / _bwd, csrc/loss.hip).

(1) the kernels against tests/scst_policy_util.policy_reference (fp64, pinned against torch autograd in tests/test_scst_policy_cpu.py) over the
    grid of the issue, on hand-built rows, bit for bit against vlp_token_logprob_fwd / _bwd at T = 1, bit-equal repeats, guard bands, refusals
    by return code with nothing written;
(2) the model: tempered draws equal Engine.decode_sample_group's, the scoring pass's log-probabilities, the entropy output and every
    parameter gradient of RewardCriterion - beta * mean_masked(H) against oracle autograd, next to the same case at T = 1, beta = 0 (the code
    path of before) which sets the bound; refusals; defaults unchanged call for call and bit for bit; a used engine equals a fresh one; an
    optimizer step, and the sign of beta;
(3) the entry script with --scst_temperature / --scst_entropy_weight.

Bounds.  Forward: tests/test_80_scst_gpu.py's 1e-4 for logp, times max(1, 1/T), the factor the logits are magnified by; the same for H.
Backward: test_80's rel metric < 2e-3.  Model: test_80's bounds for the T = 1 run, 1.5 x that run's own measured errors (x max(1, 1/T) for
log-probabilities and entropy) for the tempered run -- other draws move these errors by tens of per cent.
Every test prints what it measured through report() (pytest -s); the figures of an MI355X run are in profiles/scst_policy.json."""
import ctypes as C
import inspect
import json
import math
import os
import re

import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from oracle import vlp_oracle as O                                   # noqa: E402  (checker only)
from tests import guard_util as GU                                   # noqa: E402
from tests import scst_policy_util as PU                             # noqa: E402
from tests.test_80_scst_gpu import _decoder, rel                     # noqa: E402
from tests.test_scst_cpu import scst_inputs                          # noqa: E402
from vlp_amd import _lib as K                                        # noqa: E402
from vlp_amd import scst as SC                                       # noqa: E402
from vlp_amd import synthetic as S                                   # noqa: E402

DEV = torch.device("cuda:0")
REPORT = {}
BAD_ARG = -1                                                         # include/vlp_hip.h VLP_ERR_BAD_ARG


def report(key, **kw):
    """Prints what a test measured; with VLP_SCST_POLICY_RECORD=<json file> (profiles/scst_policy.json when the record is taken) the figures
    are also kept under that file's "test_86" key, next to the timing runs tools/scst_bench.py writes there."""
    REPORT.setdefault(key, {}).update(kw)
    print("%s: %s" % (key, json.dumps(REPORT[key], sort_keys=True)))
    path = os.environ.get("VLP_SCST_POLICY_RECORD")
    if path:
        rec = json.load(open(path)) if os.path.exists(path) else {}
        rec.setdefault("test_86", {})[key] = REPORT[key]
        with open(path, "w") as f:
            json.dump(rec, f, indent=2, sort_keys=True)


def fwd_bound(T):
    return 1e-4 * max(1.0, 1.0 / T)


def padded(x, ld, fill=30.0):
    """[R, V] fp16 -> device [R, ld] with the pad columns holding `fill`, large values the kernels must not see."""
    R, V = x.shape
    buf = torch.full((R, ld), fill, device=DEV, dtype=torch.half)
    buf[:, :V] = x.to(DEV)
    return buf


def run_fwd(logits, ld, ids, rows, V, T, entropy=True):
    out = [torch.full((rows,), float("nan"), device=DEV) for _ in range(3 if entropy else 2)]
    K.token_policy_fwd(logits, ld, ids, out[0], out[1], rows, V, temperature=T, entropy=out[2] if entropy else None)
    return out


# =====================================================================================================================================
# (1) kernels
# =====================================================================================================================================
@pytest.mark.parametrize("extra_ld", [0, 64])
@pytest.mark.parametrize("V", PU.GRID_V)
def test_policy_kernels_against_fp64_reference(V, extra_ld):
    R = 48
    ld = GU.roundup8(V) + extra_ld
    x, ids = PU.grid_rows(V, R, 11 + V)
    gen = torch.Generator().manual_seed(7 + V)
    g = torch.randn(R, generator=gen) * 512.0                         # signed, loss-scaled
    h = torch.randn(R, generator=gen) * 512.0
    logits, ids_d, g_d, h_d, zero = padded(x, ld), ids.to(DEV), g.to(DEV), h.to(DEV), torch.zeros(R, device=DEV)
    worst = dict(logp=0.0, H=0.0, lse=0.0, full=0.0, g_only=0.0, h_only=0.0)
    for T in PU.GRID_T:
        lse_r, lp_r, H_r, dg = PU.reference_rows(x, ids, T, g=g, h=None)
        _, _, _, dh = PU.reference_rows(x, ids, T, g=torch.zeros(R), h=h)
        for rows in (1, 3, 48):
            logp, lse, ent = run_fwd(logits, ld, ids_d, rows, V, T)
            e_lp = float((logp.double().cpu() - lp_r[:rows]).abs().max()) / fwd_bound(T)
            e_H = float((ent.double().cpu() - H_r[:rows]).abs().max()) / fwd_bound(T)
            e_lse = float(((lse.double().cpu() - lse_r[:rows]).abs() / lse_r[:rows].abs().clamp(min=1.0)).max())
            worst.update(logp=max(worst["logp"], e_lp), H=max(worst["H"], e_H), lse=max(worst["lse"], e_lse))
            assert e_lp <= 1.0 and e_H <= 1.0, (V, ld, rows, T, e_lp, e_H)
            assert e_lse < 1e-5, (V, ld, rows, T, e_lse)
            assert float(ent.min()) >= -fwd_bound(T) and float(ent.max()) <= math.log(V) + fwd_bound(T)
            for name, gg, hh, want in (("full", g_d, h_d, dg + dh), ("g_only", g_d, None, dg), ("h_only", zero, h_d, dh)):
                dl = torch.full((R, ld), 7.0, device=DEV, dtype=torch.half)
                K.token_policy_bwd(logits, ld, ids_d, lse, gg, dl, ld, rows, V, temperature=T, h=hh, entropy=None if hh is None else ent)
                assert bool((dl[:rows, V:] == 0).all()), (name, V, ld, rows, T)         # every pad column ends at 0
                assert bool((dl[rows:] == 7.0).all()), (name, V, ld, rows, T)            # rows past `rows` are not this launch's
                got = dl[:rows, :V].double().cpu()
                assert bool(torch.isfinite(got).all())
                if V == 1:                  # one class: q = 1 and the gradient vanishes, up to the forward's error in log q times the scale
                    assert float(got.abs().max()) <= float((g.abs() + h.abs()).max()) / T * fwd_bound(T), (name, T)
                    continue
                e = rel(got, want[:rows])
                worst[name] = max(worst[name], e)
                assert e < 2e-3, (name, V, ld, rows, T, e)
    report("kernels_V%d_ld%d" % (V, ld), fwd_logp_over_bound=worst["logp"], fwd_H_over_bound=worst["H"], lse_rel=worst["lse"],
           bwd_rel_full=worst["full"], bwd_rel_g_only=worst["g_only"], bwd_rel_h_only=worst["h_only"], bwd_bound=2e-3)


@pytest.mark.parametrize("T", [0.5, 2.0])
def test_policy_kernels_hand_built_rows(T):
    V, ld = 1000, 1000 + 64
    rows = PU.hard_rows(V)
    names = list(rows)
    x = torch.stack([rows[n][0] for n in names])
    ids = torch.tensor([rows[n][1] for n in names])
    R = len(names)
    g, h = torch.full((R,), 1.25 * 512.0), torch.full((R,), -0.75 * 512.0)
    logits, ids_d = padded(x, ld), ids.to(DEV)
    logp, lse, ent = run_fwd(logits, ld, ids_d, R, V, T)
    dl = torch.full((R, ld), 7.0, device=DEV, dtype=torch.half)
    K.token_policy_bwd(logits, ld, ids_d, lse, g.to(DEV), dl, ld, R, V, temperature=T, h=h.to(DEV), entropy=ent)
    dl_h = torch.full((R, ld), 7.0, device=DEV, dtype=torch.half)
    K.token_policy_bwd(logits, ld, ids_d, lse, torch.zeros(R, device=DEV), dl_h, ld, R, V, temperature=T, h=h.to(DEV), entropy=ent)
    for t in (logp, lse, ent, dl, dl_h):
        assert bool(torch.isfinite(t).all())                                             # all outputs finite, on every row
    assert bool((dl[:, V:] == 0).all()) and bool((dl_h[:, V:] == 0).all())
    lse_r, lp_r, H_r, d_r = PU.reference_rows(x, ids, T, g=g, h=h)
    lp, H, dlc, dlhc = logp.double().cpu(), ent.double().cpu(), dl[:, :V].double().cpu(), dl_h[:, :V].double().cpu()
    b = fwd_bound(T)
    i = names.index("all_equal")
    assert abs(float(H[i]) - math.log(V)) <= b and abs(float(lp[i]) + math.log(V)) <= b
    # dH/dz = -q (log q + H) is 0 on a uniform row: what is left is (|h| / T) q times the forward's error in log q + H, and fp16's smallest step
    zero_bound = float(h.abs().max()) / T * (1.0 / V) * 2 * b + 2.0 ** -24
    assert float(dlhc[i].abs().max()) <= zero_bound, (float(dlhc[i].abs().max()), zero_bound)
    i = names.index("one_peak")
    assert abs(float(H[i]) - float(H_r[i])) <= b and abs(float(H[i])) <= 1e-3 + b
    i = names.index("third_minus_inf")
    dead = ~torch.isfinite(x[i].double())
    assert int(dead.sum()) >= V // 3 and bool((dlc[i][dead] == 0).all()) and bool((dlhc[i][dead] == 0).all())     # exactly 0
    assert abs(float(H[i]) - float(H_r[i])) <= b and abs(float(lp[i]) - float(lp_r[i])) <= b
    assert rel(dlc[i], d_r[i]) < 2e-3
    i = names.index("one_finite")
    assert abs(float(lp[i])) <= b and abs(float(H[i])) <= b and bool((dlc[i] == 0).all()) and bool((dlhc[i] == 0).all())
    i = names.index("span_fp16")
    report("hand_rows_T%g" % T, all_equal_H_err=abs(float(H[names.index("all_equal")]) - math.log(V)),
           all_equal_dH_abs=float(dlhc[names.index("all_equal")].abs().max()), all_equal_dH_bound=zero_bound,
           one_peak_H=float(H[names.index("one_peak")]), one_finite_logp=float(lp[names.index("one_finite")]),
           span_logp_err=abs(float(lp[i]) - float(lp_r[i])), span_H=float(H[i]), fwd_bound=b)
    # V = 1: the only column has probability 1
    one = padded(torch.tensor([[3.0], [-2.5]]).half(), 8)
    id1 = torch.tensor([0, 4], device=DEV)
    logp, lse, ent = run_fwd(one, 8, id1, 2, 1, T)
    dl = torch.full((2, 8), 7.0, device=DEV, dtype=torch.half)
    K.token_policy_bwd(one, 8, id1, lse, g[:2].to(DEV), dl, 8, 2, 1, temperature=T, h=h[:2].to(DEV), entropy=ent)
    assert float(logp.abs().max()) <= b and float(ent.abs().max()) <= b and bool((dl == 0).all())


def test_policy_kernels_at_T1_equal_token_logprob_bit_for_bit_and_repeat():
    R, V, ld = 48, 28996, 29056
    x, ids = PU.grid_rows(V, R, 11)
    logits, ids_d = padded(x, ld), ids.to(DEV)
    g = (torch.randn(R, generator=torch.Generator().manual_seed(2)) * 512.0).to(DEV)
    logp0, lse0 = torch.zeros(R, device=DEV), torch.zeros(R, device=DEV)
    K.token_logprob_fwd(logits, ld, ids_d, logp0, lse0, R, V)
    dl0 = torch.full((R, ld), 7.0, device=DEV, dtype=torch.half)
    K.token_logprob_bwd(logits, ld, ids_d, lse0, g, dl0, ld, R, V)
    logp1, lse1 = run_fwd(logits, ld, ids_d, R, V, 1.0, entropy=False)
    dl1 = torch.full((R, ld), 7.0, device=DEV, dtype=torch.half)
    K.token_policy_bwd(logits, ld, ids_d, lse1, g, dl1, ld, R, V, temperature=1.0)
    assert torch.equal(GU.bits(logp0), GU.bits(logp1)) and torch.equal(GU.bits(lse0), GU.bits(lse1))
    assert torch.equal(GU.bits(dl0), GU.bits(dl1))
    # two launches on the same inputs: the same bits in every output, with the entropy and h as well
    h = (torch.randn(R, generator=torch.Generator().manual_seed(3)) * 512.0).to(DEV)
    outs = []
    for _ in range(2):
        logp, lse, ent = run_fwd(logits, ld, ids_d, R, V, 0.7)
        dl = torch.full((R, ld), 7.0, device=DEV, dtype=torch.half)
        K.token_policy_bwd(logits, ld, ids_d, lse, g, dl, ld, R, V, temperature=0.7, h=h, entropy=ent)
        outs.append((logp, lse, ent, dl))
    for a, b in zip(*outs):
        assert torch.equal(GU.bits(a), GU.bits(b))
    report("T1_bits", equal=True, repeat_equal=True)


@pytest.mark.parametrize("R,V,pad", [(48, 28996, 64), (3, 257, 24), (2, 7, 0)])
def test_policy_kernels_guard_bands(R, V, pad):
    T = 0.7
    x, ids = PU.grid_rows(V, R, 31 + V)
    ld = GU.roundup8(V) + pad
    logits = GU.guarded(R, V, ld=ld, dtype=torch.half, fill="nan", device=DEV).set(x.to(DEV))       # NaN padding and guards: never read
    ids_g = GU.guarded_vec(R, torch.long, fill=0, device=DEV).set(ids.to(DEV))
    outs = {n: GU.guarded_vec(R, torch.float32, fill="sentinel", device=DEV) for n in ("logp", "lse", "entropy")}
    K.token_policy_fwd(logits.view, ld, ids_g.vec, outs["logp"].vec, outs["lse"].vec, R, V, temperature=T, entropy=outs["entropy"].vec)
    for n, gd in outs.items():
        GU.assert_written(gd, "logical", n)
        GU.assert_finite(gd.vec, n)
        GU.assert_untouched(gd, written="logical", name=n)
    gen = torch.Generator().manual_seed(5)
    gv = GU.guarded_vec(R, torch.float32, fill="nan", device=DEV).set((torch.randn(R, generator=gen) * 512.0).to(DEV))
    hv = GU.guarded_vec(R, torch.float32, fill="nan", device=DEV).set((torch.randn(R, generator=gen) * 512.0).to(DEV))
    lse_in = GU.guarded_vec(R, torch.float32, fill="nan", device=DEV).set(outs["lse"].vec.clone())
    ent_in = GU.guarded_vec(R, torch.float32, fill="nan", device=DEV).set(outs["entropy"].vec.clone())
    dl = GU.guarded(R, V, ld=ld, dtype=torch.half, fill="sentinel", device=DEV)
    K.token_policy_bwd(logits.view, ld, ids_g.vec, lse_in.vec, gv.vec, dl.view, ld, R, V, temperature=T, h=hv.vec, entropy=ent_in.vec)
    GU.assert_written(dl, "rows", "dlogits")
    GU.assert_finite(dl.view, "dlogits")
    GU.assert_zero_band(dl, V, ld, "dlogits")
    GU.assert_untouched(dl, written="rows", name="dlogits")
    for gd, n in ((logits, "logits"), (ids_g, "ids"), (gv, "g"), (hv, "h"), (lse_in, "lse"), (ent_in, "entropy")):
        GU.assert_untouched(gd, name=n)
    _, _, _, want = PU.reference_rows(x, ids, T, g=gv.vec.cpu(), h=hv.vec.cpu())
    assert rel(dl.view.double().cpu(), want) < 2e-3


def test_policy_kernels_refuse_by_return_code_and_write_nothing():
    R, V, ld = 3, 40, 40
    lib = K.load()
    logits = torch.zeros(R, ld + 8, device=DEV, dtype=torch.half)
    ids = torch.zeros(R, dtype=torch.long, device=DEV)
    outs = [torch.full((R,), 5.0, device=DEV) for _ in range(3)]
    lse, ent, g, h = (torch.zeros(R, device=DEV) for _ in range(4))
    dl = torch.full((R, ld), 7.0, device=DEV, dtype=torch.half)
    p, sp = K.ptr, K.stream_ptr()

    def fwd(T=0.7, ld_=ld, logp=outs[0], entropy=outs[2]):
        a = K.TokenPolicyFwdArgs(p(logits), ld_, p(ids), p(logp), p(outs[1]), p(entropy), R, V, T)
        return lib.vlp_token_policy_fwd(C.byref(a), sp)

    def bwd(T=0.7, ld_=ld, ldd=ld, g_=g, h_=h, ent_=ent):
        a = K.TokenPolicyBwdArgs(p(logits), ld_, p(ids), p(lse), p(ent_), p(g_), p(h_), p(dl), ldd, R, V, T)
        return lib.vlp_token_policy_bwd(C.byref(a), sp)
    codes = {}
    for T in (0.0, -1.0, float("inf"), float("nan"), 1e-40):              # the last: subnormal in fp32, its reciprocal overflows
        codes["fwd T=%r" % T], codes["bwd T=%r" % T] = fwd(T=T), bwd(T=T)
    codes["fwd ld%8"], codes["bwd ld%8"], codes["bwd ldd%8"] = fwd(ld_=ld + 4), bwd(ld_=ld + 4), bwd(ldd=ld + 4)
    codes["bwd h without entropy"] = bwd(ent_=None)
    codes["fwd null logp"], codes["bwd null g"] = fwd(logp=None), bwd(g_=None)
    torch.cuda.synchronize()
    report("refusals", codes=codes)
    assert all(c == BAD_ARG for c in codes.values()), codes
    assert all(bool((o == 5.0).all()) for o in outs) and bool((dl == 7.0).all())          # nothing was written
    assert fwd() == 0 and bwd() == 0 and fwd(entropy=None) == 0 and bwd(h_=None, ent_=None) == 0 and bwd(h_=None) == 0
    torch.cuda.synchronize()


# =====================================================================================================================================
# (2) the model
# =====================================================================================================================================
def _grad_errors(m, pd, scale):
    errs = {}
    grads = {n: (q.grad.float() / scale) for n, q in m.named_parameters()}
    for k, t in pd.items():
        if t.grad is None:
            continue
        if k.endswith("attention.self.key.bias"):     # true value 0: bounded against the sibling query-bias gradient (as test_80 does)
            d, qb = (grads[k] - t.grad).double(), pd[k.replace("key.bias", "query.bias")].grad.double()
            errs[k] = max(float(d.abs().max() / qb.abs().max()), float(d.norm() / qb.norm()))
        else:
            errs[k] = rel(grads[k], t.grad)
    worst = max(errs, key=errs.get)
    return worst, errs[worst]


def _policy_run(m, p, dv, Ks, T, beta, seed, s0):
    """One train-mode sampled forward + backward of loss = RewardCriterion - beta * mean_masked(H) (loss scale 1024) at temperature T, and
    the oracle's autograd of the same loss on the same ids, drawn from step seed s0.  Returns the measured errors."""
    eng = m.engine
    img16, vpe16 = dv[0].half(), dv[1].half()
    m.train()
    eng.step_seed = s0
    with torch.no_grad():                                   # the decoder's own draw and log-probs (same seeds as the call below)
        if Ks > 1 or T != 1.0:
            ids_d, lp_d = eng.decode_sample_group(img16, vpe16, dv[2], dv[3], dv[4], dv[5], S.MASK_ID, Ks, temperature=T)
        else:
            ids_d, lp_d = eng.decode_greedy(img16, vpe16, dv[2], dv[3], dv[4], dv[5], S.MASK_ID, sample=True)
        ids_d, lp_d = ids_d.clone(), lp_d.clone()
    eng.step_seed = s0
    kw = {}
    if Ks > 1:
        kw["n_samples"] = Ks
    if T != 1.0:
        kw["temperature"] = T
    ent = None
    if beta > 0:
        ids, logp, ent = m(img16, vpe16, *dv[2:], sample_mode="sample", return_entropy=True, **kw)
        assert ent.requires_grad and tuple(ent.shape) == tuple(logp.shape) == tuple(ids.shape)
    else:
        ids, logp = m(img16, vpe16, *dv[2:], sample_mode="sample", **kw)
    assert logp.requires_grad and logp.grad_fn is not None
    assert torch.equal(ids, ids_d)                          # bit for bit the decoder's draws
    B, n = dv[2].shape[0], ids.shape[1]
    gen = SC.clean_captions(ids, S.SEP_ID)
    g = torch.Generator().manual_seed(seed)
    reward = (torch.randn(Ks * B, 1, generator=g) * 2.0).expand(Ks * B, n).to(DEV)
    eng.zero_grad()
    loss, _ = SC.policy_loss(logp, gen, reward, entropy=ent, entropy_weight=beta)
    (loss * 1024.0).backward()
    torch.cuda.synchronize()
    pd = {k: v.to(DEV).half().float().requires_grad_(True) for k, v in p.items()}

    def tiled(t):
        return t if Ks == 1 else t.repeat(Ks, *([1] * (t.dim() - 1)))
    vf, vp = O.vis_embed(pd, tiled(img16).float()), O.vis_pe_embed(pd, tiled(vpe16).float())
    logits_o = PU.forced_decode_logits(O, pd, vf, vp, *[tiled(t) for t in dv[2:]], ids, S.MASK_ID)
    lp_o, H_o = PU.tempered_logp_entropy(logits_o, ids, T)
    loss_o, _ = SC.policy_loss(lp_o, gen, reward, entropy=H_o if beta > 0 else None, entropy_weight=beta)
    loss_o.backward()
    assert {k for k, t in pd.items() if t.grad is None} <= eng.unused_parameter_names()
    worst, e_g = _grad_errors(m, pd, 1024.0)
    out = dict(logp_vs_decoder=float((logp.detach() - lp_d).abs().max()), logp_vs_oracle=float((logp.detach() - lp_o.detach()).abs().max()),
               worst_grad=worst, worst_grad_rel=e_g, loss=float(loss.detach()), loss_oracle=float(loss_o.detach()))
    if ent is not None:
        out.update(entropy_vs_oracle=float((ent.detach() - H_o.detach()).abs().max()), entropy_min=float(ent.detach().min()), entropy_max=float(ent.detach().max()))
    return out


# The first case is test_80's _model_case, draw for draw.  The log-probability figures are maxima over the sampled positions of the fp16 logits'
# evaluation noise, and test_80's bounds were measured on 5 x 13 = 65 positions; the 12 rows of the second case get max_len_b = 4, 12 x 5 = 60
# positions, so that its maxima are taken over as many draws as the bounds were made for.
@pytest.mark.parametrize("layers,B,Ks,seed,max_len_b", [(3, 5, 1, 21, 12), (2, 4, 3, 21, 4)])
def test_model_tempered_policy_and_entropy_vs_oracle(layers, B, Ks, seed, max_len_b):
    V, T, beta = 1024, 0.7, 0.05
    p = O.init_params(vocab_size=V, layers=layers, seed=seed, std=0.05)
    m = _decoder(p, V, layers)
    img, vis_pe, prefix, seg, pos, am, _, _ = scst_inputs(B, max_len_b, seed, V, short=(1,), ragged=((0, 41),), pos_offset=2)
    dv = [t.to(DEV) for t in (img, vis_pe, prefix, seg, pos, am)]
    s0 = m.engine.step_seed                                        # a fresh engine's, as in test_80
    base = _policy_run(m, p, dv, Ks, 1.0, 0.0, seed, s0)           # the code path of before: it sets the bound
    report("model_%dl_K%d_base" % (layers, Ks), **base)
    assert base["logp_vs_decoder"] < 0.0048 and base["logp_vs_oracle"] < 0.0036 and base["worst_grad_rel"] < 0.07, base      # test_80's bounds
    got = _policy_run(m, p, dv, Ks, T, beta, seed, s0)
    mag = max(1.0, 1.0 / T)
    bounds = dict(logp_vs_decoder=min(0.0048 * mag, 1.5 * base["logp_vs_decoder"] * mag), logp_vs_oracle=1.5 * base["logp_vs_oracle"] * mag,
                  entropy_vs_oracle=1.5 * base["logp_vs_oracle"] * mag, worst_grad_rel=1.5 * base["worst_grad_rel"])
    report("model_%dl_K%d_T%g_beta%g" % (layers, Ks, T, beta), bounds=bounds, **got)
    for k, b in bounds.items():
        assert got[k] < b, (k, got[k], b)
    assert got["entropy_min"] >= 0.0 and got["entropy_max"] <= math.log(V) + 1e-3


def _small_case(seed=4, B=4, max_len_b=8, biased=False):
    V = 1024
    p = O.init_params(vocab_size=V, layers=2, seed=seed, std=0.05)
    if biased:                                  # a peaked policy: seven words carry the mass, so the entropy has room to rise
        p["cls.predictions.bias"][300:306] = 8.0
        p["cls.predictions.bias"][S.SEP_ID] = 7.0
    img, vis_pe, prefix, seg, pos, am, _, _ = scst_inputs(B, max_len_b, 6, V)
    dv = [t.to(DEV) for t in (img, vis_pe, prefix, seg, pos, am)]
    return p, [dv[0].half(), dv[1].half()] + dv[2:]


def test_model_refusals():
    p, dv = _small_case()
    m = _decoder(p, 1024, 2)
    m.eval()
    with pytest.raises(ValueError, match="return_entropy"):
        m(*dv, sample_mode="sample", return_entropy=True)
    with pytest.raises(ValueError, match="return_entropy"):
        m(*dv, sample_mode="sample", temperature=0.7, return_entropy=True)
    m.train()
    with torch.no_grad():
        with pytest.raises(ValueError, match="return_entropy"):
            m(*dv, sample_mode="sample", return_entropy=True)
    with pytest.raises(ValueError, match="return_entropy"):
        m(*dv, sample_mode="greedy", return_entropy=True)
    with pytest.raises(ValueError, match="train"):
        m(*dv, sample_mode="sample", temperature=0.7, top_k=5)
    mb = _decoder(p, 1024, 2).train()
    mb.search_beam_size = 2
    with pytest.raises(ValueError, match="beam"):
        mb(*dv, sample_mode="sample", return_entropy=True)
    gen0 = m.engine.gen
    ids, logp, ent = m(*dv, sample_mode="sample", return_entropy=True)          # and what is accepted
    assert m.engine.gen == gen0 + 1 and ent.requires_grad and logp.requires_grad


def _optimizer(m, lr=1e-4):
    from vlp_amd.optimization_fp16 import FP16_Optimizer_State, FusedAdam
    named = list(m.named_parameters())
    nd = ["bias", "LayerNorm.bias", "LayerNorm.weight"]
    groups = [{"params": [q for n, q in named if not any(x in n for x in nd)], "weight_decay": 0.01},
              {"params": [q for n, q in named if any(x in n for x in nd)], "weight_decay": 0.0}]
    return FP16_Optimizer_State(FusedAdam(groups, lr=lr, bias_correction=False, max_grad_norm=1.0), dynamic_loss_scale=True)


def _step_case(V=1024, B=4, max_len_b=12):
    p = O.init_params(vocab_size=V, layers=2, seed=21, std=0.05)
    p["cls.predictions.bias"][300:306] = 8.0                  # samples that overlap with the references: rewards that are not all zero
    p["cls.predictions.bias"][S.SEP_ID] = 7.0
    batch = S.batch_to(S.make_batch(B, max_len_b=max_len_b, len_vis_input=100, vocab_size=V, max_pred=0, mask_prob=0.0, seed=7), DEV, half=True)
    gen = torch.Generator().manual_seed(5)
    ids = batch.input_ids.clone()
    for b in range(B):
        n = int(torch.randint(3, max_len_b + 1, (1,), generator=gen))
        row = [int(t) for t in torch.randint(300, 306, (n,), generator=gen)] + [S.SEP_ID]
        ids[b, 102:] = torch.tensor(row + [0] * (max_len_b + 1 - len(row)), device=DEV)
    return p, batch._replace(input_ids=ids)


def _fresh(p):
    torch.manual_seed(3)
    m = _decoder(p, 1024, 2).train()
    m.engine.step_seed = 1234
    return m, _optimizer(m)


def _recorded_step(monkeypatch, m, opt, batch, samples, **kw):
    """scst_step (gradients kept: accumulate=True) with every _lib wrapper recording its name.  Returns (calls, plan keys, loss, reward,
    gradients)."""
    from vlp_amd import run_img2txt_dist as R
    calls = []
    with monkeypatch.context() as mp:
        for name, fn in list(vars(K).items()):
            if inspect.isfunction(fn) and fn.__module__ == K.__name__ and not name.startswith("_") and name not in ("load", "ptr", "stream_ptr"):
                def rec(*a, _fn=fn, _name=name, **k):
                    calls.append(_name)
                    return _fn(*a, **k)
                mp.setattr(K, name, rec)
        loss, mean_r = R.scst_step(m, opt, batch, 1e-4, 100, SC.RewardCriterion(), accumulate=True, reward_on="device", samples=samples, **kw)
        torch.cuda.synchronize()
    plans = {str(k): sorted(map(str, ws["plans"])) for k, ws in m.engine._ws.items() if isinstance(ws, dict) and "plans" in ws}
    grads = {n: q.grad.detach().clone() for n, q in m.named_parameters() if q.grad is not None}
    return calls, plans, loss.detach().clone(), mean_r.detach().clone(), grads


def _same_step(a, b):
    assert a[0] == b[0], [(i, x, y) for i, (x, y) in enumerate(zip(a[0], b[0])) if x != y][:3]       # the same _lib calls in the same order
    assert a[1] == b[1]                                                                              # the same decode plan keys
    assert torch.equal(GU.bits(a[2]), GU.bits(b[2])) and torch.equal(GU.bits(a[3]), GU.bits(b[3]))   # loss, reward
    assert a[4].keys() == b[4].keys() and all(torch.equal(GU.bits(a[4][k]), GU.bits(b[4][k])) for k in a[4])


@pytest.mark.parametrize("samples", [1, 3])
def test_defaults_issue_the_same_calls_and_bits(monkeypatch, samples):
    p, batch = _step_case()
    m0, o0 = _fresh(p)
    plain = _recorded_step(monkeypatch, m0, o0, batch, samples)
    m1, o1 = _fresh(p)
    named = _recorded_step(monkeypatch, m1, o1, batch, samples, temperature=1.0, entropy_weight=0.0)
    _same_step(plain, named)
    assert "token_logprob_fwd" in plain[0] and "token_logprob_bwd" in plain[0]
    assert "token_policy_fwd" not in plain[0] and "token_policy_bwd" not in plain[0]
    assert any(bool(g.ne(0).any()) for g in plain[4].values())
    # a used engine equals a fresh one: a (0.7, 0.05) step, then the default step, against `plain`
    m2, o2 = _fresh(p)
    stats = {}
    used = _recorded_step(monkeypatch, m2, o2, batch, samples, temperature=0.7, entropy_weight=0.05, stats=stats)
    assert "token_policy_fwd" in used[0] and "token_policy_bwd" in used[0] and "token_logprob_fwd" not in used[0]
    assert math.isfinite(float(stats["entropy"])) and 0.0 <= float(stats["entropy"]) <= math.log(1024) + 1e-3
    o2.zero_grad()
    m2.engine.zero_grad()
    m2.engine.step_seed = 1234
    again = _recorded_step(monkeypatch, m2, o2, batch, samples)          # (its call list lacks the first call's one-time set-up)
    assert torch.equal(GU.bits(again[2]), GU.bits(plain[2])) and torch.equal(GU.bits(again[3]), GU.bits(plain[3]))
    assert all(torch.equal(GU.bits(again[4][k]), GU.bits(plain[4][k])) for k in plain[4])
    report("defaults_samples%d" % samples, calls=len(plain[0]), loss=float(plain[2]), mean_reward=float(plain[3]),
           policy_step_loss=float(used[2]), policy_step_entropy=float(stats["entropy"]))


def test_optimizer_step_and_the_sign_of_the_entropy_weight():
    from vlp_amd import run_img2txt_dist as R
    p, batch = _step_case()
    m, opt = _fresh(p)
    before = {n: q.detach().clone() for n, q in m.named_parameters()}
    stats = {}
    skipped0 = getattr(opt, "skipped_steps", None)
    loss, mean_r = R.scst_step(m, opt, batch, 1e-4, 100, SC.RewardCriterion(), reward_on="device", temperature=0.7, entropy_weight=0.05, stats=stats)
    torch.cuda.synchronize()
    assert math.isfinite(float(loss.detach())) and math.isfinite(float(mean_r)) and math.isfinite(float(stats["entropy"]))
    changed = [n for n, q in m.named_parameters() if not torch.equal(q.detach(), before[n])]
    assert "bert.embeddings.word_embeddings.weight" in changed and "bert.encoder.layer.0.attention.self.query.weight" in changed      # no overflow skip
    if skipped0 is not None:
        assert opt.skipped_steps == skipped0
    # beta's sign: reward 0 everywhere, so the only gradient is the bonus's; a few steps raise the masked mean entropy.  The steps must be
    # small for that first-order statement to hold: without bias correction Adam's first updates move every weight by about 3.2 x lr
    # (0.1 g / sqrt(0.001 g^2)), and a logit sums 768 such moves, so lr = 1e-5 changes a logit by at most 0.025 per step
    _, dv = _small_case(B=4, max_len_b=12)
    m, opt = _fresh(p)
    for grp in opt.param_groups:
        grp["lr"] = 1e-5
    hs = []
    for it in range(6):
        m.engine.step_seed = 1234                            # the same draws, as far as the moving policy allows
        ids, logp, ent = m(*dv, sample_mode="sample", return_entropy=True)
        gen = SC.clean_captions(ids, S.SEP_ID)
        loss, mean_h = SC.policy_loss(logp, gen, torch.zeros_like(logp), entropy=ent, entropy_weight=0.1)
        hs.append(float(mean_h))
        opt.backward(loss)
        opt.step()
        opt.zero_grad()
    report("entropy_weight_sign", mean_entropy_per_step=hs, changed=len(changed))
    assert all(math.isfinite(v) for v in hs) and hs[-1] > hs[0], hs


# =====================================================================================================================================
# (3) the entry script
# =====================================================================================================================================
def test_entry_script_with_temperature_and_entropy_weight(tmp_path):
    from tests.test_80_scst_gpu import BASE, _ce_checkpoint
    from vlp_amd import run_img2txt_dist as R
    ckpt = _ce_checkpoint(R, tmp_path)
    out = os.path.join(tmp_path, "scst")
    R.main(BASE + ["--scst", "--scst_temperature", "0.8", "--scst_entropy_weight", "0.01", "--scst_samples", "3", "--scst_reward", "device",
                   "--synthetic", "3", "--learning_rate", "1e-4", "--model_recover_path", ckpt, "--output_dir", out, "--num_train_epochs", "1"])
    log = open(os.path.join(out, "training.log")).read()
    rows = re.findall(r"Loss (\S+), Mean R (\S+), Mean H (\S+)", log)
    vals = [[float(v.rstrip(",")) for v in r] for r in rows]
    report("entry_policy", rows=vals)
    assert len(vals) == 3 and all(math.isfinite(v) and abs(v) < 1e4 for r in vals for v in r), log
    assert all(0.0 <= r[2] <= math.log(28996) + 1e-3 for r in vals)
    assert os.path.exists(os.path.join(out, "model.1.bin"))
