"""CPU: the SCST policy controls (--scst_temperature, --scst_entropy_weight).

(1) tests/scst_policy_util.policy_reference, the fp64 restatement the GPU tests check the kernels against, itself against fp64 torch autograd
    of g * logp + h * H on the fp16 row, over the grid and the hard rows (rows with -inf columns included);
(2) vlp_amd.scst.policy_loss against a plain fp64 expression and its autograd; weight 0 is RewardCriterion's value bit for bit;
(3) the two flags: parser defaults and types, derive_args' refusals and an accepted combination;
(4) the two argument structs against gcc's layout, the declarations compiled as C, the names in _lib.SYMBOLS.
Every test prints what it measured (pytest -s)."""
import math
import os
import subprocess

import pytest
import torch

from tests import scst_policy_util as PU
from vlp_amd import scst as SC


def _autograd(row16, id, T, g, h):
    """lse, logp, H and d(g logp + h H)/dl by fp64 torch autograd on the row; -inf columns are left out of the graph (their gradient is 0)."""
    l = row16.double()
    V = l.numel()
    i = min(max(int(id), 0), V - 1)
    live = torch.isfinite(l)
    x = l[live].clone().requires_grad_(True)
    z = x / T
    lp = torch.log_softmax(z, 0)
    q = lp.exp()
    H = -(torch.where(q > 0, q * lp, torch.zeros_like(q))).sum()
    pos = int(live[:i].sum())
    assert bool(live[i])
    (g * lp[pos] + h * H).backward()
    grad = torch.zeros(V, dtype=torch.float64)
    grad[live] = x.grad
    return float(torch.logsumexp(z.detach(), 0)), float(lp[pos].detach()), float(H.detach()), grad


def test_policy_reference_vs_fp64_autograd():
    worst = {"lse": 0.0, "logp": 0.0, "H": 0.0, "dlogits": 0.0}
    cases = []
    for V in PU.GRID_V:
        x, ids = PU.grid_rows(V, 3, 100 + V)
        cases += [(x[r], int(ids[r])) for r in range(3)]
    for V in (1, 1000):
        cases += [v for k, v in PU.hard_rows(V).items() if V > 1 or k in ("all_equal", "one_finite")]
    for row, id in cases:
        for T in PU.GRID_T:
            for g, h in ((1.3 * 512, -0.7 * 512), (-2.0, 0.0), (0.0, 3.0)):
                ref = PU.policy_reference(row, id, T, g, h)
                lse, lp, H, grad = _autograd(row, id, T, g, h)
                scale = max(1.0, abs(lse))
                worst["lse"] = max(worst["lse"], abs(ref["lse"] - lse) / scale)
                worst["logp"] = max(worst["logp"], abs(ref["logp"] - lp) / max(1.0, abs(lp)))
                worst["H"] = max(worst["H"], abs(ref["H"] - H))
                worst["dlogits"] = max(worst["dlogits"], float((ref["dlogits"] - grad).abs().max()) / max(1.0, float(grad.abs().max())))
                assert math.isfinite(ref["H"]) and bool(torch.isfinite(ref["dlogits"]).all())
                assert bool((ref["dlogits"][~torch.isfinite(row.double())] == 0).all())
    print("policy_reference vs autograd:", worst)
    assert max(worst.values()) < 1e-10, worst         # fp64 on both sides: two orders of summation of <= 28 996 terms


def test_policy_reference_hand_values():
    V = 1000
    rows = PU.hard_rows(V)
    for T in (0.5, 2.0):
        r = PU.policy_reference(*rows["all_equal"], T, 1.0, 1.0)
        assert abs(r["H"] - math.log(V)) < 1e-12 and abs(r["logp"] + math.log(V)) < 1e-12
        r = PU.policy_reference(*rows["one_finite"], T, 2.0, 3.0)
        assert r["logp"] == 0.0 and r["H"] == 0.0 and bool((r["dlogits"] == 0).all())
        r = PU.policy_reference(*rows["one_peak"], T)
        assert 0.0 <= r["H"] < 1e-3
        r = PU.policy_reference(*rows["span_fp16"], T, 1.0, 1.0)
        assert math.isfinite(r["lse"]) and bool(torch.isfinite(r["dlogits"]).all())


def test_policy_loss_vs_plain_expression():
    gen = torch.Generator().manual_seed(3)
    B, T = 6, 9
    seq = torch.randint(1, 50, (B, T), generator=gen)
    seq[0, 3:] = 0
    seq[2, 0:] = 0
    seq[4, 8] = 0
    reward = torch.randn(B, 1, generator=gen).expand(B, T)
    logp = (-torch.rand(B, T, generator=gen, dtype=torch.float64) * 5).requires_grad_(True)
    H = (torch.rand(B, T, generator=gen, dtype=torch.float64) * 6).requires_grad_(True)
    w = 0.05
    loss, mean_h = SC.policy_loss(logp, seq, reward, entropy=H, entropy_weight=w)
    loss.backward()
    lp2, H2 = logp.detach().clone().requires_grad_(True), H.detach().clone().requires_grad_(True)
    mask = torch.ones(B, T, dtype=torch.float64)
    mask[:, 1:] = (seq[:, :-1] > 0).double()
    want = -(lp2 * reward.double() * mask).sum() / mask.sum() - w * (H2 * mask).sum() / mask.sum()
    want.backward()
    errs = dict(loss=abs(float(loss.detach()) - float(want.detach())), dlogp=float((logp.grad - lp2.grad).abs().max()), dH=float((H.grad - H2.grad).abs().max()),
                mean_h=abs(float(mean_h) - float((H2 * mask).sum() / mask.sum())))
    print("policy_loss vs plain fp64:", errs)
    assert max(errs.values()) < 1e-14
    assert not mean_h.requires_grad
    assert torch.equal(SC.reward_mask(seq, torch.float64), mask)
    # weight 0: RewardCriterion's value, bit for bit, with and without the entropy
    lp32 = logp.detach().float()
    base = SC.RewardCriterion()(lp32, seq, reward)
    for ent in (None, H.detach().float()):
        got, mh = SC.policy_loss(lp32, seq, reward, entropy=ent, entropy_weight=0.0)
        assert torch.equal(got, base) and (mh is None) == (ent is None)
    for bad in (-0.1, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            SC.policy_loss(lp32, seq, reward, entropy=H.detach().float(), entropy_weight=bad)
    with pytest.raises(ValueError):
        SC.policy_loss(lp32, seq, reward, entropy=None, entropy_weight=0.1)


BASE = ["--enable_butd", "--fp16", "--max_pred", "0", "--mask_prob", "0"]


def test_flags_defaults_and_types():
    from vlp_amd import run_img2txt_dist as R
    a = R.build_parser().parse_args(BASE)
    assert a.scst_temperature == 1.0 and isinstance(a.scst_temperature, float)
    assert a.scst_entropy_weight == 0.0 and isinstance(a.scst_entropy_weight, float)
    a = R.build_parser().parse_args(BASE + ["--scst_temperature", "0.8", "--scst_entropy_weight", "0.01"])
    assert (a.scst_temperature, a.scst_entropy_weight) == (0.8, 0.01)


def test_derive_args_refusals_and_acceptance():
    from vlp_amd import run_img2txt_dist as R

    def derive(extra):
        return R.derive_args(R.build_parser().parse_args(BASE + extra))
    with pytest.raises(ValueError, match="--scst_temperature.*needs --scst"):
        derive(["--scst_temperature", "0.8"])
    with pytest.raises(ValueError, match="--scst_entropy_weight.*needs --scst"):
        derive(["--scst_entropy_weight", "0.01"])
    for t in ("0", "-1", "inf", "nan"):
        with pytest.raises(ValueError, match="--scst_temperature"):
            derive(["--scst", "--scst_temperature", t])
    for w in ("-0.1", "inf", "nan"):
        with pytest.raises(ValueError, match="--scst_entropy_weight"):
            derive(["--scst", "--scst_entropy_weight", w])
    a = derive(["--scst", "--scst_temperature", "0.8", "--scst_entropy_weight", "0.01", "--scst_samples", "5", "--scst_reward", "device"])
    assert (a.scst_temperature, a.scst_entropy_weight, a.scst_samples, a.scst_reward) == (0.8, 0.01, 5, "device")
    derive([])                                        # the defaults need no --scst


def test_policy_structs_match_c_layout_and_are_registered(tmp_path):
    import ctypes
    from vlp_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    structs = {"vlp_token_policy_fwd_args": _lib.TokenPolicyFwdArgs, "vlp_token_policy_bwd_args": _lib.TokenPolicyBwdArgs}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "vlp_hip.h"',
             "int (*fwd)(const vlp_token_policy_fwd_args*, void*) = vlp_token_policy_fwd;",       # the declarations, as C
             "int (*bwd)(const vlp_token_policy_bwd_args*, void*) = vlp_token_policy_bwd;", "int main(void) {"]
    for cname, st in structs.items():
        lines.append('printf("%s %%zu", sizeof(%s));' % (cname, cname))
        for fname, _ in st._fields_:
            lines.append('printf(" %%zu", offsetof(%s, %s));' % (cname, fname))
        lines.append('printf("\\n");')
    lines.append("return 0; }")
    src = os.path.join(tmp_path, "layout.c")
    open(src, "w").write("\n".join(lines))
    obj = os.path.join(tmp_path, "decl.o")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(root, "include"), "-c", src, "-o", obj])
    # the layout program does not link the library: the two pointers are dropped for it
    open(src, "w").write("\n".join(l for l in lines if not l.startswith("int (*")))
    exe = os.path.join(tmp_path, "layout")
    subprocess.check_call(["gcc", "-I", os.path.join(root, "include"), src, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.strip().splitlines()
    assert len(out) == 2
    for line in out:
        parts = line.split()
        st = structs[parts[0]]
        print(line)
        assert int(parts[1]) == ctypes.sizeof(st), parts[0]
        assert [int(x) for x in parts[2:]] == [getattr(st, f).offset for f, _ in st._fields_], parts[0]
    for name in ("vlp_token_policy_fwd", "vlp_token_policy_bwd"):
        assert name in _lib.SYMBOLS
