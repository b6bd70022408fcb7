"""GPU: vlp_sample_rows_filtered (csrc/sampling.hip) -- temperature, top-k and top-p on the Gumbel-max sampler -- against the fp64 host
restatement of tests/sample_filter_util.py.  The padding columns V..ld hold +50 (or NaN, in the contract test): they do not exist.

The kept set is compared exactly (cutoff and |S| of every draw): the grid's rows keep top_p at least MARGIN_MIN = 1e-5 away from the
cumulative masses next to the threshold, a figure derived from the kernel's arithmetic in tests/sample_filter_util.py, where it is also said why
the 1e-3 first asked for is out of reach of N(0, 2^2) rows (63 of the 252 cases under it with the base rows, some at V = 28996 for every row).

The log-probability bound is the existing sampler's own error, doubled for the division by T: LOGP_ERR_REP is the largest |logp - fp64| of
vlp_sample_rows_rep over 256 draws of each of the grid's base rows (V = 257, 1000, 28996; test_logp_bound_is_the_existing_samplers_error
measures it again and prints it), LOGP_BOUND = 2 * LOGP_ERR_REP.  Measured on an MI355X: vlp_sample_rows_rep 3.36e-7 / 4.59e-7 / 3.23e-7 at the
three V, LOGP_ERR_REP = 4.59e-7, the bound therefore 9.18e-7; no figure of the new kernel went into either.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from tests import guard_util as G                           # noqa: E402
from tests import sample_filter_util as U                   # noqa: E402
from tests.step_seq_util import first_difference            # noqa: E402
from vlp_amd import _lib as K                               # noqa: E402

DEV = torch.device("cuda:0")
LOGP_ERR_REP = 4.59e-7
LOGP_BOUND = 2 * LOGP_ERR_REP
BASE11 = [2.0, 1.0, 0.0, -1.0, 0.5, 3.0, -2.0, 0.0, 1.5, -0.5, 2.5]       # the vector of test_sample_rows_distribution_and_logprob


def _cell(seed):
    return torch.tensor([seed], dtype=torch.long, device=DEV)


def padded(rows16, ld=None):
    """fp16 [R, V] (numpy or torch) -> device [R, ld] with the padding columns at +50."""
    t = torch.from_numpy(rows16) if isinstance(rows16, np.ndarray) else rows16
    R, V = t.shape
    ld = (V + 63) // 64 * 64 if ld is None else ld
    out = torch.full((R, ld), 50.0, dtype=torch.float16)
    out[:, :V] = t
    return out.to(DEV)


def draw(logits, V, n, rep=1, seed=1234, add=0, T=1.0, top_k=0, top_p=1.0):
    """-> dict(ids, ids2, logp, cutoff, kept) of n draws."""
    o = dict(ids=torch.full((n,), -7, dtype=torch.long, device=DEV), ids2=torch.full((n,), -7, dtype=torch.long, device=DEV),
             logp=torch.full((n,), 9.0, dtype=torch.float32, device=DEV), cutoff=torch.full((n,), 9.0, dtype=torch.float32, device=DEV),
             kept=torch.full((n,), -7, dtype=torch.int32, device=DEV))
    K.sample_rows_filtered(logits, logits.stride(0), n, V, rep, _cell(seed), add, 7001, T, top_k, top_p, o["ids"], o["logp"], ids2=o["ids2"],
                           cutoff=o["cutoff"], kept=o["kept"])
    return o


def rep_logp_error(V, rep=256):
    """Largest |logp - fp64 log-softmax| of the EXISTING sampler over `rep` draws of each of the grid's base rows at this V."""
    rows = U.random_rows(U.GRID_BASE_SEED + V, U.GRID_ROWS, V)
    n = U.GRID_ROWS * rep
    ids = torch.zeros(n, dtype=torch.long, device=DEV)
    lp = torch.zeros(n, dtype=torch.float32, device=DEV)
    logits = padded(rows)
    K.sample_rows_rep(logits, logits.stride(0), n, V, rep, _cell(77), 0, 7001, ids, lp)
    ref = np.stack([U.RowRef(x).filter()["logp"] for x in rows])
    ids, lp = ids.cpu().numpy(), lp.cpu().numpy().astype(np.float64)
    return float(np.abs(lp - ref[np.arange(n) // rep, ids]).max())


def test_logp_bound_is_the_existing_samplers_error():
    errs = {V: rep_logp_error(V) for V in U.GRID_V}
    print("vlp_sample_rows_rep against fp64, largest |logp error| per V: %s -> %.3e" % (errs, max(errs.values())))
    assert max(errs.values()) <= LOGP_ERR_REP, errs           # the figure in the docstring still describes the sampler


@pytest.mark.parametrize("rows,V,ld", [(5, 11, 64), (64, 1000, 1024), (8, 28996, 29056)])
def test_neutral_parameters_are_the_existing_sampler(rows, V, ld):
    g = torch.Generator().manual_seed(V)
    logits = padded((torch.randn(rows, V, generator=g) * 3).half(), ld)
    ids = torch.zeros(rows, dtype=torch.long, device=DEV)
    ids2 = torch.zeros(rows, dtype=torch.long, device=DEV)
    lp = torch.zeros(rows, dtype=torch.float32, device=DEV)
    K.sample_rows_rep(logits, ld, rows, V, 1, _cell(990), 3, 7001, ids, lp, ids2=ids2)
    o = draw(logits, V, rows, seed=990, add=3)
    assert torch.equal(o["ids"], ids) and torch.equal(o["ids2"], ids2)
    err = float((o["logp"] - lp).abs().max())
    print("neutral against vlp_sample_rows_rep: |logp difference| %.3e" % err)
    assert err <= 1e-5
    assert torch.equal(o["kept"], torch.full_like(o["kept"], V))
    assert torch.equal(o["cutoff"], logits[:, :V].float().min(dim=1)[0])


@pytest.mark.parametrize("T,top_p", [(1.0, 1.0), (0.5, 0.3), (2.0, 0.9)])
def test_top_k_1_on_a_unique_maximum_is_the_argmax(T, top_p):
    rows, V = 16, 1000
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(rows, V, generator=g) * 2).half()
    x[torch.arange(rows), torch.arange(rows) * 61 + 3] = 20.0
    o = draw(padded(x), V, rows, T=T, top_k=1, top_p=top_p)
    assert torch.equal(o["ids"].cpu(), torch.arange(rows) * 61 + 3) and torch.equal(o["ids2"], o["ids"])
    assert torch.equal(o["logp"], torch.zeros_like(o["logp"]))                 # exactly 0
    assert torch.equal(o["kept"], torch.ones_like(o["kept"])) and torch.equal(o["cutoff"], torch.full_like(o["cutoff"], 20.0))


def test_three_equal_maxima_are_all_kept_by_top_k_1():
    V, n = 300, 512
    g = torch.Generator().manual_seed(9)
    x = torch.randn(1, V, generator=g).clamp(-3, 3).half()
    cols = [17, 130, 299]
    x[0, cols] = 5.0
    o = draw(padded(x), V, n, rep=n, top_k=1)
    assert torch.equal(o["kept"], torch.full_like(o["kept"], 3)) and torch.equal(o["cutoff"], torch.full_like(o["cutoff"], 5.0))
    assert sorted(set(o["ids"].tolist())) == cols                              # only those three, and each of them
    err = float((o["logp"].double() + np.log(3.0)).abs().max())
    print("three maxima: |logp + log 3| %.3e" % err)
    assert err <= 1e-6


@pytest.mark.parametrize("V", U.GRID_V)
def test_threshold_grid(V):
    """T x top_k x top_p on random N(0, 2^2) rows: cutoff and |S| of every draw equal the host restatement, every id is in S, logp is the
    renormalised fp64 log-probability within LOGP_BOUND (8 draws of each of the 4 rows per case)."""
    rep = 8
    n = U.GRID_ROWS * rep
    row_of = np.arange(n) // rep
    worst, worst_case = 0.0, None
    for c in U.grid_cases(V):
        assert min(r["margin"] for r in c["refs"]) >= U.MARGIN_MIN
        o = draw(padded(c["rows"]), V, n, rep=rep, seed=4242, T=c["T"], top_k=c["top_k"], top_p=c["top_p"])
        tag = (V, c["T"], c["top_k"], c["top_p"])
        want_cut = np.array([c["refs"][r]["cutoff"] for r in row_of])
        want_kept = np.array([c["refs"][r]["kept"] for r in row_of])
        assert np.array_equal(o["cutoff"].cpu().numpy().astype(np.float64), want_cut), (tag, o["cutoff"][::rep].tolist(), want_cut[::rep])
        assert np.array_equal(o["kept"].cpu().numpy(), want_kept), (tag, o["kept"][::rep].tolist(), want_kept[::rep])
        ids = o["ids"].cpu().numpy()
        assert ids.min() >= 0 and ids.max() < V and torch.equal(o["ids"], o["ids2"]), tag
        assert all(c["refs"][r]["S"][i] for r, i in zip(row_of, ids)), tag
        ref = np.array([c["refs"][r]["logp"][i] for r, i in zip(row_of, ids)])
        err = float(np.abs(o["logp"].cpu().numpy().astype(np.float64) - ref).max())
        if err > worst:
            worst, worst_case = err, tag
    print("V=%d: largest |logp - fp64| %.3e at (V, T, top_k, top_p) = %s; bound %s" % (V, worst, worst_case, LOGP_BOUND))
    assert worst <= LOGP_BOUND, (worst, worst_case)


def test_distribution_of_the_filtered_draw():
    rows, V, T, top_k, top_p = 4096, 11, 0.7, 6, 0.9
    base = torch.tensor(BASE11).half()
    ref = U.filter_reference(base.numpy(), T, top_k, top_p)
    assert 1 < ref["kept"] < top_k and ref["margin"] >= 1e-3                    # both filters bite, far from a threshold
    o = draw(padded(base.unsqueeze(0).repeat(rows, 1)), V, rows, T=T, top_k=top_k, top_p=top_p)
    ids = o["ids"].cpu().numpy()
    assert ref["S"][ids].all()                                                  # no id outside S
    err = float(np.abs(o["logp"].cpu().numpy().astype(np.float64) - ref["logp"][ids]).max())
    print("distribution: kept %d, |logp - fp64| %.3e" % (ref["kept"], err))
    assert err <= LOGP_BOUND
    assert torch.equal(o["kept"], torch.full_like(o["kept"], ref["kept"])) and float(o["cutoff"][0]) == ref["cutoff"]
    freq = np.bincount(ids, minlength=V) / rows
    prob = ref["probs"]
    sigma = np.sqrt(prob * (1 - prob) / rows)
    assert float((np.abs(freq - prob)[ref["S"]] / sigma[ref["S"]]).max()) < 5.0, (freq, prob)      # every bin of S within 5 sigma


def test_minus_infinity_is_never_drawn():
    """All but two columns are -inf.  Every parameter set here has a filter that bites (top_k of 1 or 2, or top_p < 1): the kept set then
    holds at most the two finite columns.  (With nothing filtered S is every column by definition, kept = V, and still only the two are drawn.)"""
    V, n = 300, 64
    x = torch.full((1, V), float("-inf")).half()
    x[0, 41], x[0, 277] = 1.0, 0.0
    logits = padded(x)
    for T in (0.5, 1.0, 2.0):
        for top_k in (0, 1, 2, 5):
            for top_p in (1.0, 0.999, 0.9, 0.5):
                o = draw(logits, V, n, rep=n, T=T, top_k=top_k, top_p=top_p)
                assert set(o["ids"].tolist()) <= {41, 277}, (T, top_k, top_p)
                assert bool(torch.isfinite(o["logp"]).all()) and float(o["logp"].max()) <= 0.0
                if top_k in (1, 2) or top_p < 1.0:
                    ref = U.filter_reference(x[0].numpy(), T, top_k, top_p)
                    assert int(o["kept"].max()) <= 2 and torch.equal(o["kept"], torch.full_like(o["kept"], ref["kept"])), (T, top_k, top_p)
                else:
                    assert torch.equal(o["kept"], torch.full_like(o["kept"], V))


def test_rep_seed_and_repeat_launch():
    V, rep, R = 1000, 5, 3
    par = dict(T=0.8, top_k=20, top_p=0.9)
    g = torch.Generator().manual_seed(21)
    x = (torch.randn(R, V, generator=g) * 2).half()
    a = draw(padded(x), V, R * rep, rep=rep, **par)
    b = draw(padded(x.repeat_interleave(rep, dim=0)), V, R * rep, rep=1, **par)
    assert first_difference(a, b) is None, first_difference(a, b)               # draw r reads row r / rep under the row key r
    assert len(set(a["ids"][:rep].tolist())) > 1                                # the draws of one row differ
    a2 = draw(padded(x), V, R * rep, rep=rep, **par)
    assert first_difference(a, a2) is None, first_difference(a, a2)             # a repeated launch: the same bits in all outputs
    big = padded((torch.randn(8, 28996, generator=g) * 2).half())
    c, c2 = draw(big, 28996, 64, rep=8, T=1.3, top_k=0, top_p=0.7), draw(big, 28996, 64, rep=8, T=1.3, top_k=0, top_p=0.7)
    assert first_difference(c, c2) is None, first_difference(c, c2)
    flat = padded(torch.zeros(64, V).half())
    f0, f1 = draw(flat, V, 64, seed=50, add=1, T=1.3, top_k=100), draw(flat, V, 64, seed=50, add=2, T=1.3, top_k=100)
    f2 = draw(flat, V, 64, seed=51, add=1, T=1.3, top_k=100)
    assert not torch.equal(f0["ids"], f1["ids"]) and torch.equal(f1["ids"], f2["ids"])      # the seed is *seed_cell + seed_add
    assert torch.equal(f0["kept"], torch.full_like(f0["kept"], V))              # all columns tie at the threshold: all kept


@pytest.mark.parametrize("V,ld", [(1000, 1008), (1001, 1001), (11, 24)])
def test_contract_strides_guards_and_null_outputs(V, ld):
    """Strided outputs between guard bands, NaN in the padding columns and around the logits (16-byte aligned rows and, with ld = 1001,
    rows that are not), and the optional outputs left out."""
    rows, rep = 6, 2
    n = rows * rep
    g = torch.Generator().manual_seed(V)
    lg = G.guarded(rows, V, ld=ld, dtype=torch.float16, fill="nan", device=DEV)
    lg.set((torch.randn(rows, V, generator=g) * 2).half().to(DEV))
    ids = G.guarded(n, 3, dtype=torch.int64, fill="sentinel", device=DEV)
    ids2 = G.guarded(n, 2, dtype=torch.int64, fill="sentinel", device=DEV)
    lp = G.guarded(n, 2, dtype=torch.float32, fill="sentinel", device=DEV)
    cut = G.guarded_vec(n, dtype=torch.float32, fill="sentinel", device=DEV)
    kept = G.guarded_vec(n, dtype=torch.int32, fill="sentinel", device=DEV)
    par = (0.8, 20, 0.9) if V > 20 else (0.8, 5, 0.9)
    K.sample_rows_filtered(lg.full, ld, n, V, rep, _cell(31), 4, 7001, par[0], par[1], par[2], ids.view[:, 1], lp.view[:, 1], ids2=ids2.view[:, 0],
                           cutoff=cut.vec, kept=kept.vec)
    torch.cuda.synchronize()

    def col(width, c):
        m = torch.zeros(n, width, dtype=torch.bool, device=DEV)
        m[:, c] = True
        return m
    G.assert_untouched(lg, None, "logits")
    for gd, w, name in ((ids, col(3, 1), "ids"), (ids2, col(2, 0), "ids2"), (lp, col(2, 1), "logp"), (cut, "logical", "cutoff"), (kept, "logical", "kept")):
        G.assert_untouched(gd, w, name)
        G.assert_written(gd, w, name)
    G.assert_finite(lp.view[:, 1], "logp")
    G.assert_finite(cut.vec, "cutoff")
    x = lg.view.cpu().numpy()
    for r in range(n):
        ref = U.filter_reference(x[r // rep], *par)
        assert ref["S"][int(ids.view[r, 1])] and int(ids2.view[r, 0]) == int(ids.view[r, 1])
        if ref["margin"] >= U.MARGIN_MIN:
            assert int(kept.vec[r]) == ref["kept"] and float(cut.vec[r]) == ref["cutoff"]
    o = dict(ids=torch.zeros(n, dtype=torch.long, device=DEV), logp=torch.zeros(n, dtype=torch.float32, device=DEV))
    K.sample_rows_filtered(lg.full, ld, n, V, rep, _cell(31), 4, 7001, par[0], par[1], par[2], o["ids"], o["logp"])      # no ids2, cutoff, kept
    assert torch.equal(o["ids"], ids.view[:, 1]) and first_difference({"logp": o["logp"]}, {"logp": lp.view[:, 1].contiguous()}) is None


@pytest.mark.parametrize("bad", [dict(T=0.0), dict(T=-1.0), dict(T=float("inf")), dict(T=float("nan")), dict(top_k=-1), dict(top_p=0.0),
                                 dict(top_p=1.5), dict(top_p=float("nan")), dict(top_p=-0.5), dict(rep=0), dict(rep=-2)])
def test_bad_arguments_are_refused_before_anything_is_launched(bad):
    V, n = 100, 4
    logits = padded(torch.zeros(n, V).half())
    with pytest.raises(RuntimeError, match="vlp_sample_rows_filtered"):
        draw(logits, V, n, **bad)
    o = dict(ids=torch.full((n,), -7, dtype=torch.long, device=DEV), logp=torch.full((n,), 9.0, dtype=torch.float32, device=DEV),
             cutoff=torch.full((n,), 9.0, dtype=torch.float32, device=DEV), kept=torch.full((n,), -7, dtype=torch.int32, device=DEV))
    kw = dict(dict(T=1.0, top_k=0, top_p=1.0, rep=1), **bad)
    with pytest.raises(RuntimeError, match="vlp_sample_rows_filtered"):
        K.sample_rows_filtered(logits, logits.stride(0), n, V, kw["rep"], _cell(1), 0, 7001, kw["T"], kw["top_k"], kw["top_p"], o["ids"], o["logp"],
                               ids2=None, cutoff=o["cutoff"], kept=o["kept"])
    torch.cuda.synchronize()
    assert bool((o["ids"] == -7).all()) and bool((o["logp"] == 9.0).all()) and bool((o["cutoff"] == 9.0).all()) and bool((o["kept"] == -7).all())
