"""Host restatement, in fp64 on fp16 inputs, of the temperature / top-k / top-p sampling rule of vlp_sample_rows_filtered (DESIGN.md
section 6, include/vlp_hip.h), and the case generator of the threshold-grid tests.  Only numpy is imported: the CPU tests of
tests/test_sample_filter_cpu.py run without a GPU.

    z_v = l_v / T
    top-k (0 < top_k < V): S_k = {v : l_v >= tau_k}, tau_k the top_k-th largest logit with multiplicity (ties kept); else every column
    top-p (top_p < 1):     q = softmax(z) over S_k; tau_p = the largest value t with sum_{v in S_k, l_v >= t} q_v >= top_p; S = S_k and l >= tau_p
    logp(v) = z_v - logsumexp_{u in S} z_u

T and top_p are taken at the float32 value the C entry receives.
"""
import numpy as np

# A grid case is used when top_p is at least MARGIN_MIN away (relatively) from the two cumulative masses next to the chosen threshold, so that
# the kernel's fp32 masses must choose the fp64 threshold.  1e-3 was the figure first asked for; N(0, 2^2) rows cannot meet it: at V = 28996,
# T = 2, top_p = 0.9 one distinct fp16 value carries about 5e-5 of top_p, so NO row has a margin above 2.5e-5, and with the base seed below
# 63 of the 252 cases (25 %) fall under 1e-3 (17 / 84 at V = 257, 18 / 84 at V = 1000, 28 / 84 at V = 28996; tests/test_sample_filter_cpu.py
# prints the counts).  The bound used is the kernel's own arithmetic instead, which asks exactness of MORE rows, the 1e-3 ones included:
# a column's mass is exp2(fl(fl(l / T) - z_max) * log2 e) in fp32, in units of 2^-40 (exact above 2^-16 of the maximum's mass).  With
# |z| <= 20 (|l| <= 10, T >= 0.5) and d = z_max - z <= 15 for every column that matters (the columns beyond hold < 29000 e^-15 = 9e-3 of the
# maximum's mass): fl(l / T) <= 2^-24 * 20 = 1.2e-6, the subtraction, the product with log2 e and log2 e's own rounding <= 2^-24 * 15 = 0.9e-6
# each, v_exp_f32 1.2e-7: <= 4e-6 relative per column, <= 8e-6 on a ratio of two sums, plus 29000 * 2^-40.  MARGIN_MIN = 1e-5.
MARGIN_MIN = 1e-5
MARGIN_ASKED = 1e-3
GRID_T = (0.5, 1.0, 2.0)
GRID_TOP_P = (1.0, 0.9, 0.5, 0.05)
GRID_V = (257, 1000, 28996)
GRID_ROWS = 4
GRID_BASE_SEED = 20240


def grid_top_k(V):
    return (0, 1, 7, 50, V - 1, V, V + 5)


class RowRef(object):
    """One fp16 logits row: its distinct values in descending order with their multiplicities (all a threshold can depend on)."""

    def __init__(self, row16):
        row16 = np.asarray(row16)
        assert row16.dtype == np.float16 and row16.ndim == 1 and not np.isnan(row16).any()
        self.l = row16.astype(np.float64)
        vals, counts = np.unique(self.l, return_counts=True)              # ascending; -0 and +0 are one value
        self.vals, self.counts = vals[::-1].copy(), counts[::-1].copy()
        self.V = row16.shape[0]

    def filter(self, T=1.0, top_k=0, top_p=1.0):
        """-> dict(S bool [V], cutoff, kept, logp fp64 [V] (-inf outside S), probs fp64 [V], margin)."""
        T, top_p, top_k = float(np.float32(T)), float(np.float32(top_p)), int(top_k)
        assert T > 0 and top_k >= 0 and 0 < top_p <= 1
        vals, counts = self.vals, self.counts
        n = len(vals)                                    # vals[:n] are the values still kept
        if 0 < top_k < self.V:
            n = int(np.searchsorted(np.cumsum(counts), top_k, side="left")) + 1
        z = vals / T
        margin = float("inf")
        if top_p < 1.0:
            with np.errstate(invalid="ignore"):
                w = counts[:n] * np.exp(z[:n] - z[0])
            w[np.isnan(w)] = 0.0
            cum = np.cumsum(w) / w.sum()
            i = int(np.argmax(cum >= top_p))             # the first (largest-valued) threshold whose mass reaches top_p
            if not cum[i] >= top_p:                      # rounding of the last quotient below 1 >= top_p
                i = n - 1
            n = i + 1
            below = cum[i - 1] if i > 0 else 0.0
            margin = min(abs(cum[i] - top_p), abs(top_p - below)) / top_p
        cutoff = vals[n - 1]
        S = self.l >= cutoff
        zz = self.l / T
        with np.errstate(divide="ignore", invalid="ignore"):
            e = np.where(S, np.exp(zz - z[0]), 0.0)
            e[np.isnan(e)] = 0.0
            logp = np.where(S, zz - z[0] - np.log(e.sum()), -np.inf)
        return {"S": S, "cutoff": float(cutoff), "kept": int(S.sum()), "logp": logp, "probs": e / e.sum(), "margin": margin}


def filter_reference(row16, T=1.0, top_k=0, top_p=1.0):
    return RowRef(row16).filter(T, top_k, top_p)


def brute_force_set(row16, T, top_k, top_p):
    """The kept set by sorting, straight from the definition (small rows): bool [V]."""
    l = np.asarray(row16).astype(np.float64)
    T, top_p = float(np.float32(T)), float(np.float32(top_p))
    V = l.shape[0]
    order = sorted(range(V), key=lambda v: -l[v])
    keep = list(order)
    if 0 < top_k < V:
        tau = l[order[top_k - 1]]
        keep = [v for v in order if l[v] >= tau]
    if top_p < 1.0:
        zmax = l[order[0]] / T
        q = np.array([0.0 if l[v] == -np.inf else np.exp(l[v] / T - zmax) for v in keep])
        q = q / q.sum()
        acc, j = 0.0, 0
        while j < len(keep):                             # take whole groups of equal logits until the mass reaches top_p
            tau = l[keep[j]]
            while j < len(keep) and l[keep[j]] == tau:
                acc += q[j]
                j += 1
            if acc >= top_p:
                break
        keep = keep[:j]
    S = np.zeros(V, dtype=bool)
    S[keep] = True
    return S


def random_rows(seed, rows, V):
    """N(0, 2^2) rounded to fp16."""
    return (np.random.RandomState(seed).standard_normal((rows, V)) * 2.0).astype(np.float16)


def grid_cases(V):
    """The threshold grid at one V: a list of dict(T, top_k, top_p, rows fp16 [GRID_ROWS, V], refs [GRID_ROWS], regenerated).  Every case starts
    from the rows of GRID_BASE_SEED + V; a case whose smallest margin is below MARGIN_MIN takes the rows of the next seed instead (and the
    next, until the margin holds) and is counted as regenerated."""
    base = {}

    def rows_of(seed):
        if seed not in base:
            r = random_rows(seed, GRID_ROWS, V)
            base[seed] = (r, [RowRef(x) for x in r])
        return base[seed]

    cases = []
    for T in GRID_T:
        for top_k in grid_top_k(V):
            for top_p in GRID_TOP_P:
                seed = GRID_BASE_SEED + V
                while True:
                    rows, rr = rows_of(seed)
                    refs = [x.filter(T, top_k, top_p) for x in rr]
                    if min(r["margin"] for r in refs) >= MARGIN_MIN:
                        break
                    seed += 1
                    if seed - (GRID_BASE_SEED + V) > 50:
                        raise AssertionError("no rows with a margin of %g for V=%d T=%g top_k=%d top_p=%g in 50 seeds" % (MARGIN_MIN, V, T, top_k, top_p))
                cases.append({"T": T, "top_k": top_k, "top_p": top_p, "rows": rows, "refs": refs, "regenerated": seed != GRID_BASE_SEED + V})
    return cases
