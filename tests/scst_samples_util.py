"""Shared by tests/test_scst_samples_cpu.py and tests/test_83_scst_samples_gpu.py (no test in here): the leave-one-out reward restated from
scores, the shapes and seeds of the kernel comparison, and the error bounds."""
import numpy as np

from tests import scst_df_util as U

# (G, R, T, mult) -> corpus seed (scst_df_util.make_corpus).  Chosen on the HOST scorer alone: with these every score is non-zero and every
# leave-one-out reward is non-zero, with df='corpus' and with table(T, 0); the tests assert both again before they look at a kernel's output.
SHAPES = [((3, 1, 5, 4), 0), ((5, 3, 21, 5), 2), ((4, 2, 3, 16), 1), ((65, 2, 64, 3), 1), ((64, 5, 21, 5), 0), ((16, 5, 21, 16), 0)]
# rewards only (a score may be zero): ((G, R, T, mult), seed, modes)
EXTRA = [((2, 8, 1, 16), 2, ("batch", "table")), ((1, 1, 4, 3), 1, ("table",))]

score_bound = U.bound


def reward_bound(T, mult):
    """Two score errors (the sample's, and the mean of the others' is at most one more) plus the fp32 rounding of at most mult + 1 operations
    (mult - 2 additions, a divide, a subtract, and slack) on values of at most 10."""
    return 2 * U.bound(T) + (mult + 1) * 2.0 ** -24 * 10


def loo(scores, mult):
    """reward[k*G + g] = s[k*G + g] - (sum of s[j*G + g], j != k, ascending j) / (mult - 1), in the dtype of `scores`."""
    s = np.asarray(scores).reshape(mult, -1)
    out = np.empty_like(s)
    for k in range(mult):
        acc = np.zeros(s.shape[1], dtype=s.dtype)
        for j in range(mult):
            if j != k:
                acc = acc + s[j]
        out[k] = s[k] - acc / s.dtype.type(mult - 1)
    return out.reshape(-1)
