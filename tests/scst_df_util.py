"""Shared by tests/test_scst_df_cpu.py and tests/test_82_scst_df_gpu.py (no test in here): the seeded corpus of test_81, document-frequency
tables counted by brute force, and a restatement of CIDEr-D with a table that shares no code with vlp_amd.scst.CiderD -- it works on id rows,
packs its own keys and runs in the float type it is given (float64: the independent check of the host class; float32: what fp32 arithmetic
alone costs, the yardstick for the kernel's bound)."""
from collections import Counter, OrderedDict

import numpy as np

from vlp_amd import scst as SC

SEP = 102
# (G, R, T, mult) of the kernel comparison, and the seeds of the corpus and of the two tables.  Seeds are chosen on the HOST scorer alone:
# corpus seed = the first of 0, 1, 2, ... whose scores are all non-zero and whose hypothesis n-grams miss the table in 5 % .. 50 % of the
# cases (T >= 3; shorter strings never miss a 200-image table over 12 words); the conditions are asserted again by the tests.
SHAPES = [(1, 1, 4, 2), (3, 1, 5, 2), (5, 3, 21, 2), (65, 2, 64, 2), (2, 8, 1, 2), (4, 2, 3, 2), (64, 5, 21, 2)]
TABLE_SEEDS = (99, 98)
SCALE = 16000                   # the second table: every df and n_docs x 16 000 -> n_docs 3.2 M, df far beyond 11 or 16 bits


def bound(T):
    return (4 * T + 16) * 2.0 ** -24 * 10


def make_corpus(G, R, T, mult, seed):
    """test_81's generator: 12-word vocabulary 1000..1011; reference lengths uniform in 1..T, [SEP] as the last kept token of a reference
    shorter than T, then zeros; ref_count uniform in 1..R; a hypothesis is a copy of one valid reference of its group with 30 % of its
    non-zero ids redrawn."""
    rng = np.random.RandomState(seed)
    ref = np.zeros((G, R, T), dtype=np.int64)
    count = rng.randint(1, R + 1, size=G).astype(np.int32)
    for g in range(G):
        for r in range(R):
            n = rng.randint(1, T + 1)
            ref[g, r, :n] = rng.randint(1000, 1012, size=n)
            if n < T:
                ref[g, r, n - 1] = SEP
    hyp = np.zeros((mult * G, T), dtype=np.int64)
    for i in range(mult * G):
        g = i % G
        row = ref[g, rng.randint(count[g])].copy()
        redraw = (rng.rand(T) < 0.3) & (row != 0)
        row[redraw] = rng.randint(1000, 1012, size=int(redraw.sum()))
        hyp[i] = row
    return hyp, ref, count


def row_tokens(row):
    """The ids of a row up to and including the first 0."""
    out = []
    for t in row:
        out.append(int(t))
        if t == 0:
            break
    return out


def key_of(gram):
    """The table key of a tuple of ids, None when an id has no key (outside 0..65534)."""
    key = 0
    for j, t in enumerate(gram):
        if not 0 <= t < 65535:
            return None
        key |= (t + 1) << (48 - 16 * j)
    return key


def grams_of(tokens):
    c = Counter()
    for k in range(1, 5):
        for i in range(len(tokens) - k + 1):
            c[tuple(tokens[i:i + k])] += 1
    return c


def table_of_sets(ref, count, scale=1):
    """DocFreq counted by brute force: one document per group = its valid reference rows.  scale multiplies every df and n_docs."""
    df = Counter()
    for g in range(ref.shape[0]):
        seen = set()
        for r in range(int(count[g])):
            seen.update(grams_of(row_tokens(ref[g, r])))
        for gram in seen:
            df[key_of(gram)] += 1
    keys = np.array(sorted(df), dtype=np.uint64)
    vals = np.array([df[int(k)] * scale for k in keys], dtype=np.int32)
    return SC.DocFreq(keys, vals, ref.shape[0] * scale)


_TABLES = {}


def table(T, which):
    """which 0: the 200-image table of seed TABLE_SEEDS[0] as it is; 1: the one of TABLE_SEEDS[1] with df and n_docs x SCALE.  Strings as
    long as the case's (T), five references per image."""
    if (T, which) not in _TABLES:
        _, ref, count = make_corpus(200, 5, T, 1, TABLE_SEEDS[which])
        _TABLES[(T, which)] = table_of_sets(ref, count, SCALE if which else 1)
    return _TABLES[(T, which)]


def host_scores(hyp, ref, count, mult, df="corpus"):
    """CiderD.compute_score on the strings array_to_str makes: hypothesis i against the first count[g] references of group g = i % G."""
    G = ref.shape[0]
    gts, res = OrderedDict(), OrderedDict()
    for i in range(mult * G):
        g = i % G
        res[i] = [SC.array_to_str(hyp[i].tolist())]
        gts[i] = [SC.array_to_str(r) for r in ref[g, :count[g]].tolist()]
    return SC.CiderD(df=df).compute_score(gts, res)[1]


def restated_scores(hyp, ref, count, mult, tab, dtype=np.float64, sigma=6.0):
    """CIDEr-D with the table's document frequencies, restated on id rows in `dtype` arithmetic.  Returns (scores [mult*G] float64, the share
    of hypothesis n-gram occurrences the table does not hold)."""
    f = dtype
    lookup = dict(zip((int(k) for k in tab.keys), (int(v) for v in tab.vals)))
    ref_len = np.log(f(tab.n_docs))
    miss = [0, 0]

    def vec(row, tally=False):
        toks = row_tokens(row)
        w = [dict() for _ in range(4)]
        for gram, tf in grams_of(toks).items():
            df = lookup.get(key_of(gram), 0)
            if tally:
                miss[0] += tf * (df == 0)
                miss[1] += tf
            w[len(gram) - 1][gram] = f(tf) * (ref_len - np.log(f(max(1, df))))
        norm = []
        for k in range(4):
            n2 = f(0)
            for v in w[k].values():
                n2 = f(n2 + v * v)
            norm.append(np.sqrt(n2))
        return w, norm, max(len(toks) - 1, 0)

    G = ref.shape[0]
    rvec = [[vec(ref[g, r]) for r in range(int(count[g]))] for g in range(G)]
    out = []
    for i in range(mult * G):
        hw, hn, hl = vec(hyp[i], tally=True)
        acc = [f(0)] * 4
        for rw, rn, rl in rvec[i % G]:
            pen = np.exp(f(-(f(hl - rl) ** 2)) / f(2 * sigma * sigma))
            for k in range(4):
                v = f(0)
                for gram, a in hw[k].items():
                    b = rw[k].get(gram, f(0))
                    v = f(v + min(a, b) * b)
                if hn[k] != 0 and rn[k] != 0:
                    v = f(v / f(hn[k] * rn[k]))
                acc[k] = f(acc[k] + v * pen)
        out.append(float(f(f(f(f(acc[0] + acc[1]) + acc[2]) + acc[3]) / f(4) / f(len(rvec[i % G])) * f(10))))
    return np.array(out), miss[0] / max(miss[1], 1)


def table_from_dict(df, n_docs):
    """DocFreq of {tuple of ids: df}."""
    by_key = {key_of(g): v for g, v in df.items()}
    assert len(by_key) == len(df) and None not in by_key
    keys = np.array(sorted(by_key), dtype=np.uint64)
    return SC.DocFreq(keys, np.array([by_key[int(k)] for k in keys], dtype=np.int32), n_docs)


def hard_case(garbage=True):
    """G = 6, R = 3, T = 8, mult = 2 and its table (n_docs 6; the groups of the garbage-free case as documents, then edited by hand).
      group 0   first tokens 32766 / 32767: keys just below and just above 2^63.  hyp[0] equals its one reference; hyp[G+0] is made of
                words no document holds: every n-gram misses
      group 1   first token 65534: the largest keys; the 4-gram (65534, 65534, 1004, 1009) is df_keys[N-1]
      group 2   ids 65535 and 70000 in a hypothesis and in a reference: n-grams that hold them have no key.  Formed carelessly,
                (1006, 65535) is the key of (1007,) and 70000 that of 4464: (1007,) and the decoy (1009, 4464) are in the table.
                hyp[G+2] is 1009 eight times; every run of 1009 has df == n_docs: zero weights, zero norm, undivided sum
      the unigram (0,) is df_keys[0].
    garbage=False: the same case with everything behind a row's first 0, and every invalid reference row, zeroed."""
    G, R, T = 6, 3, 8
    _, ref, count = make_corpus(G, R, T, 2, 5)
    hyp = np.zeros((2 * G, T), dtype=np.int64)
    count[:] = [1, 2, 2, 3, 1, 2]
    ref[0, 0] = [32766, 1001, 32767, 1009, SEP, 0, 0, 0]
    ref[1, 0] = [65534, 65534, 1004, 1009, SEP, 0, 0, 0]
    ref[1, 1] = [1005, 1001, 1001, 1001, 1001, SEP, 0, 0]
    ref[2, 0] = [1006, 65535, 1008, 1009, 70000, 1011, 1006, 1007]            # no 0 at all
    ref[2, 1] = [1011, 1010, 1009, 1008, 1007, 1006, 1011, 1010]
    for g in (3, 4, 5):
        ref[g, 0, 0] = 1009
    hyp[0] = ref[0, 0]
    hyp[G + 0] = [2000, 2001, 2000, 2001, 2002, 2003, 2000, 2001]
    hyp[1] = [65534, 65534, 65534, 1004, 1009, SEP, 0, 0]
    hyp[G + 1] = [65534, 65534, 1004, 1009, 1001, SEP, 0, 0]
    hyp[2] = [1006, 65535, 1008, 1009, 70000, 1011, 1006, 1003]
    hyp[G + 2] = [1009] * 8
    for g in (3, 4, 5):
        hyp[g] = ref[g, 0]
        hyp[G + g] = ref[g, count[g] - 1]
        hyp[G + g, 1] = 1003
    if not garbage:
        for rows in (hyp, ref.reshape(G * R, T)):
            for row in rows:
                z = np.flatnonzero(row == 0)
                if len(z):
                    row[z[0]:] = 0
        for g in range(G):
            ref[g, count[g]:] = 0
    else:
        for row in (hyp[0], hyp[1], hyp[G + 1], ref[0, 0], ref[1, 0], ref[1, 1]):
            z = int(np.flatnonzero(row == 0)[0])
            row[z + 1:] = ([1001, 1009, 1000, 1004, SEP, 1002, 1005] * 2)[:T - z - 1]
        for g in range(G):
            for r in range(count[g], R):
                ref[g, r] = hyp[g if r % 2 else G + g]
    return hyp, ref, count


def hard_table():
    _, ref, count = hard_case(False)
    df = Counter()
    for g in range(ref.shape[0]):
        seen = set()
        for r in range(int(count[g])):
            seen.update(grams_of(row_tokens(ref[g, r])))
        df.update(g_ for g_ in seen if key_of(g_) is not None)
    for k in range(1, 5):
        df[(1009,) * k] = 6
    df[(1009, 4464)] = 3
    assert df[(1007,)] >= 1 and df[(0,)] >= 1
    return table_from_dict(df, 6)
