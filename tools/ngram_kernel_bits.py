"""SHA-256 of every output of the n-gram scoring entries (csrc/reward.hip, csrc/caption_eval.hip, the pieces of csrc/reward_common.h): cider_d,
cider_d_multi, cider_d_df, cider_d_multi_df, cider_d_consensus (with and without pair), bleu4 (plain, mixed with and without base, pair and
leave-one-out reward, stats) and caption_eval (cider, bleu_stats, lcs), over a fixed list of seeded cases: run under two builds of the library
(VLP_HIP_LIB=...) and diff the output to show that a rewrite of these kernels leaves every bit where it was.  Every output starts from a
sentinel and is hashed whole.  The corpora are the tests' own (tests/scst_df_util.py, scst_bleu_util.py, caption_eval_util.py); that their
scores are not trivially zero is asserted on the host scorers before anything is hashed.  --time prints microseconds per launch sequence at
the shapes tools/scst_bench.py, consensus_bench.py and caption_eval_bench.py use instead (device events, a warm-up, rotating operand sets, the
median of three windows).
usage: python tools/ngram_kernel_bits.py [--time]"""
import hashlib, os, sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vlp_amd import _lib as K
from vlp_amd import scst as SC
from tests import scst_df_util as U
from tests import scst_bleu_util as BU
from tests import caption_eval_util as CU
DEV = torch.device("cuda:0")
F32, I32 = torch.float32, torch.int32
# (G, R, T): n-grams longer than the string (T 1, 2, 3), P > T (5, 21), rows without a 0 (64), R 1 and 8, G 1, three tiles with a ragged last
# one in the counting pass ((33, 8, 64): tile_groups 15)
SHAPES = [(1, 1, 1), (2, 8, 2), (4, 2, 3), (3, 1, 5), (5, 3, 21), (3, 8, 64), (33, 8, 64)]
MULTS = (1, 2, 3, 16)
KS = (2, 5, 16)
EMPTY = SC.DocFreq(np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.int32), 1)
JUNK = np.array([1001, 1009, 1000, 1004, 102, 1002, 1005] * 12)


def sha(*ts):
    h = hashlib.sha256()
    for t in ts:
        h.update(t.detach().contiguous().cpu().numpy().tobytes())
    return h.hexdigest()[:16]


def out(shape, dtype=F32):
    """An output that starts from a sentinel: an element a kernel stops writing shows in the hash."""
    return torch.full(shape if isinstance(shape, tuple) else (shape,), -7 if dtype == I32 else -7.25, dtype=dtype, device=DEV)


def dev(hyp, ref, count, strided=False):
    """The three operands on the device.  strided: rows of ld = T + 5 inside a junk-filled buffer, reference groups 2 rows apart more than R."""
    c = None if count is None else torch.from_numpy(np.ascontiguousarray(count)).to(DEV)
    if not strided:
        return torch.from_numpy(hyp).to(DEV), torch.from_numpy(ref).to(DEV), c
    G, R, T = ref.shape
    hb = torch.from_numpy(np.resize(JUNK, (hyp.shape[0], T + 5))).to(DEV)
    rb = torch.from_numpy(np.resize(JUNK, (G, R + 2, T + 5))).to(DEV)
    hb[:, :T] = torch.from_numpy(hyp).to(DEV)
    rb[:, :R, :T] = torch.from_numpy(ref).to(DEV)
    return hb[:, :T], rb[:, :R, :T], c


def with_garbage(rows):
    """A copy with junk words behind every row's first 0 (no entry reads there)."""
    rows = rows.copy()
    for row in rows.reshape(-1, rows.shape[-1]):
        z = np.flatnonzero(row == 0)
        if len(z):
            row[z[0] + 1:] = JUNK[:len(row) - int(z[0]) - 1]
    return rows


def reward_corpus(shape, mult, maker=U.make_corpus):
    """The first seeded corpus whose host CIDEr-D scores against the 200-image table are not all zero; at T = 64 group 0 gets a reference and a
    hypothesis without a 0, and hypothesis 1 an id that has no key."""
    G, R, T = shape
    for seed in range(16):
        hyp, ref, count = maker(G, R, T, mult, seed)
        if T == 64:
            ref[0, 0] = 1000 + (np.arange(T) * 7) % 12
            hyp[0] = ref[0, 0]
            hyp[0, 5] = 1003
            hyp[min(1, len(hyp) - 1), 0] = 70000
        if float(np.max(U.host_scores(hyp, ref, count, mult, df=U.table(T, 0)))) > 0:
            return hyp, ref, count
    raise AssertionError("no seed below 16 gives a non-zero host score for %r x %d" % (shape, mult))


def cider_cases(tag, hyp, ref, count, mult, tabs, strided=False):
    h, r, c = dev(hyp, ref, count, strided)
    n, G = hyp.shape[0], ref.shape[0]
    for name, tab in [("corpus", None)] + tabs:
        scores = out(n)
        reward = out(n if mult > 2 else G) if mult >= 2 else None
        table = () if tab is None else tab.to(DEV) + (tab.n_docs,)
        fn = {(False, False): K.cider_d, (True, False): K.cider_d_multi, (False, True): K.cider_d_df, (True, True): K.cider_d_multi_df}[(mult > 2, tab is not None)]
        fn(h, r, c, mult, scores, *table, reward=reward)
        print("%-18s %s df=%-8s scores %s  reward %s" % (fn.__name__, tag, name, sha(scores), sha(reward) if mult >= 2 else "-"))
        if mult == 2:                                    # the multi entries at mult 2: the leave-one-out reward of a pair
            fn2 = K.cider_d_multi if tab is None else K.cider_d_multi_df
            scores, reward = out(n), out(n)
            fn2(h, r, c, mult, scores, *table, reward=reward)
            print("%-18s %s df=%-8s scores %s  reward %s" % (fn2.__name__, tag, name, sha(scores), sha(reward)))


def bleu_cases(tag, hyp, ref, count, mult, strided=False):
    h, r, c = dev(hyp, ref, count, strided)
    n, G = hyp.shape[0], ref.shape[0]
    base = torch.from_numpy(np.random.RandomState(n).rand(n).astype(np.float32) * 10).to(DEV)
    variants = [("plain", {}), ("stats", dict(stats=True)), ("mixed+base", dict(base=True, mixed=True)), ("mixed", dict(mixed=True))]
    if mult == 2:
        variants.append(("pair", dict(base=True, mixed=True, reward=G)))
    if mult >= 2:
        variants.append(("loo", dict(base=True, mixed=True, reward=n, loo=True)))
    hs = []
    for name, v in variants:
        b, stats = out(n), out((n, 6), I32) if v.get("stats") else None
        mixed, reward = out(n) if v.get("mixed") else None, out(v["reward"]) if v.get("reward") else None
        K.bleu4(h, r, c, mult, b, stats=stats, base=base if v.get("base") else None, w_base=0.75, w_bleu=2.5, mixed=mixed, reward=reward,
                loo=bool(v.get("loo")))
        hs.append("%s %s" % (name, sha(*[t for t in (b, stats, mixed, reward) if t is not None])))
    print("%-18s %s %s" % ("bleu4", tag, "  ".join(hs)))


def consensus_cases(tag, ids, Kn, tabs):
    h = torch.from_numpy(ids).to(DEV)
    G = ids.shape[0] // Kn
    for name, tab in tabs:
        keys, vals = tab.to(DEV)
        hs = []
        for want_pair in (True, False):
            utility, pick, pair = out(Kn * G), out(G, I32), out((G, Kn, Kn)) if want_pair else None
            K.cider_d_consensus(h, Kn, keys, vals, tab.n_docs, utility, pick, pair=pair)
            hs.append("%s %s" % ("pair" if want_pair else "no pair", sha(*[t for t in (utility, pick, pair) if t is not None])))
        print("%-18s %s df=%-8s %s" % ("cider_d_consensus", tag, name, "  ".join(hs)))


def caption_cases(tag, hyp, ref, count, tabs, strided=False):
    h, r, c = dev(hyp, ref, count, strided)
    G, R, _ = ref.shape
    for name, tab in tabs:
        keys, vals = tab.to(DEV)
        cider, stats, lcs = out(G), out((G, 6), I32), out((G, R, 2), I32)
        K.caption_eval(h, r, c, cider, stats, lcs, keys, vals, tab.n_docs)
        print("%-18s %s df=%-8s cider %s  bleu_stats %s  lcs %s" % ("caption_eval", tag, name, sha(cider), sha(stats), sha(lcs)))


def bits():
    for shape in SHAPES:
        G, R, T = shape
        tabs = [("n200", U.table(T, 0)), ("n3200000", U.table(T, 1)), ("empty", EMPTY)]
        for mult in MULTS:
            if G * mult > 160:                           # (33, 8, 64) at mult 16 adds no path
                continue
            tag = "G=%-2d R=%d T=%-2d mult=%-2d" % (G, R, T, mult)
            hyp, ref, count = reward_corpus(shape, mult)
            cider_cases(tag, hyp, ref, count, mult, tabs)
            cider_cases(tag + " count=None", hyp, ref, None, mult, tabs[:1])
            bshape = (G, R, T, mult)
            bh, br, bc = BU.make_corpus(*bshape, BU.seed_of(bshape))
            assert BU.conditions(bshape, BU.host_bleu(bh, br, bc, mult)[0])
            bleu_cases(tag, bh, br, bc, mult)
            bleu_cases(tag + " count=None", bh, br, None, mult)
            if T in (5, 64):
                cider_cases(tag + " strided", with_garbage(hyp), with_garbage(ref), count, mult, tabs[:1], strided=True)
                bleu_cases(tag + " strided", with_garbage(bh), with_garbage(br), bc, mult, strided=True)
        for Kn in KS:
            if G * Kn > 160:
                continue
            ids = reward_corpus((G, 1, T), Kn)[0]        # the K samples of an image: K edited copies of one caption
            consensus_cases("G=%-2d K=%-2d T=%-2d" % (G, Kn, T), ids, Kn, tabs)
        seed = CU.seed_of(shape)
        ch, cr, cc = CU.make_corpus(G, R, T, seed)
        stats, lcs, _ = CU.host_counts(ch, cr, cc, cache_key=(shape, seed))
        assert CU.conditions(shape, stats, lcs, cc)
        ctabs = [("n200", CU.table(T)), ("empty", EMPTY)]
        tag = "G=%-2d R=%d T=%-2d" % shape
        caption_cases(tag, ch, cr, cc, ctabs)
        caption_cases(tag + " count=None", ch, cr, None, ctabs[:1])
        if T in (5, 64):
            caption_cases(tag + " strided", with_garbage(ch), with_garbage(cr), cc, ctabs[:1], strided=True)
    # the hand-built hard rows of the three makers
    hyp, ref, count = U.hard_case()
    assert float(np.max(U.host_scores(hyp, ref, count, 2, df=U.hard_table()))) > 0
    cider_cases("df hard", hyp, ref, count, 2, [("hard", U.hard_table())])
    consensus_cases("df hard K=2", hyp, 2, [("hard", U.hard_table())])
    hyp, ref, count = BU.hard_case()
    assert int(BU.host_bleu(hyp, ref, count, 2)[0][:, 0].max()) > 0
    bleu_cases("bleu hard", hyp, ref, count, 2)
    cider_cases("bleu hard", hyp, ref, count, 2, [("n200", U.table(8, 0))])
    hyp, ref, count = CU.hard_case()
    assert int(CU.host_counts(hyp, ref, count)[1][..., 0].max()) > 0
    caption_cases("caption hard", hyp, ref, count, [("n200", CU.table(64))])
    torch.cuda.synchronize()


def timed(fn, iters=200, nset=4):
    for i in range(10):
        fn(i % nset)
    torch.cuda.synchronize()
    windows = []
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(iters):
            fn(i % nset)
        e1.record()
        torch.cuda.synchronize()
        windows.append(e0.elapsed_time(e1) * 1e3 / iters)
    return float(np.median(windows))


def timing():
    NSET, T = 4, 21
    tab = U.table(T, 0)
    keys, vals = tab.to(DEV)
    for G, R, mult in ((64, 1, 2), (64, 5, 2), (64, 5, 5)):
        sets = [dev(*U.make_corpus(G, R, T, mult, s)) for s in range(NSET)]
        n = mult * G
        scores, reward, b = out(n), out(n if mult > 2 else G), out(n)
        plain, df = (K.cider_d_multi, K.cider_d_multi_df) if mult > 2 else (K.cider_d, K.cider_d_df)
        ws = torch.empty(max(K.cider_d_multi_df_workspace_bytes(G, R, T, mult), K.cider_d_df_workspace_bytes(G, R, T, mult)), dtype=torch.uint8, device=DEV)
        tag = "G=%d R=%d T=%d mult=%d" % (G, R, T, mult)

        def mixed(i, first):
            first(i, None)
            K.bleu4(*sets[i], mult, b, base=scores, w_base=1.0, w_bleu=2.5, mixed=scores, reward=reward, loo=mult > 2)
        run_plain = lambda i, rw=reward: plain(*sets[i], mult, scores, reward=rw, workspace=ws)
        run_df = lambda i, rw=reward: df(*sets[i], mult, scores, keys, vals, tab.n_docs, reward=rw, workspace=ws)
        print("time %-44s %8.2f us" % (plain.__name__ + " " + tag, timed(run_plain)))
        print("time %-44s %8.2f us" % (df.__name__ + " " + tag, timed(run_df)))
        print("time %-44s %8.2f us" % (plain.__name__ + "+bleu4 " + tag, timed(lambda i: mixed(i, run_plain))))
        print("time %-44s %8.2f us" % (df.__name__ + "+bleu4 " + tag, timed(lambda i: mixed(i, run_df))))
    for G, Kn in ((64, 5), (1024, 5)):
        sets = [torch.from_numpy(U.make_corpus(G, 1, T, Kn, s)[0]).to(DEV) for s in range(NSET)]
        utility, pick = out(Kn * G), out(G, I32)
        ws = torch.empty(K.cider_d_consensus_workspace_bytes(G, Kn, T), dtype=torch.uint8, device=DEV)
        print("time %-44s %8.2f us" % ("cider_d_consensus G=%d K=%d T=%d" % (G, Kn, T),
                                      timed(lambda i: K.cider_d_consensus(sets[i], Kn, keys, vals, tab.n_docs, utility, pick, workspace=ws))))
    G, R, T = 1024, 5, 64
    ctab = CU.table(T)
    ckeys, cvals = ctab.to(DEV)
    sets = [dev(*CU.make_corpus(G, R, T, s)) for s in range(NSET)]
    cider, stats, lcs = out(G), out((G, 6), I32), out((G, R, 2), I32)
    ws = torch.empty(K.caption_eval_workspace_bytes(G, R, T), dtype=torch.uint8, device=DEV)
    print("time %-44s %8.2f us" % ("caption_eval G=%d R=%d T=%d" % (G, R, T),
                                  timed(lambda i: K.caption_eval(*sets[i], cider, stats, lcs, ckeys, cvals, ctab.n_docs, workspace=ws))))


if __name__ == "__main__":
    print("library:", os.environ.get("VLP_HIP_LIB", "(product)"), file=sys.stderr)
    timing() if "--time" in sys.argv else bits()
