"""SHA-256 of every output of the entry points that walk one fp16 logits row of the vocabulary (csrc/vocab_row.h): mlm_loss_fwd/bwd,
mlm_loss_ls_fwd/bwd, token_logprob_fwd/bwd, argmax_rows, argmax_rows2, vqa_answer_rows, logsoftmax_topk, logsoftmax_topk_list, sample_rows
and bce_loss_fwd/bwd, over a fixed set of seeded cases: run under two builds of the library (VLP_HIP_LIB=...) and diff the output to show
that a rewrite of these kernels leaves every bit where it was.  Every row buffer holds NaN in its padding [V, ld), every output starts from a
sentinel, and the whole buffer is hashed.  --time prints microseconds per launch at the shapes bench.py, tools/decode_bench.py and
tools/scst_bench.py issue by default instead (HIP events, a warm-up, rotating operand sets).
usage: python tools/row_kernel_bits.py [--time]"""
import hashlib, math, os, sys, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vlp_amd import _lib as K
from tests.hard_inputs import ce_hard_rows
DEV = torch.device("cuda:0")
HALF, F32, I64, I32 = torch.float16, torch.float32, torch.int64, torch.int32
SHAPES = [(28996, 29056), (1001, 1008), (17, 24), (8, 8), (1, 8)]
UNALIGNED = (1001, 1001)            # rows that are not 16-byte aligned: the scalar paths of top-k, sample_rows and argmax_rows
TOPK = (1, 3, 5, 16, 17)            # 17 runs the 256-thread kernel


def sha(*ts):
    h = hashlib.sha256()
    for t in ts:
        h.update(t.detach().contiguous().cpu().numpy().tobytes())
    return h.hexdigest()[:16]


def out(shape, dtype=F32):
    """An output that starts from a sentinel: an element a kernel stops writing shows in the hash."""
    return torch.full(shape if isinstance(shape, tuple) else (shape,), -7 if dtype in (I64, I32) else -7.25, dtype=dtype, device=DEV)


def padded(x, ld):
    """[rows, ld] with x in [:, :V] and NaN in [V, ld)."""
    buf = torch.full((x.shape[0], ld), float("nan"), dtype=x.dtype, device=DEV)
    buf[:, :x.shape[1]] = x
    return buf


def labels_for(rows, V, g):
    lab = torch.randint(0, V, (rows,), device=DEV, generator=g)
    lab[0] = V - 1
    lab[-1] = 0                                          # also the smoothed loss's ignore index
    if rows > 2:
        lab[1] = V - 1
    return lab


def ls_scalars(V, ls=0.1):
    s, c = ls / (V - 2), 1.0 - ls
    return s, c, (V - 2) * s + c, (V - 2) * s * math.log(s) + c * math.log(c)


def loss_cases(tag, logits, V, lab, g):
    """mlm_loss (plain and smoothed, drop-worst 0 and 0.3), token_logprob and bce, forward and backward, on one [rows, ld] logits buffer."""
    rows, ld = logits.shape
    P = 3 if rows % 3 == 0 else 1
    B = rows // P
    w = (torch.rand(rows, device=DEV, generator=g) < 0.7).long()
    w.view(B, P)[:, 0] = 1
    gs = torch.full((1,), 128.0, device=DEV)
    for ratio in (0.0, 0.3):
        for smoothed in (False, True):
            if smoothed and V <= 2:
                continue
            loss, lse, coef, row, dl = out(1), out(rows), out(rows), out(rows), out((rows, ld), HALF)
            if smoothed:
                s, c, q_sum, q_log_q = ls_scalars(V)
                K.mlm_loss_ls_fwd(logits, ld, lab, w, loss, lse, coef, row, B, P, V, s, c, q_sum, q_log_q, ignore_index=0, drop_worst_ratio=ratio)
                K.mlm_loss_ls_bwd(logits, ld, lab, lse, coef, gs, dl, ld, rows, V, s, c, q_sum, ignore_index=0)
            else:
                K.mlm_loss_fwd(logits, ld, lab, w, loss, lse, coef, row, B, P, V, drop_worst_ratio=ratio)
                K.mlm_loss_bwd(logits, ld, lab, lse, coef, gs, dl, ld, rows, V)
            name = "mlm_loss_ls" if smoothed else "mlm_loss"
            print("%-22s %s drop=%.1f  fwd %s  bwd %s" % (name, tag, ratio, sha(loss, lse, coef, row), sha(dl)))
    logp, lse, dl = out(rows), out(rows), out((rows, ld), HALF)
    grow = torch.randn(rows, device=DEV, generator=g) * 64.0
    K.token_logprob_fwd(logits, ld, lab, logp, lse, rows, V)
    K.token_logprob_bwd(logits, ld, lab, lse, grow, dl, ld, rows, V)
    print("%-22s %s  fwd %s  bwd %s" % ("token_logprob", tag, sha(logp, lse), sha(dl)))
    y = padded(torch.rand(rows, V, device=DEV, generator=g), ld)
    loss257, dl = out(257), out((rows, ld), HALF)
    K.bce_loss_fwd(logits, ld, y, ld, rows, V, loss257)
    K.bce_loss_bwd(logits, ld, y, ld, rows, V, gs, dl, ld)
    print("%-22s %s  fwd %s  bwd %s" % ("bce_loss", tag, sha(loss257), sha(dl)))


def select_cases(tag, logits, V, g):
    """argmax_rows, argmax_rows2 (16-byte aligned rows only), vqa_answer_rows, sample_rows and the top-k forms on one [rows, ld] logits buffer."""
    rows, ld = logits.shape
    aligned = ld % 8 == 0
    for name, x in (("", logits), (" -inf row 0", torch.cat([torch.full_like(logits[:1], float("-inf")), logits[1:]]))):
        ids, vals = out(rows, I64), out(rows)
        K.argmax_rows(x, ld, rows, V, ids, vals)
        print("%-22s %s%s  %s" % ("argmax_rows", tag, name, sha(ids, vals)))
        if aligned:
            ida, idb, v2 = out(rows, I64), out(rows, I64), out(rows)
            K.argmax_rows2(x, ld, rows, V, ida, idb, v2)
            print("%-22s %s%s  %s" % ("argmax_rows2", tag, name, sha(ida, idb, v2)))
        if V > 1:
            S = 4
            aidx = torch.randint(-1, V, (rows, S), device=DEV, generator=g).to(I32)
            asc = torch.rand(rows, S, device=DEV, generator=g)
            oid, ov, osc = out(rows, I64), out(rows), out(rows)
            K.vqa_answer_rows(x, ld, rows, V, 1, oid, ov, aidx, asc, osc)
            print("%-22s %s%s  %s" % ("vqa_answer_rows", tag, name, sha(oid, ov, osc)))
    sid, slp = out(rows, I64), out(rows)
    K.sample_rows(logits, ld, rows, V, 17, 3, sid, slp)
    print("%-22s %s  %s" % ("sample_rows", tag, sha(sid, slp)))
    forbid = (torch.rand(rows, V, device=DEV, generator=g) < 0.3).to(torch.uint8)
    C = min(V, 40)
    cand = torch.stack([torch.randperm(V, device=DEV, generator=g)[:C] for _ in range(rows)]).to(I32)
    cnt = torch.randint(0, C + 1, (rows,), device=DEV, generator=g).to(I32)
    amax = logits[:, :V].float().argmax(1)
    cand[:, 0] = amax.to(I32)                            # the best word of a row is on its list whenever the list is not empty
    eos = int(amax[0])
    for Kb in TOPK:
        if Kb > V:
            continue
        for block_eos in (False, True):
            hs = []
            for mode in ("none", "dense", "list"):
                sc, oi = out((rows, Kb)), out((rows, Kb), I64)
                if mode == "list":
                    K.logsoftmax_topk_list(logits, ld, rows, V, Kb, sc, oi, cand, cnt, eos_id=eos, block_eos=block_eos)
                else:
                    K.logsoftmax_topk(logits, ld, rows, V, Kb, sc, oi, forbid=forbid if mode == "dense" else None, eos_id=eos, block_eos=block_eos)
                hs.append("%s %s" % (mode, sha(sc, oi)))
            print("%-22s %s K=%-2d eos=%d  %s" % ("logsoftmax_topk", tag, Kb, block_eos, "  ".join(hs)))


def bits():
    for V, ld in SHAPES + [UNALIGNED]:
        for rows in (1, 5, 48):
            g = torch.Generator(device=DEV); g.manual_seed(1000 * rows + V)
            logits = padded((torch.randn(rows, V, device=DEV, generator=g) * 2.0).half(), ld)
            tag = "V=%-5d ld=%-5d rows=%-2d" % (V, ld, rows)
            if ld % 8 == 0:
                loss_cases(tag, logits, V, labels_for(rows, V, g), g)
            select_cases(tag, logits, V, g)
    for V, ld in SHAPES[:2]:                             # the hard rows of tests/hard_inputs.py
        x, lab = ce_hard_rows(V, device=DEV)
        g = torch.Generator(device=DEV); g.manual_seed(V)
        tag = "V=%-5d ld=%-5d hard   " % (V, ld)
        loss_cases(tag, padded(x, ld), V, lab, g)
        select_cases(tag, padded(x, ld), V, g)
    torch.cuda.synchronize()


def timing():
    V, ld, NSET = 28996, 29056, 6
    g = torch.Generator(device=DEV); g.manual_seed(0)
    R_MLM, R_TOK, R_DEC = 64 * 3, 64 * 21, 64            # bench.py (B = 64, 3 masked positions), scst_bench.py (B = 64, T = 21), decode_bench.py (B = 64)
    logits = [padded((torch.randn(R_TOK, V, device=DEV, generator=g) * 2.0).half(), ld) for _ in range(NSET)]
    dl = [torch.empty(R_TOK, ld, dtype=HALF, device=DEV) for _ in range(NSET)]
    lab = torch.randint(1, V, (R_TOK,), device=DEV, generator=g)
    w = torch.ones(R_TOK, dtype=I64, device=DEV)
    f = [out(R_TOK * 16) for _ in range(4)]            # [0] also takes the [rows, K] top-k scores
    i64 = [out(R_TOK * 16, I64) for _ in range(2)]
    gs = torch.full((1,), 128.0, device=DEV)
    s, c, q_sum, q_log_q = ls_scalars(V)
    NA, ldv = 3129, 3136                                 # the VQA 2.0 answer vocabulary
    vq = padded((torch.randn(R_DEC, NA, device=DEV, generator=g) * 2.0).half(), ldv)
    yv = padded(torch.rand(R_DEC, NA, device=DEV, generator=g), ldv)
    cand = torch.randint(0, V, (320, 24), device=DEV, generator=g).to(I32)
    cnt = torch.full((320,), 20, dtype=I32, device=DEV)
    ops = [
        ("mlm_loss_fwd rows=192", lambda i: K.mlm_loss_fwd(logits[i], ld, lab, w, f[0], f[1], f[2], f[3], 64, 3, V, drop_worst_ratio=0.0)),
        ("mlm_loss_bwd rows=192", lambda i: K.mlm_loss_bwd(logits[i], ld, lab, f[1], f[2], gs, dl[i], ld, R_MLM, V)),
        ("mlm_loss_ls_fwd rows=192", lambda i: K.mlm_loss_ls_fwd(logits[i], ld, lab, w, f[0], f[1], f[2], f[3], 64, 3, V, s, c, q_sum, q_log_q)),
        ("mlm_loss_ls_bwd rows=192", lambda i: K.mlm_loss_ls_bwd(logits[i], ld, lab, f[1], f[2], gs, dl[i], ld, R_MLM, V, s, c, q_sum)),
        ("token_logprob_fwd rows=1344", lambda i: K.token_logprob_fwd(logits[i], ld, lab, f[0], f[1], R_TOK, V)),
        ("token_logprob_bwd rows=1344", lambda i: K.token_logprob_bwd(logits[i], ld, lab, f[1], f[2], dl[i], ld, R_TOK, V)),
        ("argmax_rows rows=64", lambda i: K.argmax_rows(logits[i], ld, R_DEC, V, i64[0], f[0])),
        ("argmax_rows2 rows=64", lambda i: K.argmax_rows2(logits[i], ld, R_DEC, V, i64[0], i64[1], f[0])),
        ("sample_rows rows=64", lambda i: K.sample_rows(logits[i], ld, R_DEC, V, 17, i, i64[0], f[0])),
        ("vqa_answer_rows rows=64 N=3129", lambda i: K.vqa_answer_rows(vq, ldv, R_DEC, NA, 1, i64[0], f[0])),
        ("bce_loss_fwd B=64 N=3129", lambda i: K.bce_loss_fwd(vq, ldv, yv, ldv, R_DEC, NA, f[3])),
        ("bce_loss_bwd B=64 N=3129", lambda i: K.bce_loss_bwd(vq, ldv, yv, ldv, R_DEC, NA, gs, dl[i], ldv)),
        ("logsoftmax_topk rows=192 K=3", lambda i: K.logsoftmax_topk(logits[i], ld, 192, V, 3, f[0], i64[0], eos_id=102, block_eos=True)),
        ("logsoftmax_topk rows=320 K=5", lambda i: K.logsoftmax_topk(logits[i], ld, 320, V, 5, f[0], i64[0], eos_id=102, block_eos=True)),
        ("logsoftmax_topk_list rows=192 K=3", lambda i: K.logsoftmax_topk_list(logits[i], ld, 192, V, 3, f[0], i64[0], cand, cnt, eos_id=102, block_eos=True)),
        ("logsoftmax_topk_list rows=320 K=5", lambda i: K.logsoftmax_topk_list(logits[i], ld, 320, V, 5, f[0], i64[0], cand, cnt, eos_id=102, block_eos=True)),
        ("logsoftmax_topk rows=64 K=17", lambda i: K.logsoftmax_topk(logits[i], ld, 64, V, 17, f[0], i64[0], eos_id=102, block_eos=True)),
    ]
    f[1].fill_(11.0); f[2].fill_(1e-3)                   # an lse and a coef the backward kernels can use
    for name, op in ops:
        for i in range(NSET):
            op(i)
        torch.cuda.synchronize()
        f[1].fill_(11.0); f[2].fill_(1e-3)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        n = 60
        a.record()
        for i in range(n):
            op(i % NSET)
        b.record(); torch.cuda.synchronize()
        print("time %-36s %8.2f us per launch" % (name, a.elapsed_time(b) / n * 1e3))
        f[1].fill_(11.0); f[2].fill_(1e-3)


if __name__ == "__main__":
    print("library:", os.environ.get("VLP_HIP_LIB", "(product)"))
    timing() if "--time" in sys.argv else bits()
