#!/usr/bin/env python
"""LayerNorm forward / backward lab (csrc/layernorm.hip).
Default: microseconds per launch at the step's shape (M = 64 x 167, H = 768), cold operands (12 rotating sets as the layers of a step).
--bits: one SHA-256 line per case over EVERY output of layernorm_fwd, layernorm_bwd (immediate, and defer_reduce +
layernorm_bwd_reduce_batched) and colsum -- y, mean, rstd, dx, dx_drop, dgamma, dbeta and the whole partials workspace -- on seeded inputs
with NaN in the padding of every row; every output starts from a sentinel and the whole buffer is hashed.  Run under two builds of the
library (VLP_HIP_LIB=...) and diff the output to show that a rewrite of these kernels leaves every bit where it was (tools/row_kernel_bits.py
is the same tool for the vocabulary-row kernels).
usage: python tools/ln_lab.py [--bits]"""
import os
import sys
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vlp_amd import _lib as K
from row_kernel_bits import out, padded, sha

DEV = "cuda"
M, H, ROT = 64 * 167, 768, 12
HALF, I32, I64 = torch.float16, torch.int32, torch.int64
BITS_H_BWD = (64, 256, 520, 768, 1024, 1032, 2048)       # 520 / 1032: column-predicated pieces; 768: the step's instantiations
BITS_H_FWD = BITS_H_BWD + (2056, 4096)                    # > 2048: forward only (NP = 16)
BITS_M = (1, 5, 257, 4100, 10688)                         # <= 4096: one row per wave at most; 4100: some waves two rows, the others one; 10688: the step
DROPS = (("off", 0.0, 0.0), ("dy", 0.2, 0.0), ("out", 0.0, 0.1), ("both", 0.2, 0.1))
COLSUM = ((1, 28996, 0), (63, 1001, 1), (2085, 7, 0), (333, 3129, 1), (4097, 1001, 0))          # tests/test_05: test_colsum_ragged


def logical_rows(n):
    """Packed row -> logical row: ascending, with gaps."""
    i = torch.arange(n, device=DEV)
    return (i + i // 100).to(I32)


def bench(fn, iters=120, warm=12):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3


def timing():
    g = torch.Generator(device=DEV)
    g.manual_seed(0)
    r = lambda *s: torch.randn(*s, device=DEV, generator=g).half()
    sets = []
    for _ in range(ROT):
        sets.append(dict(x=r(M, H), dy=r(M, H), y=torch.empty(M, H, device=DEV, dtype=torch.half), dx=torch.empty(M, H, device=DEV, dtype=torch.half),
                         dxd=torch.empty(M, H, device=DEV, dtype=torch.half), mean=torch.empty(M, device=DEV), rstd=torch.empty(M, device=DEV)))
    gamma, beta = r(H), r(H)
    dgam, dbet = torch.empty(H, device=DEV, dtype=torch.half), torch.empty(H, device=DEV, dtype=torch.half)
    ws = torch.empty(K.layernorm_bwd_workspace_bytes(H), device=DEV, dtype=torch.uint8)
    rmap = logical_rows(M)
    ctr = [0]

    def fwd(drop, row_map=None):
        s = sets[ctr[0] % ROT]
        ctr[0] += 1
        K.layernorm_fwd(s["x"], gamma, beta, s["y"], M, H, mean=s["mean"], rstd=s["rstd"], eps=1e-12, dropout_p=drop[0], seed=drop[1], rng_stream=drop[2],
                        row_map=row_map)

    def bwd(dyd, outd, deferred, row_map=None):
        s = sets[ctr[0] % ROT]
        ctr[0] += 1
        K.layernorm_bwd(s["dy"], s["x"], gamma, s["mean"], s["rstd"], s["dx"], dgam, dbet, M, H, ws, dx_drop=s["dxd"] if outd[0] > 0 else None,
                        dy_drop=dyd, out_drop=outd, defer_reduce=deferred, row_map=row_map)

    for s in sets:
        K.layernorm_fwd(s["x"], gamma, beta, s["y"], M, H, mean=s["mean"], rstd=s["rstd"], eps=1e-12)
    print("fwd plain            %6.1f us" % bench(lambda: fwd((0.0, 0, 0))))
    print("fwd dropout          %6.1f us" % bench(lambda: fwd((0.1, 1, 2))))
    print("fwd dropout row_map  %6.1f us" % bench(lambda: fwd((0.1, 1, 2), rmap)))
    print("bwd plain  deferred  %6.1f us" % bench(lambda: bwd((0.0, 0, 0), (0.0, 0, 0), True)))
    print("bwd dy-drop deferred %6.1f us" % bench(lambda: bwd((0.1, 1, 2), (0.0, 0, 0), True)))
    print("bwd out-drop deferred%6.1f us" % bench(lambda: bwd((0.0, 0, 0), (0.1, 1, 3), True)))
    print("bwd both   deferred  %6.1f us" % bench(lambda: bwd((0.1, 1, 2), (0.1, 1, 3), True)))
    print("bwd both row_map def.%6.1f us" % bench(lambda: bwd((0.1, 1, 2), (0.1, 1, 3), True, rmap)))
    print("bwd plain  + reduce  %6.1f us" % bench(lambda: bwd((0.0, 0, 0), (0.0, 0, 0), False)))


def bits_ln(Hh, Mm, pad):
    """Every forward and (H <= 2048) backward case of one (H, M, leading-dimension padding)."""
    g = torch.Generator(device=DEV)
    g.manual_seed(100003 * Hh + 7 * Mm + pad)
    r = lambda *s: torch.randn(*s, device=DEV, generator=g)
    ld = [Hh + k * pad for k in (1, 2, 3, 4, 5)]                   # x, y, dy, dx, dx_drop: all different when padded
    x, dy = padded((r(Mm, Hh) * 2.0).half(), ld[0]), padded(r(Mm, Hh).half(), ld[2])
    gamma, beta = (1 + 0.1 * r(Hh)).half(), (0.1 * r(Hh)).half()
    rmap = logical_rows(Mm)
    tag = "H=%-4d M=%-5d ld%sH" % (Hh, Mm, ">" if pad else "=")
    mean = rstd = None
    for p in (0.0, 0.1):
        for rm in (None, rmap):
            y, mean_o, rstd_o = out((Mm, ld[1]), HALF), out(Mm), out(Mm)
            K.layernorm_fwd(x[:, :Hh], gamma, beta, y[:, :Hh], Mm, Hh, mean_o, rstd_o, dropout_p=p, seed=5, rng_stream=1000, row_map=rm)
            print("layernorm_fwd %s p=%.1f map=%d  y %s  mean %s  rstd %s" % (tag, p, rm is not None, sha(y), sha(mean_o), sha(rstd_o)))
            if mean is None:
                mean, rstd = mean_o, rstd_o
    if Hh > 2048:
        return
    nws = K.layernorm_bwd_workspace_bytes(Hh) // 4
    init = [(0.5 * r(Hh)).half() for _ in range(4)]                # what beta = 1 accumulates onto
    # the cross product (dropout x row_map x beta) at the small M; at the large ones every (dropout, row_map) with beta alternating
    for di, (dname, p_dy, p_out) in enumerate(DROPS):
        for mi, rm in enumerate((None, rmap)):
            for acc in ((0, 1) if Mm <= 257 else ((di + mi) & 1,)):
                dyd, outd = (p_dy, 3, 9), (p_out, 4, 2)
                dx, dxd = out((Mm, ld[3]), HALF), out((Mm, ld[4]), HALF) if p_out else None
                dg, db, ws = init[0].clone(), init[1].clone(), out(nws)
                K.layernorm_bwd(dy[:, :Hh], x[:, :Hh], gamma, mean, rstd, dx[:, :Hh], dg, db, Mm, Hh, ws, beta=acc,
                                dx_drop=dxd[:, :Hh] if p_out else None, dy_drop=dyd, out_drop=outd, row_map=rm)
                now = "dx %s  dxd %s  dg %s  db %s  ws %s" % (sha(dx), sha(dxd) if p_out else "-" * 16, sha(dg), sha(db), sha(ws))
                # deferred: two LayerNorms (the second with x and dy swapped) into two slots, one batched reduce
                dx2 = [out((Mm, ld[3]), HALF) for _ in range(2)]
                dxd2 = [out((Mm, ld[4]), HALF) if p_out else None for _ in range(2)]
                dst = [t.clone() for t in init]
                slots = out(2 * nws)
                for i, (dy_i, x_i) in enumerate(((dy, x), (x, dy))):
                    K.layernorm_bwd(dy_i[:, :Hh], x_i[:, :Hh], gamma, mean, rstd, dx2[i][:, :Hh], dst[2 * i], dst[2 * i + 1], Mm, Hh,
                                    slots[i * nws:(i + 1) * nws], beta=acc, dx_drop=dxd2[i][:, :Hh] if p_out else None, dy_drop=dyd, out_drop=outd,
                                    defer_reduce=True, row_map=rm)
                kept = sha(*dst)                                   # defer_reduce leaves dgamma / dbeta alone
                table = torch.tensor([[dst[0].data_ptr(), dst[1].data_ptr()], [dst[2].data_ptr(), dst[3].data_ptr()]], dtype=I64, device=DEV)
                K.layernorm_bwd_reduce_batched(slots, table, 2, Mm, Hh, beta=acc)
                print("layernorm_bwd %s drop=%-4s map=%d beta=%d  %s  deferred: dx %s  dxd %s  kept %s  dg/db %s  ws %s" % (
                    tag, dname, mi, acc, now, sha(*dx2), sha(*dxd2) if p_out else "-" * 16, kept, sha(*dst), sha(slots)))


def bits():
    for Hh in BITS_H_FWD:
        for Mm in BITS_M:
            for pad in ((0, 8) if Mm <= 257 or Hh == H else (8,)):           # the large M: exact leading dimensions at the step's H only
                bits_ln(Hh, Mm, pad)
    for Mm, N, acc in COLSUM:
        g = torch.Generator(device=DEV)
        g.manual_seed(31 * Mm + N)
        a = padded(torch.randn(Mm, N, device=DEV, generator=g).half(), (N + 7) // 8 * 8 + 16)
        o = out(N, HALF)
        if acc:
            o.copy_(torch.randn(N, device=DEV, generator=g).half())
        ws = out(K.colsum_workspace_bytes(Mm, N) // 4)
        K.colsum(a[:, :N], o, Mm, N, beta=acc, workspace=ws)
        print("colsum M=%-5d N=%-5d beta=%d  out %s  ws %s" % (Mm, N, acc, sha(o), sha(ws)))
    torch.cuda.synchronize()


if __name__ == "__main__":
    print("library:", os.environ.get("VLP_HIP_LIB", "(product)"), file=sys.stderr)           # not part of the listing: two runs diff clean
    bits() if "--bits" in sys.argv else timing()
