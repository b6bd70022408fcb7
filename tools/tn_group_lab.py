"""Grouped wgrad lab: the four weight gradients of one BertLayer at the BASELINE shape (M = 10 688) in one vlp_gemm_tn_grouped launch, operand sets
rotated so every launch reads cold data (as in the step).  VLP_TN_GROUP_MODE selects tile shape / ring depth (read once per process).
   for m in 0 1 2 3; do VLP_TN_GROUP_MODE=$m python tools/tn_group_lab.py; done
Mapped mode (vlp_gemm_tn_grouped_mapped, the dense step's walk over the kept rows): KEPT=0.823,0.5,1.0 times, after the unmapped launch, the mapped
launch at each kept fraction -- 64 samples of 167 positions, sample b keeps its first n_b positions, the n_b spread around the fraction as the
synthetic batches' are; the rows past n_b of dY are zeros (as in the step), so every launch computes the same product and is checked against it."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vlp_amd import _lib as K  # noqa: E402

DEV = torch.device("cuda:0")
B, L = 64, 167
M, H, I = B * L, 768, 3072
ROT = int(os.environ.get("ROT", "6"))
KEPT = [float(x) for x in os.environ.get("KEPT", "").split(",") if x]


def kept_map(frac, seed=0):
    """(map [M] int32, count [1] int32, M') for per-sample kept lengths drawn around frac * L (at least 102 = 100 regions + 2)."""
    g = torch.Generator().manual_seed(seed)
    if frac >= 1.0:
        lens = torch.full((B,), L)
    else:
        lo = max(102, int(2 * frac * L) - L)
        lens = torch.randint(lo, L + 1, (B,), generator=g) if frac * L > 102 else torch.full((B,), max(1, int(frac * L)))
    rows = torch.cat([b * L + torch.arange(int(n)) for b, n in enumerate(lens)]).to(torch.int32)
    m = torch.full((M,), M - 1, dtype=torch.int32)
    m[:rows.numel()] = rows
    return m.to(DEV), torch.tensor([rows.numel()], dtype=torch.int32, device=DEV), int(rows.numel())


def main():
    g = torch.Generator(device=DEV)
    g.manual_seed(0)

    def r(*s):
        return (torch.randn(*s, device=DEV, generator=g) * 0.25).half()

    shapes = [(3 * H, H), (H, H), (I, H), (H, I)]           # (N of dY, K of X): w_qkv, w_out, w_ffn1, w_ffn2
    sets = []
    for _ in range(ROT):
        sets.append([(r(M, n), r(M, k), torch.empty(n, k, device=DEV, dtype=torch.half), torch.empty(n, device=DEV, dtype=torch.half)) for n, k in shapes])
    i = [0]

    tiles = sum((n // 128) * (k // 128) for n, k in shapes)
    wsk = torch.empty(K.gemm_tn_grouped_workspace_bytes(tiles), device=DEV, dtype=torch.uint8) if K.lab_build() else None      # stream-K form (mode 5, investigation library)

    def timed(launch, label):
        for _ in range(3):
            launch()
        torch.cuda.synchronize()
        st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        st.record()
        n = 24
        for _ in range(n):
            launch()
        en.record()
        torch.cuda.synchronize()
        us = st.elapsed_time(en) / n * 1e3
        # correctness of the last set against torch (fp32 accumulate)
        a, b, c, bias = sets[(i[0] - 1) % ROT][2]
        ref = (a.float().t() @ b.float())
        err = float((c.float() - ref).abs().max() / ref.abs().max())
        print("%s  %.1f us per layer  (w_ffn1 rel err %.2e)" % (label, us, err))
        return us

    def f():
        s = sets[i[0] % ROT]
        K.gemm_tn_grouped([(a, b, c, M, a.shape[1], b.shape[1], 0, bias) for a, b, c, bias in s], workspace=wsk)
        i[0] += 1

    gf = sum(2.0 * M * a * b for a, b in shapes) / 1e9
    us = timed(f, "mode %s" % os.environ.get("VLP_TN_GROUP_MODE", "0"))
    print("   %.0f TFLOP/s over all %d rows" % (gf / us * 1e3, M))
    for frac in KEPT:
        row_map, count, kept = kept_map(frac)
        dropped = torch.ones(M, dtype=torch.bool, device=DEV)
        dropped[row_map[:kept].long()] = False
        for s in sets:
            for a, _, _, _ in s:
                a[dropped] = 0          # dY of a dropped row is an exact zero in the step: mapped and unmapped launches compute the same product

        def fm():
            s = sets[i[0] % ROT]
            K.gemm_tn_grouped_mapped([(a, b, c, M, a.shape[1], b.shape[1], 0, bias) for a, b, c, bias in s], row_map, count)
            i[0] += 1

        u0 = timed(f, "kept %.3f (%5d of %d rows, %3d of %d stages): unmapped" % (frac, kept, M, (kept + 63) // 64, (M + 63) // 64))
        u1 = timed(fm, "kept %.3f (%5d of %d rows, %3d of %d stages): mapped  " % (frac, kept, M, (kept + 63) // 64, (M + 63) // 64))
        print("   mapped / unmapped %.3f, stages %.3f" % (u1 / u0, ((kept + 63) // 64) / ((M + 63) // 64)))


main()
