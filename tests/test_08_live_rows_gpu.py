"""GPU: the listed-row backward of the last encoder layer (Engine._bwd_layer with listed=True) and the kernels under it.

In a masked-LM step the gradient that enters the encoder is zero outside the masked rows, so the last layer's LayerNorm backwards, FFN /
attention-output dgrads and their weight gradients walk a device list of the distinct masked rows (vlp_live_rows_build, vlp_gemm_nt_rows,
vlp_gemm_tn_grouped_rows, vlp_layernorm_bwd_rows) instead of all M rows.

Kernel level: every listed kernel against the SAME kernel without a list on inputs whose dead rows are zero.  Row-local results (dgrad rows,
LayerNorm dx rows) must be bit-equal; sums over rows (weight / bias gradients, dgamma / dbeta) are compared with an fp64 evaluation of the same
fp16 operands, and the listed launch may exceed the unlisted launch's own error by at most one fp16 ulp of the largest output magnitude (the
bound comes from the unlisted path, never from the code under test).

Step level: model + backward with the path on against VLP_LAST_LAYER_LIVE=0 in one process, NT variant forced equal (17) in both runs.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from oracle import vlp_oracle as O                                      # noqa: E402 (checker)
from tests.guard_util import assert_untouched, guarded                  # noqa: E402
from tests.kernel_util import DEV, h16                                  # noqa: E402
from vlp_amd import _lib as K                                           # noqa: E402
from vlp_amd import synthetic as S                                      # noqa: E402
from vlp_amd.modeling import BertConfig, BertForPreTrainingLossMask     # noqa: E402

H, I = 768, 3072
KB, KP, KL = 3, 60, 111          # kernel-level list: 180 entries over M = 333 rows (not a multiple of any tile), ~140 distinct -> two 128-row tiles
KM = KB * KL


def ulp16(x):
    """One fp16 ulp at magnitude x (normal range)."""
    x = float(x)
    return 2.0 ** (math.floor(math.log2(x)) - 10) if x > 2.0 ** -14 else 2.0 ** -24


def host_rows(pos, L, row_off=None):
    """The distinct rows scatter_add_rows adds to, ascending (the host statement of vlp_live_rows_build)."""
    B, P = pos.shape
    rows = set()
    for b in range(B):
        base, n = (b * L, L) if row_off is None else (int(row_off[b]), int(row_off[b + 1] - row_off[b]))
        for j in range(P):
            rows.add(base + min(max(int(pos[b, j]), 0), n - 1))
    return sorted(rows)


def build_live(pos, L, row_off=None):
    B, P = pos.shape
    live = torch.full((B * P,), 12345, device=DEV, dtype=torch.int32)
    cnt = torch.full((1,), -7, device=DEV, dtype=torch.int32)
    K.live_rows_build(pos.to(DEV), B, P, L, live, cnt, row_off=None if row_off is None else row_off.to(DEV))
    return live, int(cnt.item())


_KLIST = {}


def kernel_list():
    """Shared by the kernel tests: pos [3, 60] with duplicates, position 0 several times and the last row of the batch; the device list."""
    if not _KLIST:
        g = torch.Generator().manual_seed(808)
        pos = torch.randint(0, KL, (KB, KP), generator=g)
        pos[0, 1] = pos[0, 0]                 # a duplicate
        pos[0, 2] = 0
        pos[1, 5] = 0                         # the pad position of a real batch
        pos[1, 6] = 0
        pos[2, 0] = KL - 1                    # last row of the batch
        live, n = build_live(pos, KL)
        rows = host_rows(pos, KL)
        _KLIST.update(pos=pos, live=live, n=n, rows=rows, idx=torch.tensor(rows, device=DEV, dtype=torch.long))
    return _KLIST


def dead_zero(t, idx):
    out = torch.zeros_like(t)
    out[idx] = t[idx]
    return out


def test_live_rows_build_dedup_order_padding():
    kl = kernel_list()
    assert kl["n"] == len(kl["rows"]) and 128 < kl["n"] < KB * KP
    assert kl["live"][:kl["n"]].tolist() == kl["rows"]
    assert bool((kl["live"][kl["n"]:] == -1).all())
    assert kl["rows"][0] == 0 and kl["rows"][-1] == KM - 1
    # packed rows: bases from row_off, positions clamped into the kept rows (as vlp_scatter_add_rows does)
    row_off = torch.tensor([0, 40, 41, 120], dtype=torch.int32)
    live, n = build_live(kl["pos"], KL, row_off)
    rows = host_rows(kl["pos"], KL, row_off)
    assert n == len(rows) and live[:n].tolist() == rows and bool((live[n:] == -1).all())
    assert rows[-1] == 119 and 40 in rows
    # every entry the same row; a single entry
    live, n = build_live(torch.full((2, 3), 5, dtype=torch.long), 9)
    assert n == 2 and live.tolist() == [5, 14, -1, -1, -1, -1]
    live, n = build_live(torch.tensor([[7]]), 9)
    assert n == 1 and live.tolist() == [7]


# --------------------------------------------------------------------------------------------------------------------------------------
# NT dgrad
# --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,Kd,mul,res,drop", [(I, H, True, False, 0.0), (H, I, False, True, 0.0), (H, H, False, False, 0.0), (H, H, True, True, 0.1)])
def test_nt_rows_equal_the_unlisted_launch(N, Kd, mul, res, drop):
    kl = kernel_list()
    live, n, idx, Rm = kl["live"], kl["n"], kl["idx"], KB * KP
    g = torch.Generator(device=DEV).manual_seed(N + Kd)
    x = dead_zero(h16(KM, Kd, gen=g), idx)
    w = h16(N, Kd, scale=Kd ** -0.5, gen=g)
    ms = h16(KM, N, gen=g) if mul else None
    rs = dead_zero(h16(KM, N, gen=g), idx) if res else None
    rm = (torch.arange(KM, device=DEV, dtype=torch.int32) + torch.arange(KM, device=DEV, dtype=torch.int32) // 50 * 7) if drop else None
    kw = dict(mul_src=ms, mul_mode=K.MUL_PLAIN if mul else K.MUL_NONE, residual=rs, dropout_p=drop, seed=77, rng_stream=5, row_map=rm)
    y_full = torch.empty(KM, N, device=DEV, dtype=torch.float16)
    K.gemm_nt(x, w, y_full, KM, N, Kd, variant=17, **kw)
    assert K.gemm_nt_resolved_variant() == 17
    fl_in = (K.ROWS_MUL if mul else 0) | (K.ROWS_RES if res else 0)
    # (a) operands read in place at live[m], compact output between guard bands
    yc = guarded(Rm, N, fill="sentinel", device=DEV)
    K.gemm_nt_rows(x, w, yc.view, live, K.ROWS_X | fl_in, Rm, N, Kd, **kw)
    assert K.gemm_nt_resolved_variant() == 17
    assert torch.equal(yc.view[:n], y_full[idx])
    wr = torch.zeros(Rm, N, dtype=torch.bool, device=DEV)
    wr[:n] = True
    assert_untouched(yc, written=wr, name="compact Y")
    # (b) compact X (pad rows poisoned), output written at live[m] of a cleared full buffer
    xc = torch.full((Rm, Kd), float("nan"), device=DEV, dtype=torch.float16)
    xc[:n] = x[idx]
    yf = guarded(KM, N, fill=0.0, device=DEV)
    K.gemm_nt_rows(xc, w, yf.view, live, fl_in | K.ROWS_Y, Rm, N, Kd, **kw)
    assert torch.equal(yf.view[idx], y_full[idx])
    wr = torch.zeros(KM, N, dtype=torch.bool, device=DEV)
    wr[idx] = True
    assert_untouched(yf, written=wr, name="indexed Y")
    # the variants the step's unlisted launches use at these shapes: both paths against fp64 of the same fp16 operands
    ref = x.double() @ w.double().t()
    if mul:
        ref = ref * ms.double()
    if not drop:
        if res:
            ref = ref + rs.double()
        ref = ref[idx]
        one = ulp16(ref.abs().max())
        e_list = float((yc.view[:n].double() - ref).abs().max())
        for v in (29, 77):
            K.gemm_nt(x, w, y_full, KM, N, Kd, variant=v, **kw)
            e_full = float((y_full[idx].double() - ref).abs().max())
            print("nt N=%d K=%d variant %d: listed err %.3e, unlisted err %.3e, ulp %.3e" % (N, Kd, K.gemm_nt_resolved_variant(), e_list, e_full, one))
            assert e_list <= e_full + one


# --------------------------------------------------------------------------------------------------------------------------------------
# grouped TN
# --------------------------------------------------------------------------------------------------------------------------------------
def test_tn_grouped_rows_against_fp64_and_the_unlisted_launch():
    kl = kernel_list()
    live, n, idx, Rm = kl["live"], kl["n"], kl["idx"], KB * KP
    g = torch.Generator(device=DEV).manual_seed(4)
    shapes = [(H, I), (I, H), (3 * H, H), (H, H)]           # (N, K): FFN down, FFN up, QKV (unlisted), attention output
    dys = [h16(KM, N, scale=0.25, gen=g) for N, _ in shapes]
    acts = [h16(KM, Kd, gen=g) for _, Kd in shapes]
    for j in (0, 1, 3):
        dys[j] = dead_zero(dys[j], idx)

    def outs():
        return [torch.full((N, Kd), float("nan"), device=DEV, dtype=torch.float16) for N, Kd in shapes], \
               [torch.full((N,), float("nan"), device=DEV, dtype=torch.float16) for N, _ in shapes]

    c_full, b_full = outs()
    K.gemm_tn_grouped([(dys[j], acts[j], c_full[j], KM, N, Kd, 0, b_full[j]) for j, (N, Kd) in enumerate(shapes)])

    def compact(t):
        c = torch.full((Rm, t.shape[1]), float("nan"), device=DEV, dtype=torch.float16)       # pad rows poisoned: a pad must add nothing
        c[:n] = t[idx]
        return c

    def listed(lv):
        c, b = outs()
        probs = []
        for j, (N, Kd) in enumerate(shapes):
            if j == 2:
                probs.append((dys[j], acts[j], c[j], KM, N, Kd, 0, b[j], None, 0))
            elif j == 3:      # dY read in place at live[m] (the dropout-off form of the attention-output wgrad)
                probs.append((dys[j], acts[j], c[j], Rm, N, Kd, 0, b[j], lv, K.ROWS_X))
            else:
                probs.append((compact(dys[j]), acts[j], c[j], Rm, N, Kd, 0, b[j], lv, 0))
        K.gemm_tn_grouped_rows(probs)
        return c, b

    c1, b1 = listed(live)
    c2, b2 = listed(live)
    for j in range(4):
        assert torch.equal(c1[j], c2[j]) and torch.equal(b1[j], b2[j]), "listed wgrad %d is not deterministic" % j
    assert torch.equal(c1[2], c_full[2]) and torch.equal(b1[2], b_full[2])       # the unlisted problem of the same launch
    # a list de-duplicated on the host gives the same bits as the device list built from positions with duplicates
    dedup = torch.full((Rm,), -1, device=DEV, dtype=torch.int32)
    dedup[:n] = idx.to(torch.int32)
    assert torch.equal(dedup, live)
    c3, b3 = listed(dedup)
    for j in range(4):
        assert torch.equal(c1[j], c3[j]) and torch.equal(b1[j], b3[j])
    for j in (0, 1, 3):
        ref = dys[j].double().t() @ acts[j].double()
        rb = dys[j].double().sum(0)
        for name, got, full, r in (("dW", c1[j], c_full[j], ref), ("db", b1[j], b_full[j], rb)):
            one = ulp16(r.abs().max())
            e_list, e_full = float((got.double() - r).abs().max()), float((full.double() - r).abs().max())
            print("tn problem %d %s: listed err %.3e, unlisted err %.3e, ulp %.3e" % (j, name, e_list, e_full, one))
            assert e_list <= e_full + one
    # beta = 1 accumulates
    c4 = [t.clone() for t in c1]
    b4 = [t.clone() for t in b1]
    K.gemm_tn_grouped_rows([(compact(dys[0]), acts[0], c4[0], Rm, H, I, 1, b4[0], live, 0)])
    assert torch.equal(c4[0], (c1[0].float() * 2).half()) and torch.equal(b4[0], (b1[0].float() * 2).half())


# --------------------------------------------------------------------------------------------------------------------------------------
# LayerNorm backward
# --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("drop,packed", [(0.0, False), (0.1, False), (0.1, True)])
def test_layernorm_bwd_rows(drop, packed):
    kl = kernel_list()
    live, n, idx, Rm = kl["live"], kl["n"], kl["idx"], KB * KP
    g = torch.Generator(device=DEV).manual_seed(11)
    pre = h16(KM, H, gen=g)
    gamma = (1.0 + 0.1 * torch.randn(H, device=DEV, generator=g)).half()
    mean = pre.float().mean(1)
    rstd = 1.0 / torch.sqrt(pre.float().var(1, unbiased=False) + 1e-12)
    dy = dead_zero(h16(KM, H, gen=g), idx)
    rm = (torch.arange(KM, device=DEV, dtype=torch.int32) + torch.arange(KM, device=DEV, dtype=torch.int32) // 50 * 7) if packed else None
    od = (drop, 99, 35)
    slot_bytes = K.layernorm_bwd_workspace_bytes(H)

    def params():
        return torch.full((H,), float("nan"), device=DEV, dtype=torch.float16), torch.full((H,), float("nan"), device=DEV, dtype=torch.float16)

    def reduce(slot, dg, db):
        table = torch.tensor([[dg.data_ptr(), db.data_ptr()]], device=DEV, dtype=torch.int64)
        K.layernorm_bwd_reduce_batched(slot, table, 1, KM, H, beta=0)
        torch.cuda.synchronize()

    slot_f = torch.empty(slot_bytes, device=DEV, dtype=torch.uint8)
    dx_f = torch.empty(KM, H, device=DEV, dtype=torch.float16)
    tw_f = torch.empty(KM, H, device=DEV, dtype=torch.float16) if drop else None
    dg_f, db_f = params()
    K.layernorm_bwd(dy, pre, gamma, mean, rstd, dx_f, dg_f, db_f, KM, H, slot_f, dx_drop=tw_f, out_drop=od, defer_reduce=True, row_map=rm)
    reduce(slot_f, dg_f, db_f)

    def nan_slot():
        return torch.full((slot_bytes // 4,), float("nan"), device=DEV, dtype=torch.float32)      # stale partials would poison the reduce

    # (a) dy read in place at live[m]; compact dx and twin between guard bands
    slot_a = nan_slot()
    dxc = guarded(Rm, H, fill="sentinel", device=DEV)
    twc = guarded(Rm, H, fill="sentinel", device=DEV)
    dg_a, db_a = params()
    K.layernorm_bwd_rows(dy, pre, gamma, mean, rstd, dxc.view, dg_a, db_a, live, K.ROWS_X, Rm, H, slot_a, KM, dx_drop=twc.view if drop else None,
                         out_drop=od, defer_reduce=True, row_map=rm)
    reduce(slot_a, dg_a, db_a)
    ne = dxc.view[:n] != dx_f[idx]
    assert not bool(ne.any()), "%d elements differ, max |diff| %.3e, first at %s" % (int(ne.sum()), float((dxc.view[:n].float() - dx_f[idx].float()).abs().max()),
                                                                                  torch.nonzero(ne)[0].tolist())
    wr = torch.zeros(Rm, H, dtype=torch.bool, device=DEV)
    wr[:n] = True
    assert_untouched(dxc, written=wr, name="compact dx")
    if drop:
        assert torch.equal(twc.view[:n], tw_f[idx])
        assert not torch.equal(tw_f[idx], dx_f[idx])
        assert_untouched(twc, written=wr, name="compact twin")
    else:
        assert_untouched(twc, written=None, name="twin (no dropout)")
    # (b) compact dy (pad rows poisoned), dx written at live[m] of a cleared full buffer, twin compact
    slot_b = nan_slot()
    dyc = torch.full((Rm, H), float("nan"), device=DEV, dtype=torch.float16)
    dyc[:n] = dy[idx]
    dxf = guarded(KM, H, fill=0.0, device=DEV)
    twc2 = guarded(Rm, H, fill="sentinel", device=DEV)
    dg_b, db_b = params()
    K.layernorm_bwd_rows(dyc, pre, gamma, mean, rstd, dxf.view, dg_b, db_b, live, K.ROWS_Y, Rm, H, slot_b, KM, dx_drop=twc2.view if drop else None,
                         out_drop=od, defer_reduce=True, row_map=rm)
    reduce(slot_b, dg_b, db_b)
    assert torch.equal(dxf.view[idx], dx_f[idx])
    wf = torch.zeros(KM, H, dtype=torch.bool, device=DEV)
    wf[idx] = True
    assert_untouched(dxf, written=wf, name="indexed dx")
    if drop:
        assert torch.equal(twc2.view[:n], tw_f[idx])
    # dgamma / dbeta after the batched reduce: fp64 of the same operands, the unlisted launch's own error is the ceiling
    xh = (pre.double() - mean.double()[:, None]) * rstd.double()[:, None]
    for name, r, full, got in (("dgamma", (dy.double() * xh).sum(0), dg_f, (dg_a, dg_b)), ("dbeta", dy.double().sum(0), db_f, (db_a, db_b))):
        one = ulp16(r.abs().max())
        e_full = float((full.double() - r).abs().max())
        for t in got:
            assert bool(torch.isfinite(t).all()), name + ": stale / undefined partial rows reached the reduce"
            assert torch.equal(t, full), name + ": the listed rows are summed by the waves, and in the order, of the unlisted launch"
            e_list = float((t.double() - r).abs().max())
            print("ln %s: listed err %.3e, unlisted err %.3e, ulp %.3e" % (name, e_list, e_full, one))
            assert e_list <= e_full + one


# --------------------------------------------------------------------------------------------------------------------------------------
# step level
# --------------------------------------------------------------------------------------------------------------------------------------
NV, NL_ = 8, 2
LAST = "bert.encoder.layer.%d." % (NL_ - 1)
# the last layer's gradients that are sums over the listed rows (everything else is downstream of bit-equal rows)
SUMMED = [LAST + s for s in ("output.dense.weight", "output.dense.bias", "intermediate.dense.weight", "intermediate.dense.bias",
                             "attention.output.dense.weight", "attention.output.dense.bias")]
LN_SUMMED = [LAST + s for s in ("output.LayerNorm.weight", "output.LayerNorm.bias", "attention.output.LayerNorm.weight", "attention.output.LayerNorm.bias")]
_STEP = {}


def step_batch():
    """B = 3, max_len_b = 21, 8 regions (L = 32, M = 96), P = 3; sample 0 names one row twice and carries a weight-0 pad at position 0; the
    last sample is full length and has a masked position in the last row of the batch."""
    if "raw" not in _STEP:
        for seed in range(31, 200):
            raw = S.make_batch(3, max_len_b=21, len_vis_input=NV, vocab_size=1024, max_pred=3, s2s_prob=0.5, seed=seed)
            L = raw.input_ids.shape[1]
            lens = [int(raw.input_mask[i].any(dim=0).nonzero().max()) + 1 for i in range(3)]
            if lens[2] == L and min(lens) < L:
                break
        else:
            raise AssertionError("no seed gives a full-length last sample")
        mp, mw = raw.masked_pos.clone(), raw.masked_weights.clone()
        mp[0] = torch.tensor([int(mp[0, 0]), int(mp[0, 0]), 0])
        mw[0] = torch.tensor([1, 1, 0])
        mp[2, 0] = L - 1
        mw[2, 0] = 1
        raw = raw._replace(masked_pos=mp, masked_weights=mw)
        _STEP.update(raw=raw, L=L, lens=lens, p=O.init_params(vocab_size=1024, layers=NL_, tasks="img2txt", seed=21))
    return _STEP


def step_model(drop, tasks="img2txt", p=None):
    p = step_batch()["p"] if p is None else p
    cfg = BertConfig(1024, num_hidden_layers=NL_, type_vocab_size=6, hidden_dropout_prob=drop, attention_probs_dropout_prob=drop)
    m = BertForPreTrainingLossMask(cfg, enable_butd=True, len_vis_input=NV, tasks=tasks, allow_random_fc7=True)
    sd = dict(p)
    sd["cls.predictions.decoder.weight"] = p["bert.embeddings.word_embeddings.weight"]
    m.load_state_dict(sd, strict=True)
    return m.half().to(DEV).train()


def run_step(m, b, mir=False):
    lt = m(b.img, b.vis_pe, b.input_ids, b.segment_ids, b.input_mask, b.lm_label_ids, b.ans_labels, b.is_next, masked_pos=b.masked_pos,
           masked_weights=b.masked_weights, task_idx=b.task_idx, vis_masked_pos=b.vis_masked_pos, mask_image_regions=mir, drop_worst_ratio=0)
    ((lt[0] + lt[1] + lt[2]).sum() * 256.0).backward()
    torch.cuda.synchronize()
    return lt


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("drop", [0.0, 0.1])
@pytest.mark.parametrize("beta", [0, 1])
def test_step_with_the_list_equals_the_full_step(packed, drop, beta, monkeypatch):
    """Same weights, same batch, same seeds; NT variant 17 forced in both runs.  Losses, logits, every gradient outside the last layer's
    row sums and the dx that enters layer NL - 2 are bit-equal.  The FFN / attention-output weight and bias gradients of the last layer are
    compared with fp64 of the operands read back from the unlisted run's workspace (bound: that run's own error + one fp16 ulp of the
    largest magnitude per accumulated pass).  Its four LayerNorm parameter gradients are bit-equal too: the listed kernel gives every row to
    the wave that sums it in the unlisted launch, where the rows in between add exact zeros."""
    sb = step_batch()
    raw, L = sb["raw"], sb["L"]
    batch = S.batch_to(raw, DEV, half=True)
    ro = None
    if packed:
        ro = torch.tensor([0] + list(torch.tensor(sb["lens"]).cumsum(0)), dtype=torch.int32)
    want_rows = len(host_rows(raw.masked_pos, L, ro))
    assert want_rows < 3 * 3                  # nine entries, at least one duplicate
    res = {}
    for mode in ("full", "live"):
        monkeypatch.setenv("VLP_LAST_LAYER_LIVE", "0" if mode == "full" else "1")
        m = step_model(drop)
        eng = m.engine
        eng.varlen = packed
        eng.GEMM_NT_VARIANT = 17
        eng.step_seed = 1234
        ref64 = {n: 0.0 for n in SUMMED}
        dx_in = []                      # output of the last layer's QKV dgrad = the dx that enters layer NL - 2 (first [M, H] x [H, 3H] launch of a backward)
        nt = eng._nt

        def spy(x, w, y, M_, N, Kd, **kw):
            nt(x, w, y, M_, N, Kd, **kw)
            if N == H and Kd == 3 * H:
                dx_in.append(y[:M_].clone())
        monkeypatch.setattr(eng, "_nt", spy)
        for _ in range(beta + 1):
            lt = run_step(m, batch)
            assert (eng.last_packed_rows is not None) == packed
            M = eng.last_packed_rows if packed else 3 * L
            assert eng.last_live_rows == (want_rows if mode == "live" else None)
            if mode == "full":
                ws = eng._ws[next(iter(eng._ws))]
                ds, a = ws["dyset"][(NL_ - 1) & 1], ws["layers"][NL_ - 1]
                sfx = "_d" if drop else ""
                for (wn, bn), dyt, act in ((SUMMED[0:2], ds["dpre2" + sfx], a["g"]), (SUMMED[2:4], ds["dz"], a["x1"]), (SUMMED[4:6], ds["dpre1" + sfx], a["ctx"])):
                    ref64[wn] = ref64[wn] + dyt[:M].double().t() @ act[:M].double()
                    ref64[bn] = ref64[bn] + dyt[:M].double().sum(0)
        grads = {n: q.grad.detach().clone() for n, q in m.named_parameters()}
        res[mode] = dict(loss=torch.stack([x.detach().float().reshape(()) for x in lt]), logits=m.last_mlm_logits.clone(), grads=grads,
                         dx=dx_in[-NL_], ref64=ref64)
    f, l = res["full"], res["live"]
    assert torch.equal(f["loss"], l["loss"]) and torch.equal(f["logits"], l["logits"])
    assert torch.equal(f["dx"], l["dx"]), "dx entering layer NL-2"
    for n in f["grads"]:
        gf, gl = f["grads"][n], l["grads"][n]
        assert bool(torch.isfinite(gl).all()), n
        if n in SUMMED:
            r = f["ref64"][n]
            one = ulp16(r.abs().max()) * (beta + 1)
            e_full, e_list = float((gf.double() - r).abs().max()), float((gl.double() - r).abs().max())
            print("%s: listed err %.3e, unlisted err %.3e, ulp bound %.3e" % (n, e_list, e_full, one))
            assert e_list <= e_full + one, n
        elif n in LN_SUMMED:
            assert torch.equal(gf, gl), n          # a listed row is summed by the wave, and in the order, of the unlisted launch
        else:
            assert torch.equal(gf, gl), n


def test_steps_that_keep_the_full_path(monkeypatch):
    """vqa2, a pretext (vis_masked_pos) step, P = 0 and the log-probability backward send gradient to rows outside masked_pos (or have no
    masked rows): they run every row, and say so."""
    monkeypatch.delenv("VLP_LAST_LAYER_LIVE", raising=False)
    # vqa2
    p = O.init_params(vocab_size=1024, layers=NL_, tasks="vqa2", seed=5)
    m = step_model(0.0, tasks="vqa2", p=p)
    raw = S.make_batch(3, max_len_b=21, len_vis_input=NV, vocab_size=1024, tasks="vqa2", max_pred=1, seed=9)
    lt = run_step(m, S.batch_to(raw, DEV, half=True))
    assert m.engine.last_live_rows is None and bool(torch.isfinite(lt[2]).all())
    # pretext branch
    m = step_model(0.0)
    raw = S.make_batch(3, max_len_b=21, len_vis_input=NV, vocab_size=1024, max_pred=3, s2s_prob=0.5, seed=21, vis_mask_prob=0.25)
    lt = run_step(m, S.batch_to(raw, DEV, half=True), mir=True)
    assert m.engine.last_live_rows is None and bool(torch.isfinite(lt[1]).all())
    # the same model on a plain masked-LM batch takes the list, and P = 0 (no masked positions) does not
    sb = step_batch()
    run_step(m, S.batch_to(sb["raw"], DEV, half=True))
    assert m.engine.last_live_rows == len(host_rows(sb["raw"].masked_pos, sb["L"]))
    raw0 = S.make_batch(3, max_len_b=21, len_vis_input=NV, vocab_size=1024, max_pred=0, mask_prob=0.0, s2s_prob=0.5, seed=21, vis_mask_prob=0.25)
    assert raw0.masked_pos.shape[1] == 0
    run_step(m, S.batch_to(raw0, DEV, half=True), mir=True)
    assert m.engine.last_live_rows is None
    # task="logprob" (self-critical training): the existing comparison against the oracle, then the flag
    from tests.test_80_scst_gpu import _model_case
    dec, _ = _model_case(1024, 3, 5, 12, 21, 0.05, (0.0048, 0.0036, 0.07))
    assert dec.engine.last_live_rows is None
