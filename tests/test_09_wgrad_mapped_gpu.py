"""GPU: the mapped grouped wgrad of the dense step (vlp_gemm_tn_grouped_mapped) and the device map it walks (vlp_kept_rows_build).

In the dense step every position past a sample's last attended key is attended by no query and read by no head, so its dY row is an exact
zero in all four weight gradients of every layer (Engine._kept_lengths states the rule for the padding-free step).  The mapped launch
contracts over the compact list of the other rows: full 64-row stages gather their rows through the LDS-DMA path, the last partial stage is
zero-filled through registers, and the stage count follows a count that only the device knows.

Kernel level (one layer's four problems with N, K in {128, 384}, bias gradients, beta 0 and 1; six samples of 70 positions, kept lengths
(70, 41, 5, 0, 64, 65): stage 1 spans four samples, one of them empty; M' in {0, 1, 63, 64, 65, 128, 129, 245}):
  1. the identity map gives the bits of the unmapped launch;
  2. dropped rows are never read (NaN there: finite output, the bits of the run with zeros there);
  3. against the fp64 product of the fp16 operands the error stays inside the bound test_00's grouped-wgrad cases assert (rel() < 1.5e-3,
     accumulated 2.5e-3, bias 2e-3 of the largest column sum + 1e-2);
  4. out-of-range map entries and count are clamped: the run equals the run with the clamped values;
  5. vlp_kept_rows_build against a Python restatement of the rule of Engine._kept_lengths (s2s, bidirectional, MaskSpec lengths, a masked
     position past the last attended key).
Engine level (2 layers, 8 regions, B = 64, L = 35: M = 2240 >= 2048, dropout 0.1): VLP_WGRAD_KEPT on against off -- losses and logits equal
bit for bit, every gradient tensor within test_25's dense-against-packed bound (2e-4 rel-L2); three steps of different kept lengths on one
engine equal a fresh engine's bit for bit; the packed step does not change with the switch.
"""
import collections
import copy
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from oracle import vlp_oracle as O                                      # noqa: E402
from vlp_amd import _lib as K                                           # noqa: E402
from vlp_amd import synthetic as S                                      # noqa: E402
from vlp_amd.input_prep import MaskSpec                                 # noqa: E402
from vlp_amd.modeling import BertConfig, BertForPreTrainingLossMask     # noqa: E402
from tests.kernel_util import DEV, h16, rel                             # noqa: E402
from tests.step_seq_util import first_difference                        # noqa: E402

LENS = (70, 41, 5, 0, 64, 65)
LS = 70                                   # positions per sample
M = LS * len(LENS)                        # 420 dense rows = 6 full stages + 36
SHAPES = [(128, 384), (384, 128), (384, 384), (128, 128)]     # (N, K) of the four problems
COUNTS = [0, 1, 63, 64, 65, 128, 129, sum(LENS)]


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


@functools.lru_cache(maxsize=None)
def _operands():
    """(a, b) fp16 operands of the four problems, the start values of C / bias for beta = 1, the full kept map.  Built once, never modified."""
    gen = torch.Generator(device=DEV)
    gen.manual_seed(909)
    ops = []
    for N, Kd in SHAPES:
        ops.append((h16(M, N, scale=0.3, gen=gen), h16(M, Kd, scale=0.3, gen=gen), h16(N, Kd, gen=gen), h16(N, gen=gen)))
    kept = torch.cat([b * LS + torch.arange(n) for b, n in enumerate(LENS)]).to(torch.int32).to(DEV)
    return ops, kept


def _padded_map(rows):
    """An [M] map whose first len(rows) entries are `rows`; the rest names row 0 (never walked)."""
    m = torch.zeros(M, dtype=torch.int32, device=DEV)
    m[:rows.numel()] = rows
    return m


def _run(ops_ab, starts, row_map, count, beta, rows=M):
    """One launch over copies of the start values; row_map None = the unmapped launch.  Returns [(C, bias)]."""
    outs = [(c.clone(), bias.clone()) for c, bias in starts]
    probs = [(a, b, c, rows, N, Kd, beta, bias) for (a, b), (c, bias), (N, Kd) in zip(ops_ab, outs, SHAPES)]
    if row_map is None:
        K.gemm_tn_grouped(probs)
    else:
        K.gemm_tn_grouped_mapped(probs, row_map, count)
    torch.cuda.synchronize()
    return outs


def _equal(x, y):
    return all(torch.equal(c0, c1) and torch.equal(b0, b1) for (c0, b0), (c1, b1) in zip(x, y))


@pytest.mark.parametrize("beta", [0, 1])
@pytest.mark.parametrize("rows", [M, 384])
def test_identity_map_gives_the_bits_of_the_unmapped_launch(rows, beta):
    ops, _ = _operands()
    ab = [(a, b) for a, b, _, _ in ops]
    starts = [(c, bias) for _, _, c, bias in ops]
    ident = torch.arange(M, dtype=torch.int32, device=DEV)
    assert _equal(_run(ab, starts, ident, _i32([rows]), beta, rows), _run(ab, starts, None, None, beta, rows))


@pytest.mark.parametrize("beta", [0, 1])
@pytest.mark.parametrize("count", COUNTS)
def test_mapped_rows_only_and_accuracy(count, beta):
    """Checks 2 and 3 on one set of launches."""
    ops, kept = _operands()
    rows = kept[:count].long()
    row_map, cnt = _padded_map(kept[:count]), _i32([count])
    dropped = torch.ones(M, dtype=torch.bool, device=DEV)
    dropped[rows] = False
    zeroed, poisoned = [], []
    for a, b, _, _ in ops:
        a0, b0, a1, b1 = a.clone(), b.clone(), a.clone(), b.clone()
        a0[dropped], b0[dropped] = 0, 0
        a1[dropped], b1[dropped] = float("nan"), float("nan")
        zeroed.append((a0, b0))
        poisoned.append((a1, b1))
    # beta = 1 accumulates onto the beta = 0 result, as test_00's grouped case does (then the sum is 2 x the product)
    zero_start = [(torch.zeros_like(c), torch.zeros_like(bias)) for _, _, c, bias in ops]
    first = _run(zeroed, zero_start, row_map, cnt, 0)
    starts = first if (beta and count) else [(c, bias) for _, _, c, bias in ops]
    got0 = _run(zeroed, starts, row_map, cnt, beta)
    got1 = _run(poisoned, starts, row_map, cnt, beta)
    for (c, bias) in got1:
        assert bool(torch.isfinite(c).all()) and bool(torch.isfinite(bias).all())
    assert _equal(got0, got1)
    if count == 0 and beta:
        assert _equal(got0, starts)          # nothing to add: C and the bias gradient (random start values) stay as they were
        return
    for (a, b, _, _), (c, bias) in zip(ops, got0):
        ref = (a[rows].double().t() @ b[rows].double()) * (2 if beta else 1)
        col = a[rows].double().sum(0) * (2 if beta else 1)
        e = rel(c.float(), ref)
        eb = float((bias.double() - col).abs().max())
        print("M' = %d beta = %d N = %d K = %d: rel %.2e, bias error %.2e (column sums up to %.2f)" % (count, beta, c.shape[0], c.shape[1], e, eb, float(col.abs().max())))
        assert e < (2.5e-3 if beta else 1.5e-3)
        assert eb < 2e-3 * float(col.abs().max()) + 1e-2


def test_map_entries_and_count_are_clamped():
    """Entries below 0 / above M - 1 and a count above M are clamped to valid rows: the run completes and equals the run with the clamped values."""
    ops, _ = _operands()
    ab = [(a, b) for a, b, _, _ in ops]
    starts = [(c, bias) for _, _, c, bias in ops]
    gen = torch.Generator().manual_seed(5)
    good = torch.randint(0, M, (M,), generator=gen, dtype=torch.int32)
    bad = good.clone()
    bad[3], bad[64], bad[200], bad[M - 1] = M + 1000, -7, 2 ** 31 - 1, -2 ** 31
    good[3], good[64], good[200], good[M - 1] = M - 1, 0, M - 1, 0
    want = _run(ab, starts, good.to(DEV), _i32([M]), 0)
    assert _equal(_run(ab, starts, bad.to(DEV), _i32([M + 50]), 0), want)
    assert _equal(_run(ab, starts, bad.to(DEV), _i32([2 ** 31 - 1]), 0), want)
    zero = _run(ab, starts, good.to(DEV), _i32([0]), 0)
    assert _equal(_run(ab, starts, bad.to(DEV), _i32([-5]), 0), zero)
    assert all(float(c.abs().max()) == 0.0 and float(bias.abs().max()) == 0.0 for c, bias in zero)


# ---- vlp_kept_rows_build ----------------------------------------------------------------------------------------------------------------
def _host_rule(attended_end, masked_pos, L, Nv):
    """Engine._kept_lengths, restated: 1 + the last attended key column, at least Nv + 2, at least max(masked_pos) + 1 (clamped to L)."""
    lens = []
    for b, n in enumerate(attended_end):
        n = max(int(n), Nv + 2)
        if masked_pos is not None:
            n = max(n, min(int(masked_pos[b].max()) + 1, L))
        lens.append(min(n, L))
    return lens


def _build_and_check(B, L, Nv, want, **kw):
    lens = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    row_map = torch.full((B * L,), -1, dtype=torch.int32, device=DEV)
    count = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    K.kept_rows_build(B, L, Nv, lens, row_map, count, **kw)
    torch.cuda.synchronize()
    assert lens.tolist() == want
    rows = [b * L + l for b, n in enumerate(want) for l in range(n)]
    assert int(count) == len(rows)
    assert row_map[:len(rows)].tolist() == rows
    assert bool((row_map[len(rows):] == B * L - 1).all())


@pytest.mark.parametrize("L,Nv", [(35, 8), (167, 100), (64, 8)])
def test_kept_rows_build_against_the_host_rule(L, Nv):
    B = 7
    gen = torch.Generator().manual_seed(L)
    n_b = torch.randint(1, L - Nv - 3 + 1, (B,), generator=gen).tolist()
    n_b[0], n_b[1] = L - Nv - 3, 1                           # a full sample, a shortest one
    modes = ["s2s" if i % 2 == 0 else "bi" for i in range(B)]
    mask = torch.stack([S.build_attention_mask(L, Nv, n, m) for n, m in zip(n_b, modes)])
    mask[2] = 0                                              # nothing attended at all: Nv + 2 rows stay
    end = [int(m.any(dim=0).nonzero().max()) + 1 if bool(m.any()) else 0 for m in mask]
    pos = torch.stack([torch.randint(Nv + 2, e if e > Nv + 2 else Nv + 3, (3,), generator=gen) for e in end])
    pos[1, 2] = L - 1                                        # a masked position past the sample's last attended key
    pos[3, 0] = L + 5                                        # out of range: the gather clamps it to L - 1
    Lp = (L + 31) // 32 * 32
    maskb = torch.empty(B, L, Lp, dtype=torch.uint8, device=DEV)
    K.mask_pack(mask.to(DEV), maskb, B, L, Lp)
    _build_and_check(B, L, Nv, _host_rule(end, pos, L, Nv), maskb=maskb, Lp=Lp, pos=pos.to(DEV))
    _build_and_check(B, L, Nv, _host_rule(end, None, L, Nv), maskb=maskb, Lp=Lp)
    # MaskSpec: the lengths come from its device array (second_end), the mask bytes are not read
    spec = MaskSpec.from_lengths(Nv, n_b, [m == "s2s" for m in modes], device=DEV)
    assert spec.lens_host == [Nv + n + 3 for n in n_b]
    _build_and_check(B, L, Nv, _host_rule(spec.lens_host, pos, L, Nv), lens_in=spec.second_end, pos=pos.to(DEV))
    _build_and_check(B, L, Nv, _host_rule(spec.lens_host, None, L, Nv), lens_in=spec.second_end)


# ---- engine -----------------------------------------------------------------------------------------------------------------------------
V, NV, BE, LE = 1024, 8, 64, 35


@functools.lru_cache(maxsize=None)
def _template():
    p = O.init_params(vocab_size=V, layers=2, tasks="img2txt", seed=9)
    cfg = BertConfig(V, num_hidden_layers=2, type_vocab_size=6, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1)
    m = BertForPreTrainingLossMask(cfg, enable_butd=True, len_vis_input=NV, tasks="img2txt", allow_random_fc7=True)
    sd = dict(p)
    sd["cls.predictions.decoder.weight"] = p["bert.embeddings.word_embeddings.weight"]
    m.load_state_dict(sd, strict=True)
    return m.half().to(DEV).train()


def _new():
    m = copy.deepcopy(_template())
    m.engine.pack()
    return m


@functools.lru_cache(maxsize=None)
def _batch(seed, max_len_b=LE - NV - 3, min_len_b=2):
    raw = S.make_batch(BE, max_len_b=max_len_b, len_vis_input=NV, vocab_size=V, max_pred=3, s2s_prob=0.75, seed=seed, min_len_b=min_len_b)
    L = raw.input_ids.shape[1]
    if L < LE:      # shorter samples inside the same L = 35 (the workspace key stays, the kept lengths change)
        pad = torch.nn.functional.pad
        e = LE - L
        raw = raw._replace(input_ids=pad(raw.input_ids, (0, e)), segment_ids=pad(raw.segment_ids, (0, e)), input_mask=pad(raw.input_mask, (0, e, 0, e)))
    return raw, S.batch_to(raw, DEV, half=True)


def _kept_rows(raw):
    end = [int(m.any(dim=0).nonzero().max()) + 1 for m in raw.input_mask]
    return sum(_host_rule(end, raw.masked_pos, LE, NV))


def _step(model, b, seed, varlen=False):
    eng = model.engine
    eng.varlen = varlen
    eng.zero_grad()
    eng.step_seed = seed
    lt = model(b.img, b.vis_pe, b.input_ids, b.segment_ids, b.input_mask, b.lm_label_ids, b.ans_labels, b.is_next, masked_pos=b.masked_pos,
               masked_weights=b.masked_weights, task_idx=b.task_idx, vis_masked_pos=b.vis_masked_pos, mask_image_regions=False, drop_worst_ratio=0)
    ((lt[0] + lt[1] + lt[2]) * 1024.0).backward()
    torch.cuda.synchronize()
    out = collections.OrderedDict()
    for i, x in enumerate(lt):
        out["loss[%d]" % i] = x.detach().clone()
    out["logits"] = model.last_mlm_logits.clone()
    for n, q in model.named_parameters():
        out["grad " + n] = q.grad.detach().clone()
    return out


def _not_grads(d):
    return collections.OrderedDict((k, v) for k, v in d.items() if not k.startswith("grad "))


def test_dense_step_switch_on_against_off(monkeypatch):
    raw, b = _batch(31)
    assert BE * LE >= 2048 and _kept_rows(raw) < BE * LE
    res = {}
    for sw in ("1", "0"):
        monkeypatch.setenv("VLP_WGRAD_KEPT", sw)
        model = _new()
        res[sw] = _step(model, b, 77)
        assert model.engine.last_wgrad_mapped == (sw == "1")
        assert model.engine.last_packed_rows is None
        if sw == "1":
            assert int(model.engine._workspace(BE, LE, 3)["kept_n"]) == _kept_rows(raw)
    assert first_difference(_not_grads(res["1"]), _not_grads(res["0"])) is None      # the forward is untouched
    worst = ("", 0.0)
    for n in res["0"]:
        if not n.startswith("grad "):
            continue
        g0, g1 = res["0"][n].float(), res["1"][n].float()
        d, ref = float((g0 - g1).norm()), float(g0.norm())
        r = d / ref if ref > 0 else d
        if r > worst[1]:
            worst = (n, r)
        assert r <= 2e-4, (n, r)            # test_25's bound for dense against packed gradients
    print("mapped vs unmapped dense step: worst gradient tensor %s rel-L2 %.2e" % worst)


def test_three_steps_of_different_kept_lengths_equal_a_fresh_engine(monkeypatch):
    monkeypatch.setenv("VLP_WGRAD_KEPT", "1")
    batches = [_batch(41), _batch(42, max_len_b=9), _batch(43, max_len_b=17, min_len_b=12)]
    assert len({_kept_rows(raw) for raw, _ in batches}) == 3
    used = _new()
    for i, (raw, b) in enumerate(batches):
        got = _step(used, b, 500 + i)
        assert used.engine.last_wgrad_mapped
        assert int(used.engine._workspace(BE, LE, 3)["kept_n"]) == _kept_rows(raw)
        fresh = _new()
        want = _step(fresh, b, 500 + i)
        d = first_difference(got, want)
        assert d is None, "step %d: the used engine differs from a fresh one -- %s" % (i, d)


def test_packed_step_does_not_change_with_the_switch(monkeypatch):
    raw, b = _batch(31)
    res = []
    for sw in ("1", "0"):
        monkeypatch.setenv("VLP_WGRAD_KEPT", sw)
        model = _new()
        res.append(_step(model, b, 77, varlen=True))
        assert model.engine.last_packed_rows is not None and not model.engine.last_wgrad_mapped
    assert first_difference(res[0], res[1]) is None
