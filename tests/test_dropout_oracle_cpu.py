"""CPU: the dropout-on step check (tests/test_15_dropout_step_gpu.py) discriminates -- each slip it exists to catch moves some parameter
gradient by at least 5x the bound the GPU test applies to that tensor.

The hooked oracle (fp32, 2 layers, Nv = 8, B = 2, L = 20, vocab 1024) with the correct masks of tests/dropout_ref.step_masks is the truth;
the same oracle under a MUTATED mask set stands for an engine with that slip.  The bound of every tensor is computed exactly as on the
GPU: dropout_ref.grad_tensor_bound with the fp16 oracle's own error on this batch as the yardstick.  The 5x is a condition: a mutant
below it would mean the GPU bound is too loose to mean anything.

Measured (largest ratio || g_mutant - g_truth || / bound over the parameters, and where):
    attn_out / ffn_out streams swapped (16i+2 <-> 16i+3)      14.2   bert.encoder.layer.0.output.dense.weight
    vis / vispe streams swapped (1001 <-> 1002)                7.5   vis_embed.0.weight
    attention stream of layer i+1                              7.1   bert.encoder.layer.1.attention.output.dense.weight
    seed + 1                                                  20.3   bert.encoder.layer.1.intermediate.dense.weight
    attention mask transposed (query, key)                     7.1   bert.encoder.layer.1.attention.output.dense.weight
    kept multiplier 1 in place of 1/(1-p)                      5.3   vis_embed.2.weight
    "emb" mask left out                                       13.0   cls.predictions.transform.dense.weight
    FFN-down wgrad reads the undropped gradient (hand-built)   9.0   bert.encoder.layer.1.output.dense.weight
One more, beyond the list above: the kept multiplier 1 at the FFN-out sites ONLY (the smallest form of a missing 1/(1-p)) reaches 2.9
(bert.encoder.layer.0.intermediate.dense.weight).  It does not have the 5x margin; it is held to 2x, which still guarantees that the GPU
test fails: an engine whose own error is within the bound, shifted by >= 2 bounds, is outside the bound (triangle inequality)."""
import pytest
import torch
import torch.nn.functional as F

from oracle import vlp_oracle as O
from tests.dropout_ref import drop_mult_ref, grad_tensor_bound, site_table, step_masks, stream_attn
from vlp_amd import synthetic as S

LAYERS, NV, B, HID, HEADS, P, SEED, GS = 2, 8, 2, 768, 12, 0.1, 0x5EED + 7, 128.0
_cache = {}


def _setup():
    if not _cache:
        p = O.init_params(vocab_size=1024, layers=LAYERS, seed=31)
        batch = S.make_batch(B, max_len_b=9, len_vis_input=NV, vocab_size=1024, max_pred=3, s2s_prob=0.5, seed=32, min_len_b=3)
        L = batch.input_ids.shape[1]
        masks = step_masks(SEED, P, P, B, L, NV, HID, HEADS, LAYERS)
        truth = _grads(p, batch, masks, torch.float32)
        yard = _grads(p, batch, masks, torch.float16)
        gscale = max(float(g.norm()) for g in truth.values() if g is not None)
        bound = {n: grad_tensor_bound(float(g.norm()), g.numel(), gscale, float((yard[n] - g).norm())) for n, g in truth.items() if g is not None}
        _cache.update(p=p, batch=batch, L=L, masks=masks, truth=truth, bound=bound)
    return _cache


def _grads(p, batch, masks, dtype):
    pd = {k: v.to(dtype).clone().requires_grad_(True) for k, v in p.items()}
    out = O.forward_pretraining_loss_mask(pd, batch, tasks="img2txt", len_vis_input=NV, dropout=masks)
    (out["loss"].sum() * GS).backward()
    return {k: (None if t.grad is None else t.grad.float() / GS) for k, t in pd.items()}


def _worst_ratio(c, grads):
    worst = ("", 0.0)
    for n, b in c["bound"].items():
        r = float((grads[n] - c["truth"][n]).norm()) / b
        if r > worst[1]:
            worst = (n, r)
    return worst


def _swap(m, a, b):
    m = dict(m)
    m[a], m[b] = m[b], m[a]
    return m


def _mut_swap_out_streams(c):
    m = dict(c["masks"])
    for i in range(LAYERS):
        m = _swap(m, ("attn_out", i), ("ffn_out", i))
    return m


def _mut_attn_next_layer(c):
    m = dict(c["masks"])
    for i in range(LAYERS):
        m[("attn", i)] = drop_mult_ref(P, SEED, stream_attn(i + 1), range(B * HEADS * c["L"]), range(c["L"]), "cpu").view(B, HEADS, c["L"], c["L"])
    return m


def _mut_attn_transposed(c):
    m = dict(c["masks"])
    for i in range(LAYERS):
        m[("attn", i)] = m[("attn", i)].transpose(-1, -2).contiguous()
    return m


def _mut_no_rescale(c, sites):
    return {s: ((t > 0).float() if sites(s) else t) for s, t in c["masks"].items()}


MUTANTS = {
    "out_streams_swapped": _mut_swap_out_streams,
    "vis_vispe_swapped": lambda c: _swap(c["masks"], "vis", "vispe"),
    "attn_stream_of_next_layer": _mut_attn_next_layer,
    "seed_plus_1": lambda c: step_masks(SEED + 1, P, P, B, c["L"], NV, HID, HEADS, LAYERS),
    "attn_mask_transposed": _mut_attn_transposed,
    "no_rescale": lambda c: _mut_no_rescale(c, lambda s: True),
    "emb_mask_left_out": lambda c: {s: t for s, t in c["masks"].items() if s != "emb"},
}


def test_site_table_is_the_contract():
    """The table the tests build masks from: stream ids and shapes as DESIGN.md states them."""
    t = {s[0]: s for s in site_table(3, 20, 8, HID, HEADS, 2)}
    assert (t["vis"][1], t["vispe"][1], t["emb"][1]) == (1001, 1002, 1000)
    assert [t[(k, i)][1] for i in range(2) for k in ("attn", "attn_out", "ffn_out")] == [1, 2, 3, 17, 18, 19]
    assert t["vis"][4] == (24, HID) and t["emb"][4] == (60, HID) and t[("attn", 1)][4] == (3, HEADS, 20, 20) and t[("attn", 1)][2:4] == (3 * HEADS * 20, 20)
    m = step_masks(5, 0.1, 0.3, 3, 20, 8, HID, HEADS, 2)
    assert set(m) == set(t) and all(tuple(m[s].shape) == t[s][4] for s in t)
    assert set(m["emb"].unique().tolist()) == {0.0, float(torch.tensor(1.0 / 0.9))}
    assert abs(float((m["emb"] == 0).float().mean()) - 0.1) < 0.01 and abs(float((m[("attn", 0)] == 0).float().mean()) - 0.3) < 0.01


def test_correct_masks_reproduce_and_matter():
    c = _setup()
    again = _grads(c["p"], c["batch"], c["masks"], torch.float32)
    assert _worst_ratio(c, again)[1] == 0.0
    plain = _grads(c["p"], c["batch"], None, torch.float32)
    assert _worst_ratio(c, plain)[1] >= 5.0


@pytest.mark.parametrize("name", list(MUTANTS))
def test_mutant_moves_a_gradient_by_5x_the_gpu_bound(name):
    c = _setup()
    n, r = _worst_ratio(c, _grads(c["p"], c["batch"], MUTANTS[name](c), torch.float32))
    print("%s: %.1f x the bound on %s" % (name, r, n))
    assert r >= 5.0, (name, n, r)


def test_missing_rescale_at_one_site_class_is_still_outside_the_bound():
    """The smallest missing-1/(1-p) slip: the FFN-out sites only.  Held to 2x, not 5x (see the module docstring)."""
    c = _setup()
    m = _mut_no_rescale(c, lambda s: isinstance(s, tuple) and s[0] == "ffn_out")
    n, r = _worst_ratio(c, _grads(c["p"], c["batch"], m, torch.float32))
    print("no_rescale_ffn_out: %.1f x the bound on %s" % (r, n))
    assert r >= 2.0, (n, r)


class _UndroppedToWeight(torch.autograd.Function):
    """y = t * m, but the gradient reaching the weight's copy of t is the UNDROPPED one: what a wgrad GEMM computes when it is handed the
    LayerNorm gradient before the dropout mask (the engine's `dpre`) in place of the masked one (`dy2`)."""

    @staticmethod
    def forward(ctx, t_for_x, t_for_w, m):
        ctx.save_for_backward(m)
        return t_for_x * m

    @staticmethod
    def backward(ctx, g):
        m, = ctx.saved_tensors
        return g * m, g, None


def test_wgrad_fed_the_undropped_gradient_is_seen(monkeypatch):
    c = _setup()
    plain = O.linear_add

    def leaky(x, w, b, res, drop=None):
        if drop is None or w.shape[1] != 3072:                 # the FFN-down projection of every layer
            return plain(x, w, b, res, drop=drop)
        t_for_x, t_for_w = F.linear(x, w.detach(), b.detach()), F.linear(x.detach(), w, b)
        return _UndroppedToWeight.apply(t_for_x, t_for_w, drop.view(t_for_x.shape)) + res
    monkeypatch.setattr(O, "linear_add", leaky)
    g = _grads(c["p"], c["batch"], c["masks"], torch.float32)
    monkeypatch.undo()
    n, r = _worst_ratio(c, g)
    print("ffn_down_wgrad_undropped: %.1f x the bound on %s" % (r, n))
    assert n.endswith("output.dense.weight") or n.endswith("output.dense.bias")
    assert r >= 5.0, (n, r)
    # only that projection's weight / bias moved: the dgrad path was left alone
    for k, b in c["bound"].items():
        if "output.dense" not in k or "attention" in k:
            assert float((g[k] - c["truth"][k]).norm()) <= 1e-6 * b, k
