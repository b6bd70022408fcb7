"""CPU: the multi-reference SCST reward's host side -- self_critical_reward_refs against CiderD, the loader's CaptionRefs
(BatchPrefetcher(caption_refs=R)) against a restatement of its format rule, and the entry script's --scst_reward / --scst_refs plumbing
(scst_step with the defaults still calls self_critical_reward exactly as before).  The device kernel's twin is tests/test_81_scst_reward_gpu.py."""
from collections import OrderedDict

import numpy as np
import pytest
import torch

from vlp_amd import scst as SC
from vlp_amd.data import BatchPrefetcher, PackedRegionStore, TextPreprocessor, write_packed
from vlp_amd.input_prep import CaptionRefs


def _ids(rng, B, T, lo=1000, hi=1012):
    """[B, T] id rows: words, then 102 and zeros when shorter than T."""
    out = np.zeros((B, T), dtype=np.int64)
    for b in range(B):
        n = rng.randint(1, T + 1)
        out[b, :n] = rng.randint(lo, hi, size=n)
        if n < T:
            out[b, n - 1] = 102
    return out


def test_reward_refs_single_reference_is_self_critical_reward():
    rng = np.random.RandomState(0)
    B, T = 6, 9
    gen, greedy, gt = _ids(rng, B, T), _ids(rng, B, T), _ids(rng, B, T)
    gen[:3] = gt[:3]                                      # some non-zero scores
    r0, s0 = SC.self_critical_reward(greedy, gt, gen, B)
    for conv in (lambda x: x, torch.from_numpy):
        r1, s1 = SC.self_critical_reward_refs(conv(greedy), conv(gt), conv(gen))
        assert r1.shape == (B, T) and s1.shape == (2 * B,)
        assert np.array_equal(r0, r1) and np.array_equal(s0, s1)
    assert np.count_nonzero(s0) >= 3


def test_reward_refs_caption_refs_is_cider_d_on_the_strings():
    rng = np.random.RandomState(1)
    B, R, T = 5, 4, 9
    ids = np.stack([_ids(rng, B, T) for _ in range(R)], 1)
    count = np.array([1, 4, 2, 3, 4], dtype=np.int32)
    gen, greedy = _ids(rng, B, T), _ids(rng, B, T)
    for b in range(B):
        gen[b] = ids[b, count[b] - 1]                     # the sample equals its last VALID reference
        greedy[b, :2] = ids[b, 0, :2]
    ids[0, 1:] = gen[1]                                   # invalid rows (r >= count) hold another sample's words: they must not count
    refs = CaptionRefs(torch.from_numpy(ids), torch.from_numpy(count))
    reward, scores = SC.self_critical_reward_refs(torch.from_numpy(greedy), refs, torch.from_numpy(gen))
    gts, res = OrderedDict(), OrderedDict()
    for i in range(2 * B):
        b = i % B
        res[i] = [SC.array_to_str((gen if i < B else greedy)[b].tolist())]
        gts[i] = [SC.array_to_str(ids[b, r].tolist()) for r in range(count[b])]
    _, want = SC.CiderD(df="corpus").compute_score(gts, res)
    assert np.array_equal(scores, want)
    assert np.array_equal(reward, np.repeat((want[:B] - want[B:])[:, None], T, 1))
    assert np.count_nonzero(want[:B]) >= 3 and np.count_nonzero(reward[:, 0]) >= 3 and reward.shape == (B, T)      # not a comparison of zeros


def test_caption_refs_check_and_to():
    refs = CaptionRefs(torch.zeros(3, 5, 7, dtype=torch.long), torch.ones(3, dtype=torch.int32))
    refs.check(3, 7)
    assert refs.shape == (3, 5, 7) and isinstance(refs.to("cpu"), CaptionRefs)
    for bad in (CaptionRefs(refs.ids.int(), refs.count), CaptionRefs(refs.ids, refs.count.long()), CaptionRefs(refs.ids[:2], refs.count),
                CaptionRefs(torch.zeros(3, 9, 7, dtype=torch.long), refs.count)):
        with pytest.raises(RuntimeError):
            bad.check(3, 7)
    with pytest.raises(RuntimeError):
        refs.check(3, 8)


# ---- loader -------------------------------------------------------------------------------------------------------------------------
NV, MAX_LEN_B, SEP = 4, 6, 102


def _caption_store(tmp_path):
    """7 images with 1..7 captions each (lengths 1..11: some longer than max_len_b), the captions of an image scattered over the list."""
    rng = np.random.RandomState(3)
    n = 7
    ids = ["img%d" % i for i in range(n)]
    write_packed(str(tmp_path), ids, np.abs(rng.standard_normal((n, NV, 2048))).astype(np.float16), rng.rand(n, NV, 1601).astype(np.float16),
                 rng.rand(n, NV, 6).astype(np.float32))
    examples = [(ids[i], rng.randint(200, 900, size=rng.randint(1, 12)).tolist()) for i in range(n) for _ in range(i + 1)]
    order = rng.permutation(len(examples))
    examples = [examples[j] for j in order]
    assert sorted(sum(1 for e in examples if e[0] == k) for k in ids) == [1, 2, 3, 4, 5, 6, 7]
    assert any(len(e[1]) > MAX_LEN_B for e in examples) and any(len(e[1]) < MAX_LEN_B for e in examples)
    return PackedRegionStore(str(tmp_path)), examples


def _procs():
    kw = dict(max_pred=3, mask_prob=0.15, vocab_size=1000, cls_id=101, sep_id=SEP, mask_id=103, unk_id=100, max_len=NV + MAX_LEN_B + 3, max_len_b=MAX_LEN_B,
              len_vis_input=NV)
    return TextPreprocessor(mode="s2s", **kw), TextPreprocessor(mode="bi", **kw)


def _flat(x):
    if torch.is_tensor(x):
        return [x.clone()]
    return [t.clone() if torch.is_tensor(t) else t for t in x]


def _epochs(store, examples, caption_refs, workers):
    p_s2s, p_bi = _procs()
    pf = BatchPrefetcher(store, examples, 4, p_s2s, p_bi, s2s_prob=0.7, device="cpu", seed=9, num_workers=workers, caption_refs=caption_refs)
    out = []
    for epoch in range(2):
        pf.set_epoch(epoch)
        order = pf.epoch_order()
        for step, b in enumerate(pf):
            out.append(([_flat(x) for x in b[:11]], _flat(b[11]), type(b[11]), pf.step_examples(order, step)))
    return out


def test_loader_caption_refs(tmp_path):
    store, examples = _caption_store(tmp_path)
    plain = _epochs(store, examples, 0, 1)
    with5 = _epochs(store, examples, 5, 1)
    assert len(plain) == len(with5) == 2 * 7                          # 28 examples, batch 4, two epochs
    T = MAX_LEN_B + 1
    seen7 = False
    for (a, a12, ta, _), (b, b12, tb, exs) in zip(plain, with5):
        # every other field of every batch: bit for bit what caption_refs=0 gives
        for x, y in zip(a, b):
            assert len(x) == len(y)
            for u, v in zip(x, y):
                assert (torch.equal(u, v) and u.dtype == v.dtype) if torch.is_tensor(u) else u == v
        assert ta is torch.Tensor and tuple(a12[0].shape) == (4, 1)
        assert tb is CaptionRefs
        ids, count = b12
        assert ids.dtype == torch.int64 and tuple(ids.shape) == (4, 5, T) and count.dtype == torch.int32 and tuple(count.shape) == (4,)
        for j, ex in enumerate(exs):
            caps = [e[1] for e in examples if e[0] == ex[0]]          # the image's captions in order of first appearance
            want = [(c[:MAX_LEN_B] + [SEP] + [0] * T)[:T] for c in caps[:5]]
            assert int(count[j]) == min(len(caps), 5)
            assert ids[j, :len(want)].tolist() == want
            assert not bool(ids[j, len(want):].any())
            if len(caps) == 7:
                seen7 = True
                assert int(count[j]) == 5 and ids[j].tolist() == [(c[:MAX_LEN_B] + [SEP] + [0] * T)[:T] for c in caps[:5]]
            # a full-length caption ends in [SEP] in the last column, with no 0 behind it
            for c, row in zip(caps[:5], ids[j].tolist()):
                if len(c) >= MAX_LEN_B:
                    assert row[-1] == SEP and 0 not in row
    assert seen7
    # the same for 1 and 3 workers
    three = _epochs(store, examples, 5, 3)
    for (a, a12, _, _), (b, b12, _, _) in zip(with5, three):
        for x, y in zip(a + [a12], b + [b12]):
            for u, v in zip(x, y):
                assert torch.equal(u, v) if torch.is_tensor(u) else u == v


def test_loader_caption_refs_refuses_vqa_examples_and_bad_counts(tmp_path):
    store, examples = _caption_store(tmp_path)
    p_s2s, p_bi = _procs()
    vqa = [(e[0], e[1], [1, 2], 7) for e in examples]
    with pytest.raises(ValueError):
        BatchPrefetcher(store, vqa, 4, p_s2s, p_bi, device="cpu", caption_refs=5)
    with pytest.raises(ValueError):
        BatchPrefetcher(store, examples, 4, p_s2s, p_bi, device="cpu", caption_refs=9)


# ---- entry script -------------------------------------------------------------------------------------------------------------------
def test_parser_defaults_and_refusals():
    from vlp_amd import run_img2txt_dist as R
    base = ["--enable_butd", "--fp16"]
    args = R.derive_args(R.build_parser().parse_args(base))
    assert args.scst_reward == "host" and args.scst_refs == "caption"
    with pytest.raises(ValueError):
        R.derive_args(R.build_parser().parse_args(base + ["--scst_refs", "image", "--packed_features", "x"]))          # no --scst
    scst = base + ["--scst", "--max_pred", "0", "--mask_prob", "0"]
    with pytest.raises(ValueError):
        R.derive_args(R.build_parser().parse_args(scst + ["--scst_refs", "image"]))                                    # no --packed_features
    args = R.derive_args(R.build_parser().parse_args(scst + ["--scst_refs", "image", "--packed_features", "x", "--scst_reward", "device"]))
    assert args.scst_reward == "device" and args.scst_refs == "image"
    with pytest.raises(SystemExit):
        R.build_parser().parse_args(base + ["--scst_reward", "gpu"])


class _Model(object):
    def __init__(self, B, T):
        self.B, self.T, self.calls = B, T, []

    def eval(self):
        self.calls.append("eval")

    def train(self):
        self.calls.append("train")

    def __call__(self, img, vis_pe, input_dummy, segment_ids, position_ids, input_mask, task_idx=None, sample_mode=None):
        self.calls.append(sample_mode)
        g = torch.Generator().manual_seed(1 if sample_mode == "greedy" else 2)
        ids = torch.randint(1000, 1010, (self.B, self.T), generator=g)
        ids[:, -2] = 102
        return ids, torch.zeros(self.B, self.T, requires_grad=True)


class _Opt(object):
    def __init__(self):
        self.param_groups, self.calls = [{"lr": 0.0}], []

    def backward(self, loss):
        self.calls.append("backward")

    def step(self):
        self.calls.append("step")

    def zero_grad(self):
        self.calls.append("zero_grad")


def _stub_batch(B, Nv, T, refs=None):
    L = Nv + 2 + T
    input_ids = torch.randint(1000, 1010, (B, L), generator=torch.Generator().manual_seed(0))
    z = torch.zeros(B, L, dtype=torch.long)
    ans = refs if refs is not None else torch.zeros(B, 1)
    return (input_ids, z, torch.ones(B, L, L, dtype=torch.long), z, z, z, z, torch.zeros(B, dtype=torch.long), torch.zeros(B, Nv, 8), z,
            torch.zeros(B, Nv, 8), ans)


def _spies(monkeypatch, B, T):
    calls = []

    def host(*a, **kw):
        calls.append(("host", a, kw))
        return np.full((B, T), 0.25), np.zeros(2 * B)

    def refs(*a, **kw):
        calls.append(("refs", a, kw))
        return np.full((B, T), 0.5), np.zeros(2 * B)

    def device(*a, **kw):
        calls.append(("device", a, kw))
        return torch.full((B, T), 0.75), torch.zeros(2 * B)
    monkeypatch.setattr(SC, "self_critical_reward", host)
    monkeypatch.setattr(SC, "self_critical_reward_refs", refs)
    monkeypatch.setattr(SC, "self_critical_reward_device", device)
    return calls


def test_scst_step_default_calls_self_critical_reward_as_before(monkeypatch):
    from vlp_amd import run_img2txt_dist as R
    B, Nv, T = 3, 4, 6
    calls = _spies(monkeypatch, B, T)
    batch = _stub_batch(B, Nv, T)
    seen = {}

    def crit(logp, seq, reward):
        seen["reward"], seen["seq"] = reward, seq
        return logp.sum()
    marks = []
    model, opt = _Model(B, T), _Opt()
    loss, mean_r = R.scst_step(model, opt, batch, 1e-5, Nv, crit, mark=marks.append)
    assert [c[0] for c in calls] == ["host"]
    _, a, kw = calls[0]
    assert kw == {} and len(a) == 4 and a[3] == B                     # (greedy_res, gt_ids, gen_result, batch_size), positionally
    greedy_raw, gen_raw = model(None, None, None, None, None, None, sample_mode="greedy")[0], model(None, None, None, None, None, None, sample_mode="sample")[0]
    assert torch.equal(a[0], SC.clean_captions(greedy_raw, 102, 0)) and torch.equal(a[2], SC.clean_captions(gen_raw, 102, 0))
    assert torch.equal(a[1], batch[0][:, Nv + 2:])
    assert seen["reward"].dtype == torch.float32 and torch.equal(seen["reward"], torch.full((B, T), 0.25))
    assert torch.equal(seen["seq"], a[2]) and float(mean_r) == 0.25
    assert marks == ["greedy_decode", "sample_forward", "reward_host", "backward", "optimizer"]
    assert opt.calls == ["backward", "step", "zero_grad"] and opt.param_groups[0]["lr"] == 1e-5


def test_scst_step_routes_device_and_image_references(monkeypatch):
    from vlp_amd import run_img2txt_dist as R
    B, Nv, T = 3, 4, 6
    refs = CaptionRefs(torch.zeros(B, 5, T, dtype=torch.long), torch.ones(B, dtype=torch.int32))

    def crit(logp, seq, reward):
        return logp.sum() * reward.mean()
    for reward_on, with_refs, who, phase, value in (("device", False, "device", "reward_device", 0.75), ("device", True, "device", "reward_device", 0.75),
                                                    ("host", True, "refs", "reward_host", 0.5)):
        calls = _spies(monkeypatch, B, T)
        batch = _stub_batch(B, Nv, T, refs if with_refs else None)
        marks = []
        _, mean_r = R.scst_step(_Model(B, T), _Opt(), batch, 1e-5, Nv, crit, mark=marks.append, reward_on=reward_on)
        assert [c[0] for c in calls] == [who] and float(mean_r) == value
        _, a, kw = calls[0]
        assert len(a) == 3 and kw == {}
        assert (a[1] is refs) if with_refs else torch.equal(a[1], batch[0][:, Nv + 2:])
        assert marks[2] == phase and len(marks) == 5
