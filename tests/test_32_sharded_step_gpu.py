"""GPU: the sharded optimizer step (VLP_DDP_MODE=sharded) at world 8, every rank's kernels checked.

W ranks are emulated in ONE process (tests/shard_util.py: no process group, no subprocess).  Rank r is a packed small_model() of
test_30 (2 layers, vocab 1024: decay 23 521 024 + nodecay 29 184 elements in five ready-slices) with its own FP16_Optimizer_State and a
ShardPlan whose three collectives are in-process stand-ins; what runs on every rank is the PRODUCT method
FP16_Optimizer_State._step_sharded with the product kernels (vlp_sumsq / vlp_sumsq_acc / vlp_adam_hyper / vlp_fused_adam /
vlp_loss_scale_update) on the element ranges that rank owns.  The bucket cap is 16 MB: three buckets, (slices 0+1), (slices 2+3), (slice 4)
-- at the default 50 MB the model is one bucket.

Every step writes ONE mean gradient G (random fp16, normal range) into all ranks' gradient buffers and then overwrites everything a rank
does not own with NaN: after a reduce-scatter those bytes are garbage "nobody reads", and a single read of them shows in every check.

  A  clip inactive   the state assembled from the owners' chunks is bit-equal to a replicated ninth model's opt.step() on G
  B  clip active     one clip factor on all ranks, right to fp64; assembled state bit-equal to ONE full-range vlp_fused_adam call with
                     that factor, and within the kernel-contract bounds of the fp64 restatement
  C  footprint       what a rank may touch, and that the NaN stays where it is
  D  overflow on one rank (or two): every rank skips and halves its scale
  E  checkpoint      consolidate() gathers once per step, state dicts equal over the ranks
  F  hand-off        the next forward / backward consumes engine._param_works; gradient accumulation is refused

Mutations of the product (and of the stand-ins) run against this module on a scratch copy; each fails the tests beside it:
  owned_chunk() shifted by 8 elements for the last rank              C (tiling); A[2], A[8], B, D, E (the 8 orphaned elements are nobody's)
  `accumulate=not first` -> `accumulate=False` in _step_sharded      B (sum of squares = the last bucket's alone); D[middle_bucket], D[two_ranks]
                                                                     (the flag of bucket 1 is overwritten by bucket 2's); A passes: clip inactive
  the torch.maximum of the two group flags dropped                   D[middle_bucket], D[tail], D[two_ranks] (the other group applies, no scale change)
  the result of exchange_norms ignored (a private copy exchanged)    B (every rank clips by its own chunks' norm); D x 3 (rank 5 alone skips)
  gather_state skipping the tail, in the stand-in                    E; tests/test_shard_util_cpu.py
  _gather_sharded_state handing no tail tensors to gather_state      E

Cost on one MI355X: 9 cases in 7.0 s, 2.6 s of it building the nine models once (module fixture); per case 0.03 - 0.9 s; 10.5 GB high-water mark.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from vlp_amd import _lib as K                                           # noqa: E402
from vlp_amd import synthetic as S                                      # noqa: E402
from vlp_amd.distributed import coalesce_buckets                        # noqa: E402
from vlp_amd.optimization_fp16 import FP16_Optimizer_State, FusedAdam   # noqa: E402

from tests.kernel_util import _adam_ref, rel                            # noqa: E402
from tests.shard_util import LocalGroup, LocalShardPlan, run_sharded_step                 # noqa: E402
from tests.test_30_train_gpu import DEV, fwd_bwd, groups_of, small_model                  # noqa: E402

W = 8
CAP = int(16.0 * 1024 * 1024 / 2)       # elements of fp16 in 16 MB
SCALE = 2.0 ** 10                       # loss scale (dynamic: it may halve, it does not grow within three steps)
LR = 1e-3
KEYS = ("decay", "nodecay")
STATE = ("master", "m", "v", "p16")


def bits(t):
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()])


def bit_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


class Rank(object):
    def __init__(self):
        self.model, _ = small_model()
        self.model.train()
        self.opt = FP16_Optimizer_State(FusedAdam(groups_of(self.model), lr=LR, bias_correction=False, max_grad_norm=1.0), dynamic_loss_scale=True,
                                        dynamic_loss_args={"init_scale": SCALE}, verbose=False)
        self.opt.pipeline_with_forward = False
        self.eng = self.model.engine

    def idx(self, key):
        return self.opt._group_key.index(key)

    def buf(self, what, key):
        o, i = self.opt, self.idx(key)
        return {"master": o.fp32_groups_flat, "m": o._m, "v": o._v}[what][i] if what != "p16" else self.eng.flat[key]

    def snapshot(self):
        o = self.opt
        return {"buf": {(w, k): self.buf(w, k).clone() for w in STATE for k in KEYS},
                "small": [t.clone() for t in [o._scale_state, o._ovf] + o._sumsq + o._hyper],
                "host": (o._steps_issued, o._state_gathered_at, self.eng._param_works)}

    def restore(self, snap):
        o = self.opt
        for (w, k), t in snap["buf"].items():
            self.buf(w, k).copy_(t)
        for dst, src in zip([o._scale_state, o._ovf] + o._sumsq + o._hyper, snap["small"]):
            dst.copy_(src)
        o._steps_issued, o._state_gathered_at, self.eng._param_works = snap["host"]


class World(object):
    def __init__(self):
        self.ranks = [Rank() for _ in range(W)]
        self.replica = Rank()
        self.base = self.ranks[0].snapshot()
        for r in self.ranks + [self.replica]:           # every rank starts from the same parameters (DDP's initial broadcast)
            for k in KEYS:
                assert bit_equal(r.eng.flat[k], self.base["buf"][("p16", k)])
        eng = self.ranks[0].eng
        self.sizes = {k: eng.gflat[k].numel() for k in KEYS}
        self.buckets, _ = coalesce_buckets(eng.buckets, CAP)
        # the layout this module is written for: three buckets, two of them coalesced from two ready-slices
        assert len(eng.buckets) == 5 and len(self.buckets) == 3, (eng.buckets, self.buckets)
        assert self.buckets[0] == (eng.buckets[0][0], eng.buckets[1][1]) and self.buckets[1] == (eng.buckets[2][0], eng.buckets[3][1])
        self.group, self.live = None, []

    def reset(self, world):
        """Fresh ranks 0..world-1 (and the replica): state copied back from the saved tensors, new plans, nothing in flight."""
        self.group = LocalGroup(world)
        self.live = self.ranks[:world]
        for i, r in enumerate(self.ranks + [self.replica]):
            r.restore(self.base)
            r.opt._steps_issued, r.opt._state_gathered_at, r.eng._param_works = 0, -1, None
            r.eng.zero_grad()
            r.eng.shard_plan = None
            if i < world:
                r.eng.shard_plan = LocalShardPlan(self.buckets, self.sizes["nodecay"], r.eng.buckets, world, i, self.group)
        return self.live

    def make_grad(self, seed, ratio):
        """One mean gradient per group, already times the loss scale: random fp16 whose true norm / max_grad_norm is about `ratio` in
        each group, no element below fp16's normal range (2^-14)."""
        gen = torch.Generator(device=DEV).manual_seed(seed)
        G = {}
        for k in KEYS:
            n = self.sizes[k]
            g = torch.randn(n, device=DEV, generator=gen) * (ratio * SCALE / n ** 0.5)
            g = torch.where(g.abs() < 2.0 ** -13, torch.full_like(g, 2.0 ** -13).copysign(g), g).half()
            assert bool(torch.isfinite(g).all()) and float(g.abs().min()) >= 2.0 ** -14
            G[k] = g
        return G

    def write_grads(self, G):
        for r in self.live:
            for k in KEYS:
                gf = r.eng.gflat[k]
                gf.fill_(float("nan"))
                for lo, hi in r.eng.shard_plan.owned(k):
                    gf[lo:hi].copy_(G[k][lo:hi])

    def step(self, G, after_rank=None):
        """One sharded step of all live ranks on G -> the ranks' pre-step snapshots."""
        self.write_grads(G)
        live = self.live
        return run_sharded_step(self.group, [r.opt.step for r in live], [r.snapshot for r in live], [r.restore for r in live], after_rank)

    def assemble(self, what, key):
        """The buffer as the OWNERS hold it: every element taken from the rank whose plan owns it; NaN where no rank does."""
        ref = self.live[0].buf(what, key)
        full = torch.full_like(ref, float("nan"))
        for r in self.live:
            for lo, hi in r.eng.shard_plan.owned(key):
                full[lo:hi].copy_(r.buf(what, key)[lo:hi])
        return full

    def assembled(self):
        return {(w, k): self.assemble(w, k) for w in ("master", "m", "v") for k in KEYS}


@pytest.fixture(scope="module")
def world():
    torch.cuda.reset_peak_memory_stats()
    w = World()
    yield w
    print("test_32: GPU memory high-water mark %.2f GB" % (torch.cuda.max_memory_allocated() / 2.0 ** 30))
    del w
    torch.cuda.empty_cache()


def hyper_of(rank, key):
    return rank.opt._hyper[rank.idx(key)]


def check_against_kernel_and_fp64(world, pre_full, G, tag):
    """The assembled post-step state against (1) ONE full-range vlp_fused_adam call on a clone of the pre-step state with the ranks' own
    hyper -- bit for bit: "per element the arithmetic is the unsharded kernel's" -- and (2) the fp64 restatement, test_fused_adam_sizes' bounds."""
    r0 = world.live[0]
    post = world.assembled()
    for k in KEYS:
        g = r0.opt.param_groups[r0.idx(k)]
        hyper = hyper_of(r0, k).clone()
        assert float(hyper[2]) == 0.0 and float(hyper[1]) == float(torch.tensor(LR, dtype=torch.float32)), (tag, k, hyper.tolist())
        p0, m0, v0 = (pre_full[(w, k)] for w in ("master", "m", "v"))
        p, m, v = p0.clone(), m0.clone(), v0.clone()
        p16 = torch.full_like(r0.eng.flat[k], float("nan"))
        K.fused_adam(p, m, v, G[k], p16, world.sizes[k], hyper, b1=g["betas"][0], b2=g["betas"][1], eps=g["eps"], decay=g["weight_decay"])
        for what, want in (("master", p), ("m", m), ("v", v)):
            assert bit_equal(post[(what, k)], want), (tag, k, what, int((bits(post[(what, k)]) != bits(want)).sum()))
        for r in world.live:
            assert bit_equal(r.eng.flat[k], p16), (tag, k, "p16 of rank %d" % r.eng.shard_plan.rank)
        rp, rm, rv = _adam_ref(p0, m0, v0, G[k], float(hyper[0]), LR, b1=g["betas"][0], b2=g["betas"][1], eps=g["eps"], decay=g["weight_decay"])
        ep, em, ev = rel(post[("master", k)], rp), rel(post[("m", k)], rm), rel(post[("v", k)], rv)
        el = float(((post[("master", k)].double() - rp).abs() / (rp.abs() + 1e-3)).max())
        print("test_32 %s %s: rel p %.2e m %.2e v %.2e, element-wise p %.2e" % (tag, k, ep, em, ev, el))
        assert ep < 1e-5 and em < 1e-4 and ev < 1e-4 and el < 1e-4, (tag, k, ep, em, ev, el)
        assert torch.equal(r0.eng.flat[k], post[("master", k)].half())
    return post


# ---- A ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nranks", [2, W])
def test_a_clip_inactive_equals_the_replicated_step_bit_for_bit(world, nranks):
    live = world.reset(nranks)
    rep = world.replica
    for step in range(3):
        G = world.make_grad(100 + step, 0.3)
        world.step(G)
        for k in KEYS:
            rep.eng.gflat[k].copy_(G[k])
        rep.opt.step()
        for k in KEYS:
            # clip inactive on both paths: combined == scale exactly, whatever the order the norm was summed in
            for r in live + [rep]:
                assert hyper_of(r, k).tolist() == [SCALE, float(torch.tensor(LR, dtype=torch.float32)), 0.0], (step, k, hyper_of(r, k).tolist())
            for what in ("master", "m", "v"):
                got, want = world.assemble(what, k), rep.buf(what, k)
                assert bit_equal(got, want), (step, k, what, int((bits(got) != bits(want)).sum()))
            for r in live:
                assert bit_equal(r.eng.flat[k], rep.eng.flat[k]), (step, k, "p16 of rank %d" % r.eng.shard_plan.rank)
        for r in live:
            assert bit_equal(r.opt._scale_state, rep.opt._scale_state), (step, r.opt._scale_state.tolist(), rep.opt._scale_state.tolist())
        assert rep.opt._scale_state.tolist()[:3] == [SCALE, step + 1.0, -1.0]
    assert not bit_equal(rep.buf("master", "decay"), world.base["buf"][("master", "decay")])       # (the steps did move something)


# ---- B ---------------------------------------------------------------------------------------------------------------------------------
def clip_active_steps(world, check):
    live = world.reset(W)
    full = {(w, k): world.base["buf"][(w, k)].clone() for w in ("master", "m", "v") for k in KEYS}
    for step in range(3):
        G = world.make_grad(200 + step, 30.0)
        world.step(G)
        if not check:
            continue
        for k in KEYS:
            i = live[0].idx(k)
            for r in live[1:]:
                assert bit_equal(hyper_of(r, k), hyper_of(live[0], k)), (step, k, hyper_of(r, k).tolist(), hyper_of(live[0], k).tolist())
                assert bit_equal(r.opt._sumsq[r.idx(k)], live[0].opt._sumsq[i])
            # the exchanged sum of squares against fp64 over the whole G: test_sumsq_sizes_and_accumulate's bound
            got, want = float(live[0].opt._sumsq[i][0]), float(G[k].double().pow(2).sum())
            print("test_32 B step %d %s: sumsq rel err %.2e" % (step, k, abs(got - want) / want))
            assert abs(got - want) < 1e-4 * want and float(live[0].opt._sumsq[i][1]) == 0.0, (step, k, got, want)
            # hence the clip factor x scale within half of that (the square root) of fp64's, plus four fp32 roundings (sqrt, /, +, *)
            clip = (want ** 0.5 / SCALE + 1e-6) / 1.0
            assert clip > 10.0, clip                                                   # the clip IS active
            h0 = float(hyper_of(live[0], k)[0])
            assert abs(h0 - clip * SCALE) <= (0.5e-4 + 4 * 2.0 ** -24) * clip * SCALE, (step, k, h0, clip * SCALE)
        full = check_against_kernel_and_fp64(world, full, G, "B step %d" % step)
    return live


def test_b_clip_active_one_factor_and_the_unsharded_kernels_arithmetic(world):
    clip_active_steps(world, check=True)


# ---- C ---------------------------------------------------------------------------------------------------------------------------------
def test_c_footprint_of_a_rank(world):
    live = world.reset(W)
    # owned ranges: whole 8-element vectors, and over the ranks they tile each buffer exactly once
    for k in KEYS:
        count = torch.zeros(world.sizes[k], dtype=torch.int32, device=DEV)
        for r in live:
            for lo, hi in r.eng.shard_plan.owned(k):
                assert lo % 8 == 0 and (hi - lo) % 8 == 0 and 0 <= lo < hi <= world.sizes[k], (k, lo, hi)
                count[lo:hi] += 1
        assert int(count.min()) == 1 and int(count.max()) == 1, (k, int(count.min()), int(count.max()))
    outside = {}
    for i, r in enumerate(live):
        for k in KEYS:
            o = torch.ones(world.sizes[k], dtype=torch.bool, device=DEV)
            for lo, hi in r.eng.shard_plan.owned(k):
                o[lo:hi] = False
            outside[(i, k)] = o
    for step in range(3):
        G = world.make_grad(300 + step, 30.0)

        def after_rank(i, was_i):
            # straight after rank i's own step, before the next rank runs and before any gather of master / m / v: nothing outside its ranges
            # has moved (p16 too, for every rank but the last -- the in-process parameter all-gather completes when the last rank joins)
            r = live[i]
            for k in KEYS:
                o = outside[(i, k)]
                for what in STATE if i < W - 1 else STATE[:3]:
                    was, now = was_i["buf"][(what, k)], r.buf(what, k)
                    assert torch.equal(bits(now)[o], bits(was)[o]), (step, i, k, what)
                    assert not torch.equal(bits(now)[~o], bits(was)[~o]), (step, i, k, what, "own range not updated")
        world.step(G, after_rank)
        for i, r in enumerate(live):
            for k in KEYS:
                assert bit_equal(r.eng.flat[k], live[0].eng.flat[k]), (step, i, k)          # after gather_params: one set of parameters
                for what in STATE:
                    assert bool(torch.isfinite(r.buf(what, k)).all()), (step, i, k, what)
                # the premise: every gradient element this rank does not own is still NaN, every owned one is G's
                gf = r.eng.gflat[k]
                assert bool(torch.isnan(gf[outside[(i, k)]]).all()) and torch.equal(gf[~outside[(i, k)]], G[k][~outside[(i, k)]])
                assert bool(torch.isfinite(r.opt._sumsq[r.idx(k)]).all()) and bool(torch.isfinite(hyper_of(r, k)).all())
            assert float(r.opt._ovf[0]) == 0.0 and r.opt.skipped_steps == 0, (step, i)
    assert all(r.opt.applied_steps == 3 for r in live)


# ---- D ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["middle_bucket", "tail", "two_ranks"])
def test_d_overflow_seen_by_one_rank_skips_on_all(world, where):
    """Step 2 of 3 carries an inf in an element rank 5 alone owns.  two_ranks: also one in rank 2's part of bucket 0 (the same param
    group), so that the exchanged flag is 2.0 -- the skip must not depend on the flag being 1.0."""
    live = world.reset(W)
    plan5, plan2 = live[5].eng.shard_plan, live[2].eng.shard_plan
    full = {(w, k): world.base["buf"][(w, k)].clone() for w in ("master", "m", "v") for k in KEYS}
    for step in range(3):
        G = world.make_grad(400 + step, 30.0)
        if step == 1:
            if where in ("middle_bucket", "two_ranks"):
                G["decay"][plan5.owned_main[1][0] + 11] = float("inf")
            if where == "tail":
                G["nodecay"][plan5.owned_tail[0] + 3] = float("-inf")
            if where == "two_ranks":
                G["decay"][plan2.owned_main[0][1] - 1] = float("inf")
        pre = world.step(G)
        if step == 1:
            for i, r in enumerate(live):
                for key, was in pre[i]["buf"].items():
                    assert bit_equal(r.buf(*key), was), (where, i, key, "an overflow step must leave the state untouched")
                st = r.opt._scale_state.tolist()
                assert st[0] == SCALE / 2 and st[1] == 2.0 and st[2] == 1.0 and st[6] == 1.0, (where, i, st)
                assert float(r.opt._ovf[0]) == (2.0 if where == "two_ranks" else 1.0), (where, i, float(r.opt._ovf[0]))
                assert all(float(hyper_of(r, k)[2]) != 0.0 for k in KEYS), (where, i)
        else:
            assert all(r.opt._scale_state.tolist()[0] == (SCALE if step == 0 else SCALE / 2) for r in live)
            full = check_against_kernel_and_fp64(world, full, G, "D %s step %d" % (where, step))       # steps 1 and 3 apply, and apply right
    for i, r in enumerate(live):
        assert r.opt.skipped_steps == 1 and r.opt.applied_steps == 2 and r.opt.cur_scale == SCALE / 2 and r.opt.cur_iter == 3, (where, i)


# ---- E ---------------------------------------------------------------------------------------------------------------------------------
def assert_same(a, b, path):
    if torch.is_tensor(a):
        assert torch.is_tensor(b) and bit_equal(a, b), path
    elif isinstance(a, dict):
        assert isinstance(b, dict) and list(a) == list(b), path
        for k in a:
            assert_same(a[k], b[k], path + (k,))
    elif isinstance(a, (list, tuple)):
        assert type(a) is type(b) and len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            assert_same(x, y, path + (i,))
    else:
        assert a == b, (path, a, b)


def test_e_checkpoint_gathers_once_per_step(world):
    live = clip_active_steps(world, check=False)
    calls = world.group.calls
    owners = world.assembled()
    assert calls["gather_state"] == 0
    # before the gather a rank's master is stale outside its chunks: that is what consolidate() is for
    assert not bit_equal(live[0].buf("master", "decay"), owners[("master", "decay")])
    for r in live:
        r.opt.consolidate()
    assert calls["gather_state"] == W
    for r in live:
        for (what, k), want in owners.items():
            assert bit_equal(r.buf(what, k), want), (r.eng.shard_plan.rank, what, k)          # every rank: the owners' chunks, tail included
    sds = [(r.opt.state_dict(), r.opt.apex_state_dict()) for r in live]
    assert calls["gather_state"] == W                                  # state_dict() of a consolidated optimizer does not gather again
    for i in range(1, W):
        assert_same(sds[0][0], sds[i][0], ("state_dict", i))
        assert_same(sds[0][1], sds[i][1], ("apex_state_dict", i))
    assert sds[0][0]["optimizer_state_dict"]["step"] == 3 and bit_equal(sds[0][0]["fp32_groups_flat"][live[0].idx("nodecay")], owners[("master", "nodecay")])
    for r in live:
        r.opt.consolidate()
    assert calls["gather_state"] == W, "a second consolidate() without a step in between must not gather"
    world.step(world.make_grad(250, 30.0))
    for r in live:
        r.opt.consolidate()
    assert calls["gather_state"] == 2 * W
    owners = world.assembled()
    for r in live:
        for (what, k), want in owners.items():
            assert bit_equal(r.buf(what, k), want), (r.eng.shard_plan.rank, what, k)


# ---- F ---------------------------------------------------------------------------------------------------------------------------------
def test_f_hand_off_to_the_engine(world):
    live = world.reset(W)
    world.step(world.make_grad(500, 0.3))
    r0 = live[0]
    eng = r0.eng
    assert set(eng._param_works) == {"nodecay", 0, 1, 2}                # the step left its gathers for the next forward to wait for
    batch = S.batch_to(S.make_batch(4, max_len_b=20, vocab_size=1024, max_pred=3, seed=1), DEV, half=True)
    r0.opt.zero_grad()
    lt = fwd_bwd(r0.model, r0.opt, batch)
    assert eng._param_works is None
    assert bool(torch.isfinite(lt[0].detach()).all()) and float(lt[0].detach()) > 0
    with pytest.raises(RuntimeError, match="cannot be accumulated"):
        fwd_bwd(r0.model, r0.opt, batch)                                # no zero_grad() in between: accumulation, which sharded mode refuses
