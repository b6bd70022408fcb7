"""CPU: the in-process stand-ins for the sharded step's collectives (tests/shard_util.py) against the definitions of the collectives they
replace, on the bucket plans of the real 12-layer models.  tests/test_32_sharded_step_gpu.py rests on them."""
import functools

import pytest
import torch

from tests.shard_util import LocalGroup, LocalShardPlan, all_gather_chunks, real_layout, run_sharded_step, sum_in_rank_order

W = 8


def _plans(tasks, world=W):
    buckets, tail, slices = real_layout(tasks)
    group = LocalGroup(world)
    return group, [LocalShardPlan(buckets, tail, slices, world, r, group) for r in range(world)]


@functools.lru_cache(maxsize=None)
def _position(n):
    return (torch.arange(n, dtype=torch.int32) % 11).to(torch.uint8)


def _stamped(n, rank, j=0):
    """uint8 [n] (the stand-ins move bytes, whatever the dtype; 116 M elements x 8 ranks stay cheap): element i of rank r's j-th buffer
    = (i mod 11) + j + 14 (r + 1) -- no two ranks, and no two buffers of a rank, agree anywhere."""
    return _position(n) + (j + 14 * (rank + 1))


def _owner_of(plans, key, n):
    """uint8 [n]: which rank the plans' own bookkeeping says owns element i; asserts that it is exactly one everywhere."""
    own = torch.full((n,), 255, dtype=torch.uint8)
    count = torch.zeros(n, dtype=torch.uint8)
    for p in plans:
        for lo, hi in p.owned(key):
            own[lo:hi] = p.rank
            count[lo:hi] += 1
    assert int(count.min()) == 1 and int(count.max()) == 1, key              # owned ranges tile the buffer exactly once
    return own


@pytest.mark.parametrize("tasks", ["img2txt", "vqa2"])
def test_all_gathers_leave_every_rank_with_the_owners_chunks(tasks):
    group, plans = _plans(tasks)
    n_main, n_tail = plans[0].buckets[-1][1], plans[0].tail[1]
    # the definition, restated per element: after the gather element i of EVERY rank = element i of its owner's buffer before it
    want_main = _position(n_main) + 14 * (_owner_of(plans, "decay", n_main) + 1)
    want_tail = _position(n_tail) + 14 * (_owner_of(plans, "nodecay", n_tail) + 1)
    flats = [(_stamped(n_main, r), _stamped(n_tail, r)) for r in range(W)]
    for r in range(W):
        works = plans[r].gather_params(*flats[r])
        assert works == dict([("nodecay", None)] + [(b, None) for b in range(len(plans[r].buckets))])
        if r < W - 1:           # not complete before the last rank joins: a rank's buffers hold what it wrote itself
            assert torch.equal(flats[r][0], _stamped(n_main, r)) and torch.equal(flats[r][1], _stamped(n_tail, r))
    for r in range(W):
        assert torch.equal(flats[r][0], want_main) and torch.equal(flats[r][1], want_tail), r
    assert group.calls["gather_params"] == W and not group.joined_params
    del flats
    # master / m / v: three tensors per buffer, each gathered on its own
    state = [([_stamped(n_main, r, j) for j in range(3)], [_stamped(n_tail, r, j) for j in range(3)]) for r in range(W)]
    for r in range(W):
        plans[r].gather_state(*state[r])
    for r in range(W):
        for j in range(3):
            assert torch.equal(state[r][0][j], want_main + j) and torch.equal(state[r][1][j], want_tail + j), (r, j)
    assert group.calls["gather_state"] == W and not group.joined_state


def test_all_gather_chunks_is_the_collectives_definition():
    """Against torch's own statement of all_gather_into_tensor: output = concatenation of the ranks' inputs, input r = chunk r."""
    g = torch.Generator().manual_seed(5)
    ts = [torch.randn(96, generator=g) for _ in range(4)]
    before = [t.clone() for t in ts]
    all_gather_chunks(ts, [(0, 32), (32, 96)])
    want = torch.cat([before[r][0:32].view(4, -1)[r] for r in range(4)] + [before[r][32:96].view(4, -1)[r] for r in range(4)])
    for t in ts:
        assert torch.equal(t, want)
    with pytest.raises(AssertionError):
        all_gather_chunks([torch.zeros(10) for _ in range(4)])


def test_norm_exchange_is_the_rank_ordered_fp32_sum():
    group, plans = _plans("vqa2")
    # fp32 inputs whose sum depends on the order of the additions: 2^24 first swallows every later 1.0, 2^24 last does not
    local = [torch.tensor([2.0 ** 24 if r == 0 else 1.0, float(r == 5), 1.0 + r * 2.0 ** -20, float(r in (2, 5))]) for r in range(W)]
    want = torch.zeros(4)
    for r in range(W):
        want = (want + local[r]) if r else local[0].clone()
    assert torch.equal(sum_in_rank_order(local), want)
    back = torch.zeros(4)
    for r in reversed(range(W)):
        back = back + local[r]
    assert not torch.equal(back, want), "inputs chosen so that the order of the additions matters"
    seen = [None] * W
    state = [local[r].clone() for r in range(W)]

    def step(r):
        def run():
            s = state[r].clone()
            out = plans[r].exchange_norms(s)
            assert out is s                                     # in place, like dist.all_reduce
            seen[r] = s
        return run
    pre = run_sharded_step(group, [step(r) for r in range(W)], [lambda r=r: state[r].clone() for r in range(W)],
                           [lambda snap, r=r: state[r].copy_(snap) for r in range(W)])
    assert all(torch.equal(pre[r], local[r]) for r in range(W))
    for r in range(W):
        assert torch.equal(seen[r], want), r                    # every rank: the same sum, flags added up (> 1 where two ranks saw an overflow)
    assert float(want[3]) == 2.0 and float(want[1]) == 1.0
    assert group.calls["exchange_norms"] == W                   # the dry pass is not a call
    # a rank that contributes something else in the real pass than in the dry pass is caught, not averaged away
    state[3][0] += 1.0
    group.dry = False
    with pytest.raises(AssertionError):
        plans[3].exchange_norms(state[3].clone())
