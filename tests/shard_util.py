"""W data-parallel ranks of the sharded optimizer step (VLP_DDP_MODE=sharded) emulated inside ONE process: no process group, no
subprocess.  Library-free (torch and vlp_amd.distributed only), so the stand-ins themselves are checked on CPU tensors
(tests/test_shard_util_cpu.py) before the GPU tests (tests/test_32_sharded_step_gpu.py) build on them.

`LocalShardPlan` is `vlp_amd.distributed.ShardPlan` with its three collective methods replaced; the bookkeeping (who owns what) and the
product code that drives it (`FP16_Optimizer_State._step_sharded`, `consolidate`) stay the product's.  The stand-ins follow the
definitions of the collectives they replace, NOT the plan's own `owned_chunk` arithmetic:

  all-gather of a buffer cut into W equal chunks   every rank ends up with chunk r of rank r's buffer, for every r     (all_gather_chunks)
  all-reduce(SUM) of the 4-float statistics        the ranks' vectors added in rank order, in fp32                     (sum_in_rank_order)

The ranks of one process run one after the other, so a collective cannot complete inside the call of the first rank that enters it:
  * all-gathers complete when the LAST rank of the group has joined (until then a rank's buffers hold only what it wrote itself, which is
    what a rank sees before it waits for the real collective);
  * the norm exchange needs every rank's local statistics BEFORE any rank goes on, so a step runs in two passes (`run_sharded_step`):
    a dry pass that only records what each rank would contribute, a restore of every rank's state, and the real pass, in which each
    rank receives the recorded sum (and must contribute exactly what it contributed in the dry pass)."""
import functools

import torch

from vlp_amd.distributed import ShardPlan, coalesce_buckets


# ---- the two definitions -------------------------------------------------------------------------------------------------------------
def all_gather_chunks(tensors, ranges=None):
    """tensors: one same-sized 1-D tensor per rank.  In place: for every range (lo, hi) (default: the whole tensor) cut into W equal
    chunks, chunk r of rank r's tensor is copied into every other rank's -- `dist.all_gather_into_tensor(t[lo:hi], chunk r of t[lo:hi])`."""
    world = len(tensors)
    for lo, hi in (ranges if ranges is not None else [(0, tensors[0].numel())]):
        assert (hi - lo) % world == 0, ((lo, hi), world)
        views = [t[lo:hi].view(world, -1) for t in tensors]
        for owner in range(world):
            for q in range(world):
                if q != owner:
                    views[q][owner].copy_(views[owner][owner])


def sum_in_rank_order(stats):
    """stats: one f32 vector per rank -> their sum, added in rank order in fp32 (a fixed order: the emulation is reproducible)."""
    assert all(s.dtype == torch.float32 for s in stats)
    tot = stats[0].clone()
    for s in stats[1:]:
        tot = tot + s
    return tot


# ---- the stand-in plan -----------------------------------------------------------------------------------------------------------------
class LocalGroup(object):
    """What the W plans of one process share: the pass of the current step, the recorded statistics, the ranks that have joined an
    all-gather that is not complete yet, and how often each collective was called (summed over the ranks)."""

    def __init__(self, world):
        self.world = world
        self.dry = False
        self.local_stats = [None] * world
        self.joined_params, self.joined_state = {}, {}
        self.calls = {"exchange_norms": 0, "gather_params": 0, "gather_state": 0}


class LocalShardPlan(ShardPlan):
    def __init__(self, buckets, tail_numel, slices, world, rank, group):
        super(LocalShardPlan, self).__init__(buckets, tail_numel, slices, world, rank, process_group=None)
        assert group.world == world
        self.group = group

    def exchange_norms(self, stats):
        g = self.group
        if g.dry:
            g.local_stats[self.rank] = stats.clone()
            return stats                                   # this rank's own contribution only: the dry pass is thrown away
        g.calls["exchange_norms"] += 1
        assert all(s is not None for s in g.local_stats), "real pass before every rank's dry pass"
        mine = g.local_stats[self.rank]
        assert torch.equal(stats.view(torch.int32), mine.view(torch.int32)), "rank %d contributes %r in the real pass, %r in the dry pass" % (
            self.rank, stats.tolist(), mine.tolist())
        stats.copy_(sum_in_rank_order(g.local_stats))
        return stats

    def _works(self):
        works = {"nodecay": None}
        for b in range(len(self.buckets)):
            works[b] = None
        return works

    def gather_params(self, flat_main, flat_tail):
        g = self.group
        if g.dry:
            return self._works()
        g.calls["gather_params"] += 1
        assert self.rank not in g.joined_params
        g.joined_params[self.rank] = (flat_main, flat_tail)
        if len(g.joined_params) == self.world:
            all_gather_chunks([g.joined_params[r][1] for r in range(self.world)])
            all_gather_chunks([g.joined_params[r][0] for r in range(self.world)], self.buckets)
            g.joined_params = {}
        return self._works()

    def gather_state(self, tensors_main, tensors_tail):
        g = self.group
        g.calls["gather_state"] += 1
        assert self.rank not in g.joined_state
        g.joined_state[self.rank] = (list(tensors_main), list(tensors_tail))
        if len(g.joined_state) == self.world:
            for j in range(len(tensors_main)):
                all_gather_chunks([g.joined_state[r][0][j] for r in range(self.world)], self.buckets)
            for j in range(len(tensors_tail)):
                all_gather_chunks([g.joined_state[r][1][j] for r in range(self.world)])
            g.joined_state = {}


# ---- the two-pass step -----------------------------------------------------------------------------------------------------------------
def run_sharded_step(group, steps, snapshots, restores, after_rank=None):
    """One optimizer step of all ranks.  steps[r]() runs rank r's product step (which reaches the plan's stand-ins), snapshots[r]() ->
    an opaque copy of everything that step may change, restores[r](snap) puts it back.  Returns the pre-step snapshots.
    after_rank(r, pre[r]) is called after rank r's REAL step, before rank r + 1's."""
    world = group.world
    pre = [snapshots[r]() for r in range(world)]
    group.dry, group.local_stats = True, [None] * world
    for r in range(world):
        steps[r]()
    for r in range(world):
        restores[r](pre[r])
    group.dry = False
    for r in range(world):
        steps[r]()
        if after_rank is not None:
            after_rank(r, pre[r])
    assert not group.joined_params, "a parameter all-gather some rank never joined"
    return pre


# ---- the real layouts --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def real_layout(tasks, cap_mb=50.0):
    """(buckets, tail_numel, ready-slices) of the real 12-layer model, as GradReducer / ShardPlan see them at the default bucket cap.
    No GPU needed: Engine.plan_layout is a pure function of the parameter shapes."""
    from vlp_amd.modeling import BertConfig, BertForPreTrainingLossMask
    cfg = BertConfig(28996, num_hidden_layers=12, type_vocab_size=6)
    model = BertForPreTrainingLossMask(cfg, enable_butd=True, len_vis_input=100, tasks=tasks, allow_random_fc7=True)
    lay = model.engine.plan_layout(model)
    buckets, _ = coalesce_buckets(lay["buckets"], int(cap_mb * 1024 * 1024 / 2))
    return tuple(buckets), lay["sizes"]["nodecay"], tuple(lay["buckets"])
