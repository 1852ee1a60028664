"""-m gpu: RangerLars under the sharded exchange (parallel.ShardedItemSync: reduce-scatter, moments over the owned items, one
all-reduce of the partial slots, trust ratios everywhere, update over the owned items, all-gathers) -- how it is chosen, a one-rank
RCCL group eager and captured against plain steps, two ranks on one GPU over gloo against one process that averages their gradients
(with the all-reduce exchange measured on the same schedule as the yardstick), across a checkpoint, over a dropped pass and under
gradient accumulation."""
import os
import socket
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _util import tiny_cfg  # noqa: E402
from test_gpu_rangerlars import DEV, build, groups, tiny_sd  # noqa: E402

pytestmark = pytest.mark.gpu
ONE_RANK_BOUND = 2e-5       # test_rangerlars_one_rank_exchange_matches_single_process's worst parameter difference
SEQ2 = ["sap", "mlm", "sap", "mrc", "sap", "mlm", "sap"]       # the two-rank schedule (of _rl_rank_worker); k = 3: create at 2, interpolate at 5


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worst(a, b):
    return float((a.detach() - b.detach()).abs().max())


def _loop(m, o, batches, seq, sync=None):
    from vln_hamt_amd.optim import clip_grad_norm_
    for key in seq:                      # a task, or (step, task) where the batches differ from step to step
        t = key[1] if isinstance(key, tuple) else key
        m(batches[key], t, True).mean().backward()
        if sync is not None:
            sync(o)
        clip_grad_norm_(m.parameters(), 5.0, optimizer=o)
        o.step()
        o.zero_grad()


def test_sharded_rangerlars_choice(monkeypatch):
    from vln_hamt_amd.optim import AdamW, RangerLars, TorchAdamW
    from vln_hamt_amd.parallel import OverlappedGradSync, ShardedGradSync, ShardedItemSync, make_grad_sync
    monkeypatch.delenv("HAMT_SHARDED_RANGERLARS", raising=False)
    m = build(tiny_cfg(), tiny_sd(7), "bf16", train=True)
    o = RangerLars(groups(m), lr=1e-3, betas=(0.9, 0.98)).materialize()
    assert RangerLars.item_slice_update and not RangerLars.owned_slice_update and not getattr(AdamW, "item_slice_update", False)
    plain = o._items.clone()

    def kind(**kw):
        sync = make_grad_sync(o, **kw)
        try:
            return type(sync)
        finally:
            sync.close()

    assert kind(prec="bf16") is OverlappedGradSync and torch.equal(o._items, plain)          # the default has not moved
    assert kind(prec="bf16", sharded=True) is ShardedItemSync and o._sharded_sync is None      # (close() detaches)
    assert o._partials.numel() == 2 * o._nitems and len(o._item_cuts) > 2                      # rebuilt with the owners' boundaries as cuts
    assert kind(prec="bf16", sharded=False) is OverlappedGradSync
    monkeypatch.setenv("HAMT_SHARDED_RANGERLARS", "1")
    assert kind(prec="bf16") is ShardedItemSync and kind(prec="fp32") is OverlappedGradSync
    monkeypatch.setenv("HAMT_SHARDED", "0")
    assert kind(prec="bf16") is OverlappedGradSync
    monkeypatch.delenv("HAMT_SHARDED")
    monkeypatch.delenv("HAMT_SHARDED_RANGERLARS")
    with pytest.raises(ValueError, match="all-reduce"):
        ShardedGradSync(o)                                   # ranges that cut through parameters anywhere: still refused
    m2 = build(tiny_cfg(), tiny_sd(7), "bf16", train=True)
    with pytest.raises(ValueError, match="all-reduce"):
        ShardedItemSync(TorchAdamW(groups(m2), lr=1e-3).materialize())      # no item form of hamt_optim_table


def test_sharded_rangerlars_one_rank_matches_single_process(monkeypatch):
    """ShardedItemSync through a one-rank RCCL group, captured and eager, against plain single-process steps: schedule and bound of
    test_rangerlars_one_rank_exchange_matches_single_process (the item tables differ by the cuts, so the norms are summed in another
    order); against a single process whose item table has the same cuts the eager run is bit-identical."""
    import torch.distributed as dist
    from vln_hamt_amd import wgrad
    from vln_hamt_amd.graph import GraphedTrainStep
    from vln_hamt_amd.optim import RangerLars
    from vln_hamt_amd.parallel import ShardedItemSync, broadcast_params
    from vln_hamt_amd.synth import make_batch
    if not wgrad.ENABLED:
        pytest.skip("HAMT_NO_DEFER_WGRAD: no queued weight gradients to overlap with")
    cfg, sd = tiny_cfg(), tiny_sd(7)

    def make(cuts=None):
        m = build(cfg, sd, "bf16", train=True)
        o = RangerLars(groups(m), lr=1e-3, betas=(0.9, 0.98), eps=1.0).materialize()
        if cuts is not None:
            o.set_item_cuts(cuts)
        o.zero_grad()
        o.step()
        return m, o

    seq = ["sap", "mlm", "sap", "mrc", "mlm", "sap", "mrc"]
    batches = {t: make_batch(t, 4, cfg, seed=sum(map(ord, t)), txt_len=20, hist_len=4, ragged=True, device=DEV) for t in set(seq)}
    m1, o1 = make()
    _loop(m1, o1, batches, seq)
    monkeypatch.setenv("MASTER_ADDR", "127.0.0.1")
    monkeypatch.setenv("MASTER_PORT", str(_free_port()))
    created = not dist.is_initialized()
    if created:
        dist.init_process_group("nccl", rank=0, world_size=1)
    try:
        eager = None
        for use_graph in (True, False):
            m2, o2 = make()
            broadcast_params(o2)
            sync = ShardedItemSync(o2, n_groups=3, wire="fp32")
            try:
                assert len(sync._item_runs) == 1 and sync._item_runs[0] == (0, o2._nitems)     # one rank owns every item
                if use_graph:
                    gs = GraphedTrainStep(m2, o2, 5.0, grad_sync=sync)
                    for t in seq:
                        gs.step(t, batches[t], t)
                    assert sync._upd is not None and len(sync._upd[1]) == 2        # the update's two runs around the partials' all-reduce
                else:
                    _loop(m2, o2, batches, seq, sync)
                    eager = (m2, o2)
            finally:
                sync.close()
            torch.cuda.synchronize()
            worst = max(_worst(a, b) for (_, a), (_, b) in zip(m1.named_parameters(), m2.named_parameters()))
            print(f"[sharded rangerlars, one rank, graph={use_graph}] worst parameter difference after {len(seq)} steps: {worst:.2e}")
            assert worst < ONE_RANK_BOUND, (use_graph, worst)
            assert (o1._has_slow == o2._has_slow).all() and o1._has_slow.any() and (o1._steps == o2._steps).all()
            with pytest.raises(Exception, match="set_item_cuts"):
                o2.set_item_cuts(())                      # the slots have meaning by now
    finally:
        if created:
            dist.destroy_process_group()
    with pytest.raises(Exception, match="set_item_cuts"):
        ShardedItemSync(o1)                               # stepped with the table without cuts: refused, and left as it was found
    assert o1._sharded_sync is None and len(o1._item_cuts) == 0
    m2, o2 = eager
    m3, o3 = make(cuts=o2._item_cuts)
    assert torch.equal(o3._items, o2._items) and len(o2._item_cuts) > 2
    _loop(m3, o3, batches, seq)
    torch.cuda.synchronize()
    diff = {k: _worst(getattr(o2, k), getattr(o3, k)) for k in ("_flat_p", "_flat_m", "_flat_v", "_flat_slow", "_stats")}
    print(f"[sharded rangerlars, one rank, eager vs single process with the same cuts] {diff}")
    for k in diff:
        assert torch.equal(getattr(o2, k), getattr(o3, k)), (k, diff[k])
    assert torch.equal(o2._flat_p16.view(torch.int16), o3._flat_p16.view(torch.int16))


def _rank_batch(t, rank, i, cfg):
    from vln_hamt_amd.synth import make_batch
    return make_batch(t, 4, cfg, seed=1000 * rank + i, txt_len=20, hist_len=4, ragged=True, device=DEV)


def _new_rangerlars(m):
    from vln_hamt_amd.optim import RangerLars
    return RangerLars(groups(m), 0.5, 3, lr=1e-3, betas=(0.9, 0.98))


def _items_rank_worker(rank, world, port, out_dir):
    """one data-parallel rank with its own batches, gloo carrying the CUDA tensors (two ranks share the one GPU): the schedule under
    the all-reduce exchange first (the yardstick), then under the sharded one, then one more sharded step behind the checkpoint"""
    import torch.distributed as dist
    os.environ.update(RANK=str(rank), LOCAL_RANK="0", WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    from vln_hamt_amd.parallel import OverlappedGradSync, ShardedItemSync, broadcast_params, make_grad_sync
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        cfg = tiny_cfg()
        out = {}
        for sharded in (False, True):
            m = build(cfg, tiny_sd(5), "bf16", train=True)
            o = _new_rangerlars(m).materialize()
            broadcast_params(o)
            sync = make_grad_sync(o, "bf16", wire="fp32", sharded=sharded)
            assert type(sync) is (ShardedItemSync if sharded else OverlappedGradSync)
            try:
                owned = sync.owned() if sharded else None
                o.zero_grad()
                o.step()
                _loop(m, o, _Batches(rank, cfg), list(enumerate(SEQ2)), sync)
                torch.cuda.synchronize()
                assert o._has_slow.any() and [g["lookahead_step"] for g in o.param_groups] == [8, 8]
                if not sharded:
                    out["ar_p"] = o._flat_p.cpu()
                    continue
                n_a = o._n_shadow_only
                out.update(shadow=o._flat_p16.cpu().view(torch.int16), fp32read=o._flat_p[n_a:].cpu(), stats=o._stats.cpu(),
                           owned_kept=sync.owned() == owned, owned=owned, has_slow=o._has_slow.copy())
                try:
                    o.state_dict()
                    raise AssertionError("state_dict() of a sharded optimizer must refuse before gather_state()")
                except RuntimeError:
                    pass
                sync.gather_state()
                torch.cuda.synchronize()
                out.update(p=o._flat_p.cpu(), m=o._flat_m.cpu(), v=o._flat_v.cpu(), slow=o._flat_slow.cpu())
                if rank == 0:       # what ModelSaver writes from rank 0
                    torch.save({"model": {k: v.cpu() for k, v in m.state_dict().items()}, "optimizer": o.state_dict()}, os.path.join(out_dir, "ckpt.pt"))
                _loop(m, o, _Batches(rank, cfg), [(len(SEQ2), "mlm")], sync)
                sync.gather_state()
                torch.cuda.synchronize()
                out["p_next"] = o._flat_p.cpu()
            finally:
                sync.close()
        torch.save(out, os.path.join(out_dir, f"rank{rank}.pt"))
    finally:
        dist.destroy_process_group()


class _Batches:
    """batches[(i, task)] -> rank `rank`'s batch of step i; `_loop` indexes its batches by the schedule's entries"""

    def __init__(self, rank, cfg):
        self.rank, self.cfg = rank, cfg

    def __getitem__(self, key):
        i, t = key
        return _rank_batch(t, self.rank, i, self.cfg)


def _averaged_step(m, o, i, t, cfg):
    """one update from the mean of the two ranks' gradients (the reference loop of test_two_ranks_on_one_gpu_match_averaged_gradients)"""
    from vln_hamt_amd.optim import clip_grad_norm_
    m(_rank_batch(t, 0, i, cfg), t, True).mean().backward()
    o._pack_grads()
    g0 = o._flat_g.clone()
    o.zero_grad()
    m(_rank_batch(t, 1, i, cfg), t, True).mean().backward()
    o._pack_grads()
    o._flat_g.add_(g0).mul_(0.5)
    clip_grad_norm_(m.parameters(), 5.0, optimizer=o)
    o.step()
    o.zero_grad()


def test_sharded_rangerlars_two_ranks_on_one_gpu(tmp_path):
    """Two ranks, different batches, fp32 wire, pre-loop step + 7 steps (k = 3: a create and an interpolate).  Bound: the sharded
    path may deviate from the one-process reference by max(2 * d_ar, 2e-5), d_ar = the all-reduce exchange's own worst deviation on
    the same schedule (measured here first); 2 for the differently split partial sums, 2e-5 the one-rank figure."""
    import torch.multiprocessing as mp
    from vln_hamt_amd import wgrad
    if not wgrad.ENABLED:
        pytest.skip("HAMT_NO_DEFER_WGRAD")
    mp.spawn(_items_rank_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    a, b = (torch.load(os.path.join(str(tmp_path), f"rank{r}.pt"), weights_only=False) for r in range(2))
    for k in ("shadow", "fp32read", "stats"):
        assert torch.equal(a[k], b[k]), f"{k}: the ranks would run their next forward on different weights"
    assert a["owned_kept"] and b["owned_kept"] and a["owned"] != b["owned"] and (a["has_slow"] == b["has_slow"]).all()
    for k in ("p", "m", "v", "slow", "p_next", "ar_p"):
        assert torch.equal(a[k], b[k]), f"{k}: the ranks diverged"
    cfg = tiny_cfg()
    m = build(cfg, tiny_sd(5), "bf16", train=True)
    o = _new_rangerlars(m).materialize()
    o.zero_grad()
    o.step()
    for i, t in enumerate(SEQ2):
        _averaged_step(m, o, i, t, cfg)
    torch.cuda.synchronize()
    ref = o._flat_p.cpu()
    d_ar, d_sh = _worst(a["ar_p"], ref), _worst(a["p"], ref)
    bound = max(2 * d_ar, ONE_RANK_BOUND)
    print(f"[sharded rangerlars, two ranks] worst parameter deviation from the averaged-gradient reference after {len(SEQ2)} steps: "
          f"all-reduce exchange d_ar = {d_ar:.3e}, sharded exchange {d_sh:.3e} (bound {bound:.3e})")
    assert d_sh <= bound, (d_sh, d_ar)
    assert _worst(a["slow"], o._flat_slow.cpu()) <= bound and (a["has_slow"] == o._has_slow).all()
    # the gathered checkpoint in a fresh single process, one more step on both sides
    ck = torch.load(os.path.join(str(tmp_path), "ckpt.pt"), weights_only=False)
    assert len(ck["optimizer"]["slow_state"]) > 0
    m2 = build(cfg, ck["model"], "bf16", train=True)
    o2 = _new_rangerlars(m2)
    o2.load_state_dict(ck["optimizer"])
    assert torch.equal(o2._flat_p.cpu(), a["p"]) and torch.equal(o2._flat_m.cpu(), a["m"]) and torch.equal(o2._flat_slow.cpu(), a["slow"])
    _averaged_step(m2, o2, len(SEQ2), "mlm", cfg)
    torch.cuda.synchronize()
    d_next = _worst(a["p_next"], o2._flat_p.cpu())
    print(f"[sharded rangerlars, two ranks] one more step behind the checkpoint: {d_next:.3e}")
    assert d_next <= bound, (d_next, bound)


def test_sharded_rangerlars_dropped_pass_and_accumulation(monkeypatch):
    """Through parallel.ArenaDataParallel in a one-rank RCCL group, the exchange chosen by HAMT_SHARDED_RANGERLARS=1 as an unmodified
    script would: (a) backward, clip, NO step, zero_grad on the pass that would have been a Lookahead sync -- the pending exchange is
    dropped, step counts, the Lookahead counter and the slow buffers are those of a run without that pass (bound of
    test_rangerlars_dropped_pass_takes_its_counts_back); (b) an update accumulated over two backward passes exchanges once, and
    equals a plain single-process accumulation to the one-rank bound."""
    import torch.distributed as dist
    from vln_hamt_amd import wgrad
    from vln_hamt_amd.optim import clip_grad_norm_
    from vln_hamt_amd.parallel import ArenaDataParallel, ShardedItemSync
    from vln_hamt_amd.synth import make_batch
    if not wgrad.ENABLED:
        pytest.skip("HAMT_NO_DEFER_WGRAD")
    cfg, sd = tiny_cfg(), tiny_sd(7)
    batches = {t: make_batch(t, 4, cfg, seed=sum(map(ord, t)), txt_len=20, hist_len=4, ragged=True, device=DEV) for t in ("sap", "mlm", "mrc")}
    monkeypatch.setenv("MASTER_ADDR", "127.0.0.1")
    monkeypatch.setenv("MASTER_PORT", str(_free_port()))
    monkeypatch.setenv("HAMT_SHARDED_RANGERLARS", "1")
    created = not dist.is_initialized()
    if created:
        dist.init_process_group("nccl", rank=0, world_size=1)
    runs = []
    try:
        for drop in (False, True):
            m = build(cfg, sd, "bf16", train=True)
            o = _new_rangerlars(m).materialize()
            dp = ArenaDataParallel(m, wire="fp32")
            try:
                o.zero_grad()
                o.step()

                def one(t, step=True, scale=1.0):
                    (dp(batches[t], t, True).mean() * scale).backward()
                    if step is None:
                        return
                    clip_grad_norm_(m.parameters(), 5.0, optimizer=o)
                    if step:
                        o.step()
                    o.zero_grad()

                one("sap")
                sync = dp.grad_sync
                assert type(sync) is ShardedItemSync and o._sharded_sync is sync
                assert [g["lookahead_step"] for g in o.param_groups] == [2, 2] and not o._has_slow.any()
                if drop:
                    steps = o._steps.copy()
                    (dp(batches["mlm"], "mlm", True).mean()).backward()
                    clip_grad_norm_(m.parameters(), 5.0, optimizer=o)
                    assert sync._unconsumed and o._counted is not None and o.param_groups[0]["lookahead_step"] == 3 and o._has_slow.any()
                    o.zero_grad()
                    assert not sync._unconsumed and not sync._norm_reduced and o._counted is None and (o._steps == steps).all()
                    assert [g["lookahead_step"] for g in o.param_groups] == [2, 2] and not o._has_slow.any()
                one("sap")                      # the sync (create) -- after a dropped pass the exchange runs again instead of raising
                assert o._has_slow.any()
                one("mrc")
                # (b) one update from two micro-batches: the first pass only sums into the local arena
                dp.accumulation_steps = 2
                sync.log = []
                one("mlm", step=None, scale=0.5)
                assert sync.log == [] and not sync._unconsumed
                one("sap", scale=0.5)
                assert sync.log == list(sync._ranges), sync.log
                torch.cuda.synchronize()
                o.wait_update()
                runs.append((m, o, tuple(o._item_cuts)))
            finally:
                dp.close()
    finally:
        if created:
            dist.destroy_process_group()
    (m1, o1, cuts), (m2, o2, _) = runs
    assert (o1._steps == o2._steps).all() and (o1._has_slow == o2._has_slow).all()
    assert [g["lookahead_step"] for g in o1.param_groups] == [g["lookahead_step"] for g in o2.param_groups] == [5, 5]
    worst = max(_worst(x, y) for x, y in ((o1._flat_p, o2._flat_p), (o1._flat_slow, o2._flat_slow)))
    print(f"[sharded rangerlars] with / without a dropped pass: {worst:.2e}")
    assert worst < 1e-6, worst
    # the same schedule in a plain single process (same cuts), the accumulated update from .grad sums
    monkeypatch.delenv("HAMT_SHARDED_RANGERLARS")
    m3 = build(cfg, sd, "bf16", train=True)
    o3 = _new_rangerlars(m3).materialize()
    o3.set_item_cuts(cuts)
    o3.zero_grad()
    o3.step()
    _loop(m3, o3, batches, ["sap", "sap", "mrc"])
    (m3(batches["mlm"], "mlm", True).mean() * 0.5).backward()
    (m3(batches["sap"], "sap", True).mean() * 0.5).backward()
    clip_grad_norm_(m3.parameters(), 5.0, optimizer=o3)
    o3.step()
    o3.zero_grad()
    torch.cuda.synchronize()
    worst = _worst(o1._flat_p, o3._flat_p)
    print(f"[sharded rangerlars] accumulated update through the exchange vs a plain single process: {worst:.2e}")
    assert worst < ONE_RANK_BOUND, worst
