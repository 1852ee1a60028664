"""-m gpu: state-handling regressions of the host side (graph replay inputs, weight shadows, optimizer checkpoints, the deferred
weight-gradient queue after a failed backward pass).  The arithmetic itself is covered by test_gpu_model / test_gpu_ops."""
import warnings

import pytest
import torch

from _util import load_npz, tiny_cfg
from test_gpu_model import DEV, build

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tiny():
    from oracle.hamt_oracle import make_state_dict, pretrain_param_shapes
    store = load_npz("tiny_pretrain.npz")
    cfg = tiny_cfg()
    sd = make_state_dict(pretrain_param_shapes(cfg), seed=int(store["meta/sd_seed"]))
    return store, cfg, sd


def _model_opt(cfg, sd, eps=1.0, p_drop=0.0):
    from vln_hamt_amd.optim import AdamW
    from vln_hamt_amd.optim.misc import NO_DECAY
    m = build(cfg, sd, "bf16", train=True)
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = p_drop
    named = list(m.named_parameters())
    groups = [{'params': [p for n, p in named if not any(nd in n for nd in NO_DECAY)], 'weight_decay': 0.01},
              {'params': [p for n, p in named if any(nd in n for nd in NO_DECAY)], 'weight_decay': 0.0}]
    return m, AdamW(groups, lr=1e-3, betas=(0.9, 0.98), eps=eps)


def _eager_step(m, o, b, task):
    from vln_hamt_amd.optim import clip_grad_norm_
    loss = m(b, task, True).mean()
    loss.backward()
    clip_grad_norm_(m.parameters(), 5.0, optimizer=o)
    o.step()
    o.zero_grad()
    return float(loss)


def _worst(m1, m2):
    return max(float((a - b).abs().max()) for (_, a), (_, b) in zip(m1.named_parameters(), m2.named_parameters()))


def test_graph_step_trains_on_the_batch_it_is_given(tiny):
    """a replay must run on the batch passed to step(), not on the batch the key was captured with."""
    from vln_hamt_amd import _lib as L
    from vln_hamt_amd.graph import GraphedTrainStep
    from vln_hamt_amd.synth import make_batch
    _, cfg, sd = tiny
    bs = [make_batch("sap", 4, cfg, seed=50 + i, txt_len=20, hist_len=4, device=DEV) for i in range(4)]
    m1, o1 = _model_opt(cfg, sd)
    l1 = [_eager_step(m1, o1, b, "sap") for b in bs]
    m2, o2 = _model_opt(cfg, sd)
    gs = GraphedTrainStep(m2, o2, 5.0)
    l2 = [float(gs.step("sap", b, "sap")) for b in bs]          # ONE key, four different batches
    gs.finish()
    torch.cuda.synchronize()
    assert len(gs.graphs) == 1
    assert max(abs(a - b) for a, b in zip(l1, l2)) < 5e-4, (l1, l2)      # (bf16 operands one ulp apart move a loss of ~1.7 by ~1e-4)
    assert len({round(x, 3) for x in l2}) == 4, l2                  # the four batches really differ
    w = _worst(m1, m2)
    assert w < 2e-5, w
    # the captured step's own inputs can be filled by the caller: nothing to copy then
    st = gs.static_batch("sap")
    for k, v in bs[0].items():
        if torch.is_tensor(v):
            st[k].copy_(v)
    gs.step("sap", st, "sap")
    # a batch of another shape under the same key is an error, not a silent replay of the captured shape
    other = make_batch("sap", 2, cfg, seed=9, txt_len=20, hist_len=4, device=DEV)
    with pytest.raises(L.HamtError, match="key_for"):
        gs.step("sap", other, "sap")
    assert GraphedTrainStep.key_for("sap", other) != GraphedTrainStep.key_for("sap", bs[0])
    # MLM without the index list cannot be captured (nonzero() = host sync + data-dependent shape)
    mlm = make_batch("mlm", 4, cfg, seed=1, txt_len=20, hist_len=4, device=DEV)
    mlm.pop("txt_label_idx", None)
    with pytest.raises(L.HamtError, match="txt_label_idx"):
        gs.step("mlm", mlm, "mlm")


def test_weight_shadow_follows_in_place_parameter_writes(tiny):
    """load_state_dict / p.data.copy_ after materialize() must not leave the GEMMs on a stale bf16 shadow."""
    from oracle.hamt_oracle import make_state_dict, pretrain_param_shapes
    from vln_hamt_amd.synth import make_batch
    _, cfg, sd = tiny
    b = make_batch("sap", 4, cfg, seed=3, txt_len=20, hist_len=4, device=DEV)
    sd2 = make_state_dict(pretrain_param_shapes(cfg), seed=77)
    m, o = _model_opt(cfg, sd)
    o.materialize()
    m.eval()
    with torch.no_grad():
        before = m(b, "sap", False).clone()
        m.load_state_dict(sd2)                                      # in-place copies into views of the arena
        after = m(b, "sap", False).clone()
    ref = build(cfg, sd2, "bf16")
    with torch.no_grad():
        want = ref(b, "sap", False)
    fin = torch.isfinite(want)
    assert float((before[fin] - want[fin]).abs().max()) > 1e-3       # the two weight sets do differ
    assert torch.equal(after[fin], want[fin]), float((after[fin] - want[fin]).abs().max())
    # after one optimizer step the arena shadow is current again and used again
    m.train()
    _eager_step(m, o, b, "sap")
    w = m.bert.encoder.layer[0].attention.self.query.weight
    from vln_hamt_amd import ops
    assert ops.arena16_valid(w, w._hamt_arena16)
    assert torch.equal(ops.weight_operand(w, "bf16").float(), w.detach().to(torch.bfloat16).float())


def test_optimizer_state_dict_roundtrip(tiny, tmp_path):
    """moments and per-parameter step counts live in flat arenas; state_dict()/load_state_dict() must carry
    them in the reference optimizer's layout (optim/adamw.py:76-84) so that a resume continues the same trajectory."""
    from vln_hamt_amd.synth import make_batch
    _, cfg, sd = tiny
    bs = [make_batch(t, 4, cfg, seed=11 + i, txt_len=20, hist_len=4, device=DEV) for i, t in enumerate(["sap", "sar", "sap", "sar", "sap", "sar"])]
    tasks = ["sap", "sar", "sap", "sar", "sap", "sar"]
    m1, o1 = _model_opt(cfg, sd, eps=1e-4)
    for b, t in zip(bs[:3], tasks[:3]):
        _eager_step(m1, o1, b, t)
    osd = o1.state_dict()
    named = dict(m1.named_parameters())
    n_state = len(osd["state"])
    assert 0 < n_state < len(named)                                  # heads of other tasks never stepped: no state, like the reference
    some = next(iter(osd["state"].values()))
    assert set(some) == {"step", "exp_avg", "exp_avg_sq"} and some["step"] in (1, 2, 3)
    path = tmp_path / "train_state.pt"
    torch.save({"model": m1.state_dict(), "optim": osd}, path)
    for b, t in zip(bs[3:], tasks[3:]):
        _eager_step(m1, o1, b, t)
    ck = torch.load(path)
    m2, o2 = _model_opt(cfg, sd, eps=1e-4)
    o2.materialize()
    m2.load_state_dict(ck["model"])
    o2.load_state_dict(ck["optim"])
    for b, t in zip(bs[3:], tasks[3:]):
        _eager_step(m2, o2, b, t)
    torch.cuda.synchronize()
    w = _worst(m1, m2)
    m3, o3 = _model_opt(cfg, sd, eps=1e-4)                           # a resume WITHOUT the optimizer state diverges measurably
    m3.load_state_dict(ck["model"])
    for b, t in zip(bs[3:], tasks[3:]):
        _eager_step(m3, o3, b, t)
    w3 = _worst(m1, m3)
    # same kernels, same inputs, dropout off: what is left is the order of the atomic adds in the embedding gradients.  eps = 1e-4
    # keeps Adam from turning that into +-lr on parameters whose true gradient is zero (the key bias of an attention: softmax
    # does not see it, its gradient is rounding noise of ~1e-8; with the reference's 1e-6 two runs of the SAME steps already
    # differ by up to lr there), while real gradients (>= 1e-3) still move by ~lr per step
    assert w < 5e-5 and w3 > 1e-4 and w3 > 10 * w, (w, w3)


def test_wgrad_queue_recovers_after_a_failed_backward(tiny):
    """an exception inside backward must not leave the deferred-weight-gradient queue switched off."""
    from vln_hamt_amd import wgrad
    from vln_hamt_amd.synth import make_batch
    _, cfg, sd = tiny
    b = make_batch("sap", 4, cfg, seed=5, txt_len=20, hist_len=4, device=DEV)
    m, o = _model_opt(cfg, sd)
    m0, o0 = _model_opt(cfg, sd)

    class Boom(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            return x.clone()

        @staticmethod
        def backward(ctx, g):
            raise RuntimeError("boom")

    # fail late in the pass: the text embedding's backward raises after the whole trunk has queued its problems
    h = m.bert.embeddings.register_forward_hook(lambda mod, i, out: Boom.apply(out))
    with pytest.raises(RuntimeError, match="boom"):
        m(b, "sap", True).mean().backward()
    h.remove()
    assert wgrad.pending(DEV) > 0                                    # the dead pass left its queue behind
    o.zero_grad()
    assert wgrad.pending(DEV) == 0                                   # zero_grad() outside a backward pass drops it
    for p in m.parameters():
        p.grad = None
    # second failure, this time NOT cleaned up by the caller: the next pass must notice the orphan itself
    h = m.bert.embeddings.register_forward_hook(lambda mod, i, out: Boom.apply(out))
    with pytest.raises(RuntimeError, match="boom"):
        m(b, "sap", True).mean().backward()
    h.remove()
    for p in m.parameters():
        p.grad = None
    n0 = wgrad.stats["dropped_stale"]
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        l1 = _eager_step(m, o, b, "sap")
    assert wgrad.stats["dropped_stale"] > n0 and any("did not finish" in str(w.message) for w in rec)
    l0 = _eager_step(m0, o0, b, "sap")
    torch.cuda.synchronize()
    assert abs(l1 - l0) < 1e-6
    w = _worst(m, m0)
    assert w < 1e-6, w                                               # every weight gradient of the good pass was computed
    assert m.bert.encoder.layer[0].attention.self.query.weight.grad is None and wgrad.pending(DEV) == 0


def test_update_overlapped_with_the_next_forward_matches_in_stream_update(tiny):
    """optim.AdamW.attach(model): the update runs chunk by chunk on its own stream while the next forward pass starts; module
    pre-hooks order every parameter read behind its chunk.  Same steps with and without it (eager), with reads of the
    optimizer / model state in between that have to wait for the update themselves."""
    from vln_hamt_amd.synth import make_batch, make_itm_rng
    _, cfg, sd = tiny
    seq = ["sap", "mlm", "sar", "itm", "mrc", "sprel", "sap", "mlm"]
    bs = []
    for i, t in enumerate(seq):
        b = make_batch(t, 4, cfg, seed=70 + i, txt_len=20, hist_len=4, ragged=True, device=DEV)
        if t == "itm":
            r = make_itm_rng(b, seed=3)
            b["itm_neg_idxs"], b["itm_shuffled_pos_ids"] = r["neg_idxs"], r["shuffled_pos_ids"]
        bs.append(b)
    m1, o1 = _model_opt(cfg, sd)
    l1 = [_eager_step(m1, o1, b, t) for b, t in zip(bs, seq)]
    m2, o2 = _model_opt(cfg, sd)
    o2.attach(m2, chunk_elems=1 << 12)          # tiny model: many chunks
    assert len(o2._ov.chunks) > 4
    l2 = []
    for i, (b, t) in enumerate(zip(bs, seq)):
        l2.append(_eager_step(m2, o2, b, t))
        if i == 2:
            osd = o2.state_dict()               # reads the moment arenas: waits for the update itself
            assert not o2._ov.pending and len(osd["state"]) > 0
        if i == 4:                              # a no-grad forward pass of a SUBMODULE right behind a step: its hooks gate it
            with torch.no_grad():
                e_gated = m2.bert.embeddings(b["txt_ids"]).clone()
                o2.wait_update()
                torch.cuda.synchronize()
                e_after = m2.bert.embeddings(b["txt_ids"])
            assert torch.equal(e_gated, e_after)
    o2.wait_update()
    torch.cuda.synchronize()
    # (the two runs take the gradient norm from different sums -- the attached optimizer reduces the whole arena, the plain one adds the
    # weight-gradient tiles' own sums of squares -- so the clip coefficient differs in the last bit and the losses (1.2 .. 6.9 here) drift
    # apart by 1e-5 .. 2e-4 over the eight steps, run after run the same: 1.86e-4 with the half-precision dense outputs of round 6, < 1e-4
    # with the bf16 ones.  A parameter read that overtook its chunk's update shows as 1e-3 and more, and in `w` below.)
    assert max(abs(a - b) for a, b in zip(l1, l2)) < 5e-4, (l1, l2)
    w = _worst(m1, m2)
    assert w < 2e-5, w
    o2.detach()
    assert o2._ov is None


def test_graph_step_with_the_update_at_the_head_of_the_next_replay(tiny):
    """GraphedTrainStep(overlap_update=True): the replay of step t+1 starts with the update of step t on its own stream (chunk
    events gate the forward pass); finish() applies the last one.  Same parameters as the eager steps, with two keys (the
    pending update crosses from one captured graph to the other) and changing learning rates."""
    from vln_hamt_amd.graph import GraphedTrainStep
    from vln_hamt_amd.synth import make_batch
    _, cfg, sd = tiny
    seq = ["sap", "sar", "sap", "sap", "sar", "sar", "sap"]
    bs = [make_batch(t, 4, cfg, seed=90 + i, txt_len=20, hist_len=4, device=DEV) for i, t in enumerate(seq)]
    lrs = [1e-3 * (1.0 - 0.1 * i) for i in range(len(seq))]
    m1, o1 = _model_opt(cfg, sd)
    l1 = []
    for b, t, lr in zip(bs, seq, lrs):
        for g in o1.param_groups:
            g["lr"] = lr
        l1.append(_eager_step(m1, o1, b, t))
    m2, o2 = _model_opt(cfg, sd)
    gs = GraphedTrainStep(m2, o2, 5.0, overlap_update=True)
    assert gs.lag and o2._ov is not None
    l2 = []
    for b, t, lr in zip(bs, seq, lrs):
        for g in o2.param_groups:
            g["lr"] = lr
        l2.append(float(gs.step(t, b, t)))
    assert gs._pending_table is not None          # the last step's update has not been applied yet ...
    w_lag = _worst(m1, m2)
    gs.finish()                                   # ... now it has
    torch.cuda.synchronize()
    assert gs._pending_table is None and len(gs.graphs) == 2
    # (a bf16 operand one ulp off moves a loss of ~2.5 by a few 1e-4: the parameters below are the sharp comparison)
    assert max(abs(a - b) for a, b in zip(l1, l2)) < 1e-3, (l1, l2)
    w = _worst(m1, m2)
    assert w < 2e-5 and w_lag > 10 * w, (w, w_lag)


def test_unzeroed_weight_gradient_slots_do_not_leak(tiny, monkeypatch):
    """The update leaves the gradient slots of the GEMM weights unzeroed (their producer stores, 30 instead of 34 bytes per
    parameter).  A head that trained in step t and has no gradient in step t+1 then still holds step t's gradient in its slot:
    neither the global norm (hamt_sumsq_table: active parameters only) nor the update may see it, and when the head trains
    again its slot is overwritten, not accumulated into.  Same trajectory as with every slot zeroed (HAMT_ZERO_ALL_GRADS)."""
    from vln_hamt_amd.optim import arena as A       # (the module whose _build reads KEEP_GRAD)
    from vln_hamt_amd.optim import clip_grad_norm_
    from vln_hamt_amd.synth import make_batch
    _, cfg, sd = tiny
    seq = ["sap", "mlm", "sar", "sap", "mlm", "sap"]
    bs = [make_batch(t, 4, cfg, seed=40 + i, txt_len=20, hist_len=4, device=DEV) for i, t in enumerate(seq)]

    def run(keep):
        monkeypatch.setattr(A, "KEEP_GRAD", keep)
        m, o = _model_opt(cfg, sd)
        norms, stale = [], None
        for i, (b, t) in enumerate(zip(bs, seq)):
            m(b, t, True).mean().backward()
            ref = float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in m.parameters() if p.grad is not None)))
            norms.append(float(clip_grad_norm_(m.parameters(), 5.0, optimizer=o)))
            assert abs(norms[-1] - ref) <= 1e-5 * ref, (i, t, norms[-1], ref)      # table norm + the weight-gradient tiles' sums == torch's norm
            o.step()
            o.zero_grad()
            if i == 1:          # after the mlm step: the observation embedder (img_linear.weight is a GEMM weight) did not train in it
                w = m.bert.img_embeddings.img_linear.weight      # (the prediction heads compute in fp32 since round 3: their slots are zeroed)
                stale = float(w._hamt_grad_slot.abs().max())
        torch.cuda.synchronize()
        return m, o, norms, stale

    m1, o1, n1, s1 = run(True)
    m0, o0, n0, s0 = run(False)
    assert (o1._keep == 2.0).sum() > 0 and (o0._keep == 2.0).sum() == 0
    assert s1 > 0.0 and s0 == 0.0, (s1, s0)                     # the slot really is stale in one run and zero in the other
    assert max(abs(a - b) / max(b, 1e-12) for a, b in zip(n1, n0)) < 1e-5, (n1, n0)
    w = _worst(m1, m0)
    assert w < 1e-6, w
    assert o1.update_bytes() < o0.update_bytes() == 34.0 * float(o0._ends[-1])


def test_clip_without_an_optimizer_argument_binds_only_to_the_exact_parameter_set(tiny):
    """The reference's call is clip_grad_norm_(model.parameters(), n) (main_r2r.py:271-273): no optimizer.  The fused path (scale
    applied inside optimizer.step()) is taken only when the list IS the optimizer's parameter set, by identity: a subset, a list
    with one parameter twice (same length as the set minus one plus a duplicate), or another model's tensors must be clipped in
    place over exactly the listed gradients, as torch does."""
    from vln_hamt_amd.optim import clip_grad_norm_
    from vln_hamt_amd.synth import make_batch
    _, cfg, sd = tiny
    b = make_batch("sap", 4, cfg, seed=71, txt_len=20, hist_len=4, device=DEV)
    m, o = _model_opt(cfg, sd)
    o.materialize()
    m(b, "sap", True).mean().backward()
    ps = [p for p in m.parameters()]
    full = float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in ps if p.grad is not None)))
    # the exact set: deferred (gradients untouched, scale pending)
    got = float(clip_grad_norm_(ps, 1e-3))
    assert abs(got - full) <= 1e-5 * full and o._pending_clip is not None
    o._pending_clip = None
    # one parameter replaced by a duplicate of another: same length, not the set -> generic path, in place, norm over the LIST
    with_grad = [p for p in ps if p.grad is not None]
    dup = list(ps)
    dup[ps.index(with_grad[0])] = with_grad[1]
    want = float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in dup if p.grad is not None)))
    before = with_grad[1].grad.detach().clone()
    got = float(clip_grad_norm_(dup, 1e30))          # (no scaling at this max_norm: the list's own norm comes back, nothing pending)
    assert abs(got - want) <= 1e-5 * want and o._pending_clip is None, (got, want)
    assert torch.equal(before, with_grad[1].grad)
    # a subset: in place over the subset only
    sub = with_grad[:5]
    want = float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in sub)))
    keep = with_grad[7].grad.detach().clone()
    got = float(clip_grad_norm_(sub, 0.5 * want))
    assert abs(got - want) <= 1e-5 * want and o._pending_clip is None
    after = float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in sub)))
    assert abs(after - 0.5 * want) <= 1e-4 * want and torch.equal(keep, with_grad[7].grad), (after, want)


def test_gradient_norm_tracks_gradients_changed_after_the_pass(tiny):
    """The weight-gradient launch leaves each tile's sum of squares for the clip (hamt_wgrad_desc.ss) so that the norm does not
    read the gradients back -- valid only while the gradients are what that launch wrote.  Accumulating a second micro-batch,
    scaling the gradients in place, replacing a .grad or dropping one must all fall back to reducing from memory."""
    from vln_hamt_amd.optim import clip_grad_norm_
    from vln_hamt_amd.synth import make_batch
    _, cfg, sd = tiny
    b1 = make_batch("sap", 4, cfg, seed=61, txt_len=20, hist_len=4, device=DEV)
    b2 = make_batch("sap", 4, cfg, seed=62, txt_len=20, hist_len=4, device=DEV)
    m, o = _model_opt(cfg, sd)
    o.materialize()

    def torch_norm():
        return float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in m.parameters() if p.grad is not None)))

    def check(what):
        ref = torch_norm()
        got = float(clip_grad_norm_(m.parameters(), 5.0, optimizer=o))
        assert abs(got - ref) <= 1e-5 * ref, (what, got, ref)

    m(b1, "sap", True).mean().backward()
    assert o._fused is not None and len(o._fused[1]) > 10          # the plain case does use the tile sums
    check("one pass")
    o.zero_grad()
    m(b1, "sap", True).mean().backward()
    m(b2, "sap", True).mean().backward()                              # second micro-batch accumulates into the same slots
    check("two accumulated passes")
    o.zero_grad()
    m(b1, "sap", True).mean().backward()
    for p in m.parameters():
        if p.grad is not None:
            p.grad.mul_(0.5)                                           # in place: the arena's version counter moves
    check("scaled in place")
    o.zero_grad()
    m(b1, "sap", True).mean().backward()
    w = m.bert.encoder.layer[0].attention.self.query.weight
    w.grad = w.grad * 3.0                                              # replaced by a new tensor
    check("one gradient replaced")
    o.zero_grad()
    m(b1, "sap", True).mean().backward()
    m.bert.encoder.layer[0].intermediate.dense.weight.grad = None      # dropped
    check("one gradient dropped")


@pytest.mark.parametrize("sharded", ["1", "0"])
def test_two_rank_bench_with_probes_finishes(tmp_path, sharded):
    """`bench.py --gpus 2 --full` under torch.distributed.run (and run plainly) must print its JSON line and exit:
    rank 0 runs the roofline probes -- model passes of its own -- while the other ranks wait in the final barrier, so the probes
    must not start a gradient exchange (round 2: they did, and every N > 1 run hung behind the timed region).  Two ranks on the
    one GPU over gloo (RCCL refuses two ranks per device); the numbers mean nothing here, finishing does."""
    import json, os, socket, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with socket.socket() as s_:
        s_.bind(("127.0.0.1", 0))
        port = s_.getsockname()[1]
    env = dict(os.environ, HAMT_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0", HAMT_SHARDED=sharded)   # reduce-scatter / all-reduce exchange
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "2", "--batch", "8", "--full"]
    if sharded == "1":      # ... and run plainly, the way the driver runs `--gpus 1`: bench.py starts its own ranks (a child process, before any GPU call)
        cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "2", "--batch", "8", "--full"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=420, cwd=root)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
    out = json.loads(line)
    assert out["n_gpus"] == 2 and out["value"] > 0 and out["roofline"]["frac"] > 0 and out["state_finite_after_timed_region"] is True, line[:600]


def test_plain_bench_times_its_steps_and_dumps_outputs(tmp_path):
    """A plain `bench.py` run does the headline only -- set up, warm up, exactly --steps timed steps, the JSON line -- and
    `--dump-outputs DIR` writes what the last timed step computed (bench.dump_outputs): float32 .npy files, finite, under 64 MB."""
    import json, os, subprocess, sys
    import numpy as np
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out_dir = tmp_path / "outputs"
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2", "--batch", "8",
           "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=root)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert out["steps"] == 3 and out["ms_per_step"] > 0 and out["value"] > 0 and out["dtype"] == "bf16", out
    assert out["higher_is_better"] is True and out["unit"] == "panorama-steps/s" and out["metric"], out
    extras = {"regions_ms_per_step", "state_finite_after_timed_region", "batch_sweep", "full_work", "ragged", "roofline",
              "kernel_table", "box", "cpu_baseline", "e2e_image_step", "rollout_step", "exchange_overhead_ms_world1"}
    assert not extras & set(out), sorted(extras & set(out))          # (behind --full)
    names = sorted(os.listdir(out_dir))
    assert names == ["exp_avg_sample.npy", "exp_avg_sq_sample.npy", "loss.npy", "param_sample.npy"], names
    assert sum(os.path.getsize(out_dir / n) for n in names) <= 64 << 20
    for n in names:
        a = np.load(out_dir / n)
        assert a.dtype == np.float32 and np.isfinite(a).all(), n
    assert np.load(out_dir / "param_sample.npy").size > 1000
    assert float(np.load(out_dir / "exp_avg_sq_sample.npy").max()) > 0        # the moments have seen gradients


def test_role_streams_are_pairwise_distinct():
    """streams.role_stream: one HIP stream per role, whatever else the process creates in between -- torch.cuda.Stream() cycles through a
    pool of 32, and two roles of one captured step on the same HIP stream ended in a segmentation fault inside hipGraph instantiation
    (first seen when the GPU suite had created enough streams for the capture stream to come round to the second compute stream)."""
    from vln_hamt_amd import streams
    seen = {}
    for role in ["side", "capture", "update", "comm", "lane0", "lane1", "test_a", "test_b", "test_c"]:
        for _ in range(13):
            torch.cuda.Stream()                     # move torch's round-robin index (13 is coprime to 32: every slot comes up)
        s = streams.role_stream(torch.cuda.current_device(), role)
        assert streams.role_stream(torch.cuda.current_device(), role) is s
        seen[role] = s.cuda_stream
    assert len(set(seen.values())) == len(seen), seen
    assert streams.side_stream(torch.cuda.current_device()).cuda_stream == seen["side"]
