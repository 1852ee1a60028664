"""GPU: REVERIE's object-grounding model (vln_hamt_amd/reverie) on the HIP path -- the fused object embedder (ops.ObjEmbedFn,
csrc/obj_embed.hip) against an fp64 restatement, the model against the reference's own outputs (tests/golden/reverie_tiny.npz,
tools/gen_reverie_golden.py), and the model under hipGraph capture."""
import math
import types

import pytest
import torch
import torch.nn.functional as F

from _util import load_npz

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = {"fp32": 1e-3, "bf16": 1e-2}
OUTS = ("act_logits", "obj_logits", "txt", "hist", "ob", "obj")


def rel_err(a, ref):
    a, ref = a.detach().cpu().double(), torch.as_tensor(ref).double()
    fin = torch.isfinite(ref)
    assert torch.equal(torch.isfinite(a), fin), "non-finite (-inf) positions differ"
    if fin.sum() == 0:
        return 0.0
    return float((a[fin] - ref[fin]).abs().max()) / max(1.0, float(ref[fin].abs().max()))


# ------------------------------------------------------------------------------------------ op level
class _Emb(torch.nn.Module):
    """the parameters of an ObjectEmbeddings module plus the two tables whose rows 1 / 2 it adds"""

    def __init__(self, K, H, fresh, seed):
        super().__init__()
        from vln_hamt_amd.reverie.vlnbert_navref import ObjectEmbeddings
        cfg = types.SimpleNamespace(obj_feat_size=K, hidden_size=H, angle_feat_size=4, hidden_dropout_prob=0.1, hamt_precision="fp32")
        self.emb = ObjectEmbeddings(cfg)
        self.tt = torch.nn.Parameter(torch.empty(2, H))
        self.nav = torch.nn.Parameter(torch.empty(3, H))
        g = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            for n, p in self.named_parameters():
                if fresh and n.endswith("bias"):
                    p.zero_()
                elif "layer_norm.weight" in n:
                    p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=g) if not fresh else torch.ones(p.shape))
                else:
                    p.copy_((0.05 if "linear.weight" in n else 0.02) * torch.randn(p.shape, generator=g))


def _ref_fp64(m, obj, ang, pos):
    """vlnbert_navref.py:31-42 restated in fp64 (eval: no dropout)"""
    e = m.emb
    P = {n: p.detach().double().requires_grad_(True) for n, p in m.named_parameters()}
    H = m.tt.shape[1]

    def ln(x, k):
        return F.layer_norm(x, (H,), P[f"emb.{k}.weight"], P[f"emb.{k}.bias"], eps=1e-12)
    lin = lambda x, k: x.double() @ P[f"emb.{k}.weight"].t() + P[f"emb.{k}.bias"]
    x = ln(lin(obj, "img_linear"), "img_layer_norm") + ln(lin(ang, "ang_linear"), "ang_layer_norm") + ln(lin(pos, "pos_linear"), "pos_layer_norm")
    x = x + P["nav"][2] + P["tt"][1]
    assert e.layer_norm.eps == 1e-12
    return ln(x, "layer_norm"), P


def _inputs(M, K, seed, zero_rows=True):
    g = torch.Generator().manual_seed(seed)
    full = torch.relu(torch.randn(M, K + 4, generator=g))              # the agent's [.., obj_feat_size + 4] array: angles are its tail
    h = torch.rand(M, generator=g) * 6.28
    full[:, K:] = torch.stack([h.sin(), h.cos(), (h / 7).sin(), (h / 7).cos()], -1)
    pos = torch.rand(M, 5, generator=g)
    if zero_rows:                                                        # viewpoints without objects: all-zero rows
        full[::7] = 0.0
        pos[::7] = 0.0
    full, pos = full.to(DEV), pos.to(DEV)
    return full[:, :K], full[:, K:], pos


def _run_op(m, obj, ang, pos, prec, dy):
    from vln_hamt_amd import ops
    for p in m.parameters():
        p.grad = None
    o = obj.clone().requires_grad_(True)
    y = ops.obj_embed(o, ang, pos, m.emb, m.tt, m.nav, 0.0, prec)
    y.backward(dy)
    torch.cuda.synchronize()
    return y.detach(), o.grad, {n: p.grad.clone() for n, p in m.named_parameters()}


@pytest.mark.parametrize("H,M,mode,fresh", [(128, 1, "fp32", False), (128, 37, "bf16", True), (128, 1000, "fp32", True),
                                            (768, 160, "fp32", False), (768, 160, "x16", True), (768, 37, "bf16", False),
                                            (768, 1000, "x16", False), (768, 1, "bf16", True)])
def test_obj_embed_op_vs_fp64(H, M, mode, fresh, monkeypatch):
    """output and every gradient of the fused embedder against fp64 autograd; mode x16: the dense layer's output is bf16 (HAMT_OBJ_EMBED_X16);
    `fresh`: zero biases, unit gains -- with the all-zero rows, the three branch LayerNorms see constant rows (rstd 1e6)"""
    from vln_hamt_amd import ops
    monkeypatch.setattr(ops, "OBJ_EMBED_X16", mode == "x16")
    prec = "fp32" if mode == "fp32" else "bf16"
    K = 64 if H == 128 else 768
    m = _Emb(K, H, fresh, seed=H + M).to(DEV)
    obj, ang, pos = _inputs(M, K, seed=M)
    assert ang.stride(0) == K + 4 and ops.obj_embed_ok(obj, ang, pos, m.emb, m.tt, m.nav)
    dy = torch.randn(M, H, generator=torch.Generator().manual_seed(3)).to(DEV)
    y, dobj, grads = _run_op(m, obj, ang, pos, prec, dy)
    o64 = obj.double().requires_grad_(True)
    ref, P = _ref_fp64(m, o64, ang, pos)
    ref.backward(dy.double())
    tol = 2e-5 if prec == "fp32" else 2.5e-2
    assert torch.isfinite(y).all() and torch.isfinite(dobj).all()
    err = float((y.double() - ref.detach()).abs().max()) / max(1.0, float(ref.detach().abs().max()))
    assert err <= tol, ("y", err)
    worst = {}
    for n, g in list(grads.items()) + [("obj", dobj)]:
        r = o64.grad if n == "obj" else P[n].grad
        assert torch.isfinite(g).all(), n
        worst[n] = float((g.double() - r).abs().max()) / max(float(r.abs().max()), 1e-30)
    gtol = 1e-4 if prec == "fp32" else 3e-2
    assert max(worst.values()) <= gtol, sorted(worst.items(), key=lambda kv: -kv[1])[:4]
    # the two constant rows: only row 1 / row 2 receive gradient, colsum(d(LN_out input)) both
    assert float(grads["tt"][0].abs().max()) == 0.0 and float(grads["nav"][:2].abs().max()) == 0.0
    assert torch.equal(grads["tt"][1], grads["nav"][2]) and torch.equal(grads["tt"][1], grads["emb.pos_layer_norm.bias"])


def test_obj_embed_backward_bit_identical_and_nan_workspace(monkeypatch):
    """two backward runs are bit-identical; NaN-prefilled scratch (every torch.empty of the op) changes nothing"""
    from vln_hamt_amd import ops
    H, M, K = 768, 160, 768
    m = _Emb(K, H, False, seed=5).to(DEV)
    obj, ang, pos = _inputs(M, K, seed=9)
    dy = torch.randn(M, H, device=DEV)
    a = _run_op(m, obj, ang, pos, "bf16", dy)
    b = _run_op(m, obj, ang, pos, "bf16", dy)
    real_empty = torch.empty

    class _T:
        def __getattr__(self, k):
            return getattr(torch, k)

        @staticmethod
        def empty(*s, **k):
            t = real_empty(*s, **k)
            if t.is_floating_point() and t.is_cuda:
                t.fill_(float("nan"))
            return t
    monkeypatch.setattr(ops, "torch", _T())
    c = _run_op(m, obj, ang, pos, "bf16", dy)
    monkeypatch.undo()
    for x in (b, c):
        assert torch.equal(a[0], x[0]) and torch.equal(a[1], x[1])
        assert all(torch.equal(a[2][n], x[2][n]) for n in a[2]), [n for n in a[2] if not torch.equal(a[2][n], x[2][n])]


@pytest.mark.parametrize("fresh", [False, True])
def test_obj_embed_fused_equals_composed_fallback(fresh, monkeypatch):
    """HAMT_OBJ_EMBED=0 (the composed path: linear, layer_norm x 4, add3, gather_rows) gives the fused result within fp32 rounding"""
    from vln_hamt_amd import ops
    H, M, K = 128, 37, 64
    m = _Emb(K, H, fresh, seed=11).to(DEV)
    obj, ang, pos = _inputs(M, K, seed=2)
    dy = torch.randn(M, H, device=DEV)

    def run():
        for p in m.parameters():
            p.grad = None
        o = obj.clone().requires_grad_(True)
        y = m.emb(o.view(1, M, K), ang.view(1, M, 4), pos.view(1, M, 5), m.tt, m.nav)
        y.backward(dy.view(1, M, H))
        return y.detach(), o.grad, {n: p.grad.clone() for n, p in m.named_parameters()}
    m.emb.prec = "fp32"
    m.eval()
    fused = run()
    monkeypatch.setattr(ops, "OBJ_EMBED", False)
    comp = run()
    assert float((fused[0] - comp[0]).abs().max()) <= 1e-5
    for n in fused[2]:
        r = comp[2][n]
        assert float((fused[2][n] - r).abs().max()) <= 1e-4 * max(1.0, float(r.abs().max())), n
    assert float((fused[1] - comp[1]).abs().max()) <= 1e-4 * max(1.0, float(comp[1].abs().max()))


# ------------------------------------------------------------------------------------------ model level
@pytest.fixture(scope="module")
def store():
    return load_npz("reverie_tiny.npz")


def _gen():
    """tools/gen_reverie_golden.py: the cases' constants, configs and input recipe (its generate() is never called here)"""
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "gen_reverie_golden.py")
    spec = importlib.util.spec_from_file_location("gen_reverie_golden", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _gen()


def _navref(ocfg, prec, zero=False, train=False):
    from oracle.hamt_oracle import make_state_dict
    from vln_hamt_amd.modeling import HamtConfig
    from vln_hamt_amd.reverie.vlnbert_navref import NavRefCMT
    kw = dict(vars(ocfg))
    kw.pop("pretrain_tasks")
    m = NavRefCMT(HamtConfig(hamt_precision=prec, obj_feat_size=G.obj_feat_size(ocfg), **kw))
    sd = make_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=G.SD_SEED)
    if zero:
        sd = {k: (torch.zeros_like(v) if k.startswith("obj_embeddings.") and k.endswith("bias") else v) for k, v in sd.items()}
    m.load_state_dict(sd, strict=True)
    return m.to(DEV).train(train)


def _dev(x):
    return {k: v.to(DEV) for k, v in x.items()}


def _history(model, x, t, B):
    step = x["step_ids"][t:t + 1] if "step_ids" in x else torch.tensor([t], device=DEV)      # (a device tensor inside a capture)
    return model("history", hist_img_feats=x["hist_img_feats"][t], hist_ang_feats=x["hist_ang_feats"][t], ob_step_ids=step,
                 hist_pano_img_feats=x["hist_pano_img_feats"][t], hist_pano_ang_feats=x["hist_pano_ang_feats"][t])


def _episode(model, x, B):
    lang = model("language", txt_ids=x["txt_ids"], txt_masks=x["txt_masks"])
    hs = [model("history").expand(B, -1)] + [_history(model, x, t, B) for t in range(3)]
    hist_masks = (torch.arange(4)[None] < torch.tensor(G.HIST_LENS[B])[:, None]).to(DEV)
    return model("visual", txt_embeds=lang, txt_masks=x["txt_masks"], hist_embeds=torch.stack(hs, 1), hist_masks=hist_masks,
                 ob_img_feats=x["ob_img_feats"], ob_ang_feats=x["ob_ang_feats"], ob_nav_types=x["ob_nav_types"], ob_masks=x["ob_masks"],
                 obj_feats=x["obj_feats"], obj_angles=x["obj_angles"], obj_poses=x["obj_poses"], obj_masks=x["obj_masks"])


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("tag", ["a/nolangca", "a/ca", "b"])
def test_navref_visual_vs_reference(tag, prec, store):
    """cases (a) / (b): language, history cls + 3 steps, visual with ragged objects and a viewpoint without objects -- six outputs"""
    cfg = G.tiny_cfg(tag != "a/ca")
    model = _navref(cfg, prec, zero=tag == "b")
    with torch.no_grad():
        outs = _episode(model, _dev(G.inputs(cfg, G.TINY)), G.TINY["B"])
    errs = {n: rel_err(o, store[f"{tag}/{n}"]) for n, o in zip(OUTS, outs)}
    print(f"[reverie {tag} {prec}] {errs}")
    assert max(errs.values()) <= TOL[prec], errs


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("no_lang_ca", [True, False])
def test_navref_model_visual_states(no_lang_ca, prec, store):
    """case (d): NavRefModel.forward('visual', ..., return_states=True) with the list of history embeddings, ragged hist_lens"""
    from vln_hamt_amd.reverie.model_navref import NavRefModel
    cfg = G.tiny_cfg(no_lang_ca)
    agent = NavRefModel.__new__(NavRefModel)
    torch.nn.Module.__init__(agent)
    agent.args = types.SimpleNamespace(no_lang_ca=no_lang_ca, feat_dropout=0.4)
    agent.vln_bert = _navref(cfg, prec)
    agent.drop_env = torch.nn.Dropout(p=0.4)
    agent.eval()
    x = _dev(G.inputs(cfg, G.TINY))
    B = G.TINY["B"]
    with torch.no_grad():
        lang = agent("language", txt_ids=x["txt_ids"], txt_masks=x["txt_masks"])
        hs = [agent("history").expand(B, -1)]
        for t in range(3):
            hs.append(agent("history", hist_img_feats=x["hist_img_feats"][t], hist_ang_feats=x["hist_ang_feats"][t], ob_step=t,
                            hist_pano_img_feats=x["hist_pano_img_feats"][t], hist_pano_ang_feats=x["hist_pano_ang_feats"][t]))
        outs = agent("visual", txt_embeds=lang, txt_masks=x["txt_masks"], hist_embeds=hs, hist_lens=G.HIST_LENS[B],
                     ob_img_feats=x["ob_img_feats"], ob_ang_feats=x["ob_ang_feats"], ob_nav_types=x["ob_nav_types"], ob_masks=x["ob_masks"],
                     obj_feats=x["obj_feats"], obj_angles=x["obj_angles"], obj_poses=x["obj_poses"], obj_masks=x["obj_masks"], return_states=True)
    tag = "d/nolangca" if no_lang_ca else "d/ca"
    assert sorted(outs) == ["act_logits", "obj_logits", "states"]
    errs = {k: rel_err(v, store[f"{tag}/{k}"]) for k, v in outs.items()}
    assert max(errs.values()) <= TOL[prec], errs


def test_navref_full_size_forward(store):
    """case (e): run_reverie.sh's shape (H 768, 9 + 4 layers, 2 panorama layers, B 8, 60 tokens, 37 views, 20 objects), fp32 and bf16"""
    cfg = G.full_cfg()
    model = _navref(cfg, "fp32")
    x = _dev(G.inputs(cfg, G.FULL))
    for prec in ("fp32", "bf16"):
        model.set_precision(prec)
        with torch.no_grad():
            outs = _episode(model, x, G.FULL["B"])
        errs = {"act_logits": rel_err(outs[0], store["e/act_logits"]), "obj_logits": rel_err(outs[1], store["e/obj_logits"])}
        for n, o in zip(("txt", "hist", "ob", "obj"), outs[2:]):
            f = o.detach().reshape(-1).cpu()
            errs[n] = rel_err(f[:: max(1, f.numel() // 257)][:257], store[f"e/probe/{n}"])
        print(f"[reverie full {prec}] {errs}")
        assert max(errs.values()) <= TOL[prec], (prec, errs)


def _rollout(model, x, act_t, ref_t, ce):
    B = x["txt_ids"].shape[0]
    lang = model("language", txt_ids=x["txt_ids"], txt_masks=x["txt_masks"])
    hs = [model("history").expand(B, -1)]
    loss = 0.0
    for t in range(3):
        out = model("visual", txt_embeds=lang, txt_masks=x["txt_masks"], hist_embeds=torch.stack(hs, 1),
                    hist_masks=torch.ones(B, t + 1, dtype=torch.bool, device=x["txt_ids"].device),
                    ob_img_feats=x["ob_img_feats"], ob_ang_feats=x["ob_ang_feats"], ob_nav_types=x["ob_nav_types"], ob_masks=x["ob_masks"],
                    obj_feats=x["obj_feats"], obj_angles=x["obj_angles"], obj_poses=x["obj_poses"], obj_masks=x["obj_masks"])
        loss = loss + ce(out[0], act_t) + ce(out[1], ref_t)
        hs.append(_history(model, x, t, B))
    return loss


def _ce_sum(x, y):
    from vln_hamt_amd import ops
    return ops.cross_entropy(x, y).sum()


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_navref_rollout_backward_vs_reference(prec, store):
    """case (c): a 3-step rollout, action CE + object CE per step (ignore_index -100, sum), ONE backward -- the loss, every parameter
    gradient's norm (per-parameter bound) and the strided probes (global cosine) against the reference's autograd"""
    from vln_hamt_amd.reverie import synth
    cfg = G.tiny_cfg(True, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, pred_head_dropout_prob=0.0)
    model = _navref(cfg, prec, train=True)
    xc = G.inputs(cfg, G.TINY)
    act_t, ref_t = synth.targets(xc, seed=5)
    loss = _rollout(model, _dev(xc), act_t.to(DEV), ref_t.to(DEV), _ce_sum)
    loss.backward()
    torch.cuda.synchronize()
    assert abs(float(loss) - float(store["c/loss"])) <= TOL[prec] * max(1.0, abs(float(store["c/loss"])))
    got = {k: p.grad for k, p in model.named_parameters() if p.grad is not None}
    names = [str(n) for n in store["c/grad_names"]]
    norms = dict(zip(names, store["c/grad_norms"].tolist()))
    assert set(names) <= set(got) and all(float(got[k].norm()) == 0.0 for k in set(got) - set(names)), set(got) ^ set(names)
    gmax = max(norms.values())
    worst = max((abs(float(got[k].double().norm()) - r) / max(r, 5e-2 * gmax), k) for k, r in norms.items())
    dot = num = den = 0.0
    for key in store:
        if key.startswith("c/probe/"):
            k = key[len("c/probe/"):]
            f = got[k].detach().reshape(-1).cpu().double()
            g = f[:: max(1, f.numel() // G.PROBE_N)][:G.PROBE_N]
            r = torch.from_numpy(store[key]).double()
            dot += float((g * r).sum()); num += float((g * g).sum()); den += float((r * r).sum())
    cos = dot / math.sqrt(num * den)
    print(f"[reverie rollout bwd {prec}] loss {float(loss):.5f} vs {float(store['c/loss']):.5f}; probe cosine {cos:.6f}; worst norm {worst}")
    assert cos >= (0.99999 if prec == "fp32" else 0.995), cos
    assert worst[0] <= (2e-3 if prec == "fp32" else 6e-2), worst


# ------------------------------------------------------------------------------------------ graphs
def test_graphed_inference_reverie_visual_matches_eager():
    """graph.GraphedInference over REVERIE `visual` calls (one key per history length) == the eager call, on fresh inputs"""
    from vln_hamt_amd.graph import GraphedInference
    cfg = G.tiny_cfg(True)
    model = _navref(cfg, "bf16")
    B = G.TINY["B"]

    def visual(lang, txt_masks, hist, hist_masks, ob_img, ob_ang, nav, ob_masks, obj, obj_ang, obj_pos, obj_masks):
        return model("visual", txt_embeds=lang, txt_masks=txt_masks, hist_embeds=hist, hist_masks=hist_masks, ob_img_feats=ob_img,
                     ob_ang_feats=ob_ang, ob_nav_types=nav, ob_masks=ob_masks, obj_feats=obj, obj_angles=obj_ang, obj_poses=obj_pos,
                     obj_masks=obj_masks)[:2]
    gv = GraphedInference(visual)
    for seed in (41, 77, 78):
        x = _dev(G.inputs(cfg, dict(G.TINY, seed=seed)))
        with torch.no_grad():
            lang = model("language", txt_ids=x["txt_ids"], txt_masks=x["txt_masks"])
            hs = [model("history").expand(B, -1)] + [_history(model, x, t, B) for t in range(3)]
        for n in (1, 2, 4):
            args = (lang, x["txt_masks"], torch.stack(hs[:n], 1), torch.ones(B, n, dtype=torch.bool, device=DEV), x["ob_img_feats"],
                    x["ob_ang_feats"], x["ob_nav_types"], x["ob_masks"], x["obj_feats"], x["obj_angles"], x["obj_poses"], x["obj_masks"])
            with torch.no_grad():
                want = visual(*args)
            got = gv(f"v{n}", *args)
            for w, g in zip(want, got):
                fin = torch.isfinite(w)
                assert torch.equal(fin, torch.isfinite(g))
                assert float((w[fin] - g[fin]).abs().max()) <= 1e-5 * max(1.0, float(w[fin].abs().max()))
    assert len(gv.graphs) == 3


def test_graphed_reverie_rollout_training_step_matches_eager():
    """GraphedTrainStep with a REVERIE rollout loss_fn (action + object CE per step, ONE backward) and AdamW == the same steps launched
    eagerly over fresh batches: the two constant rows (token type 1, nav type 2) take gradient from the object embedder AND from the
    observation embedder in the same pass -- a contribution that overwrote another would show here"""
    from vln_hamt_amd.graph import GraphedTrainStep
    from vln_hamt_amd.optim import AdamW, clip_grad_norm_
    from vln_hamt_amd.reverie import synth
    cfg = G.tiny_cfg(True, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, pred_head_dropout_prob=0.0)
    bs = []
    for i in range(4):
        x = G.inputs(cfg, dict(G.TINY, seed=90 + i))
        x["act_t"], x["ref_t"] = synth.targets(x, seed=i)
        x["step_ids"] = torch.arange(3)
        bs.append({k: v.contiguous().to(DEV) for k, v in x.items()})

    def loss_fn(model, b, _task):
        return _rollout(model, b, b["act_t"], b["ref_t"], _ce_sum)
    runs = []
    for graphed in (False, True):
        m = _navref(cfg, "bf16", train=True)
        o = AdamW([{"params": list(m.parameters()), "weight_decay": 0.01}], lr=1e-3, betas=(0.9, 0.98), eps=1.0)
        losses = []
        if graphed:
            gs = GraphedTrainStep(m, o, 5.0, loss_fn=loss_fn)
            for b in bs:
                losses.append(float(gs.step("rollout", b, "rollout")))
            gs.finish()
            assert len(gs.graphs) == 1
        else:
            for b in bs:
                loss = loss_fn(m, b, None)
                loss.backward()
                clip_grad_norm_(m.parameters(), 5.0, optimizer=o)
                o.step()
                o.zero_grad()
                losses.append(float(loss))
        runs.append((m, losses))
    torch.cuda.synchronize()
    (m1, l1), (m2, l2) = runs
    assert max(abs(a - c) / max(1.0, abs(a)) for a, c in zip(l1, l2)) < 5e-4, (l1, l2)
    p1, p2 = dict(m1.named_parameters()), dict(m2.named_parameters())
    worst = max((float((p1[k] - p2[k]).abs().max()), k) for k in p1)
    moved = float((p1["embeddings.token_type_embeddings.weight"][1] - _navref(cfg, "bf16").embeddings.token_type_embeddings.weight[1]).abs().max())
    print(f"[graphed reverie rollout] losses {l1} / {l2}; worst parameter difference {worst}; token-type row 1 moved {moved:.2e}")
    assert worst[0] < 1e-4, worst
    assert moved > 0.0
