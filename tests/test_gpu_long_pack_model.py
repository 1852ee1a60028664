"""-m gpu: the packed text path with the limit raised to 256 tokens (vilmodel.PACK_MAX_LEN, HAMT_PACK_MAX_LEN=256), on the configuration
and batch recipe of test_gpu_model.py::test_long_text_takes_the_padded_kernels -- the R2R-canon model, four ragged instructions of up to
200 tokens with a packing plan.  Under the raised limit the nine text layers and the language side of the cross-modal layers call the
varlen entry points (attn_s128_fwd_kernel in two query chunks, the PACKED form of attn_wide_bwd_kernel); the loss meets the oracle and the
gradients meet those of the padded kernels on the same batch.  At the default limit nothing calls them: today's fallback."""
import functools

import pytest
import torch

from test_gpu_model import TOL, _CountCalls, build, rel_err, to_dev

pytestmark = pytest.mark.gpu
VARLEN = ("hamt_attn_varlen_fwd", "hamt_attn_varlen_bwd", "hamt_attn_varlen_cross_fwd", "hamt_attn_varlen_cross_bwd")


@pytest.fixture
def limit():
    """set(n): vilmodel.PACK_MAX_LEN for the rest of the test; the value it had is put back"""
    from vln_hamt_amd.model import vilmodel
    old = vilmodel.PACK_MAX_LEN
    assert old == 128                    # the default this pull request keeps

    def set_(n):
        vilmodel.PACK_MAX_LEN = n
    yield set_
    vilmodel.PACK_MAX_LEN = old


@functools.lru_cache(maxsize=2)
def _model(pano):
    from oracle.hamt_oracle import OracleConfig, make_state_dict, pretrain_param_shapes
    cfg = OracleConfig() if pano else OracleConfig(hist_enc_pano=False, num_h_pano_layers=0)
    sd = make_state_dict(pretrain_param_shapes(cfg), seed=6)
    return cfg, sd, build(cfg, sd, "bf16")


def _run(model, batch, task):
    named = dict(model.named_parameters())
    for p in named.values():
        p.grad = None
    with _CountCalls(*VARLEN) as cnt:
        loss = model(to_dev(batch), task, True)
        loss.mean().backward()
        torch.cuda.synchronize()
    return loss.detach(), {k: p.grad.detach().double().clone() for k, p in named.items() if p.grad is not None}, cnt.n


def _packed_against_padded_and_oracle(limit, pano, task, B, txt_len, hist_len, min_vis=0):
    from oracle.hamt_oracle import HamtOracle
    from vln_hamt_amd.synth import make_batch, make_itm_rng
    cfg, sd, model = _model(pano)
    batch = make_batch(task, B, cfg, seed=77, txt_len=txt_len, hist_len=hist_len, ragged=True, txt_pack=True)
    assert "txt_pack_idx" in batch and int(batch["txt_masks"].sum(1).max()) == txt_len
    n_vis = batch["hist_masks"].shape[1] + (batch["ob_masks"].shape[1] if "ob_masks" in batch else 0)
    assert max(txt_len, n_vis) > 128 and n_vis >= min_vis
    itm = None
    if task == "itm":
        itm = make_itm_rng(batch, seed=11)
        batch["itm_neg_idxs"], batch["itm_shuffled_pos_ids"] = itm["neg_idxs"], itm["shuffled_pos_ids"]
    cpu_batch = {k: v for k, v in batch.items() if not k.startswith("txt_pack") and k not in ("txt_cu", "txt_unpack_idx")}
    l0, g0, n0 = _run(model, batch, task)                   # the default limit: the padded kernels
    assert n0 == {k: 0 for k in VARLEN}, n0
    limit(256)
    l1, g1, n1 = _run(model, batch, task)
    assert all(n1[k] > 0 for k in VARLEN), n1
    ref = HamtOracle(sd, cfg).forward(cpu_batch, task, True, itm)
    e1, e0 = rel_err(l1, ref), rel_err(l0, ref)
    assert set(g1) == set(g0)
    dot = sum(float((g1[k] * g0[k]).sum()) for k in g0)
    s1, s0 = sum(float((g1[k] ** 2).sum()) for k in g0), sum(float((g0[k] ** 2).sum()) for k in g0)
    cos, ratio = dot / (s1 * s0) ** 0.5, (s1 / s0) ** 0.5
    print(f"[long pack {task} L {txt_len} vis {n_vis}] loss err vs oracle packed {e1:.2e} (padded {e0:.2e}); gradient packed vs padded: "
          f"cosine {cos:.5f}, norm ratio {ratio:.4f}; calls {n1}")
    assert e1 <= TOL["bf16"], (task, e1)
    assert cos >= 0.99 and abs(ratio - 1) <= 0.03, (task, cos, ratio)


@pytest.mark.parametrize("task", ["sap", "mlm", "itm"])
def test_long_text_runs_packed_under_the_raised_limit(limit, task):
    """200-token instructions: self-attention of the text layers and both directions of the cross attention on the packed rows
    (itm: the replicated text with its `pair`, only the [CLS] rows read behind the last layer; mlm: the masked rows)"""
    _packed_against_padded_and_oracle(limit, True, task, 8 if task == "itm" else 4, 200, 5)


def test_a_visual_side_above_128_tokens_stays_packed_under_the_raised_limit(limit):
    """100 history steps (no panorama encoder) + [CLS] + 37 observation tokens = 138 keys for the packed text queries, 138 queries on the
    packed text keys: at the default limit LxmertEncoder.forward scatters the text back in front of the cross-modal layers"""
    from vln_hamt_amd.model import vilmodel
    from vln_hamt_amd.synth import make_batch
    cfg, _, model = _model(False)
    batch = make_batch("sap", 8, cfg, seed=77, txt_len=100, hist_len=100, ragged=True, txt_pack=True)
    assert "txt_pack_idx" in batch and batch["hist_masks"].shape[1] + batch["ob_masks"].shape[1] == 138
    with _CountCalls(*VARLEN) as cnt:                      # the default limit: packed text layers, padded cross-modal layers
        assert vilmodel.PACK_MAX_LEN == 128
        model(to_dev(batch), "sap", True).mean().backward()
        torch.cuda.synchronize()
    assert cnt.n["hamt_attn_varlen_fwd"] > 0 and cnt.n["hamt_attn_varlen_cross_fwd"] == 0 == cnt.n["hamt_attn_varlen_cross_bwd"], cnt.n
    limit(256)
    with _CountCalls(*VARLEN) as cnt:
        model(to_dev(batch), "sap", True).mean().backward()
        torch.cuda.synchronize()
    assert all(cnt.n[k] > 0 for k in VARLEN), cnt.n


def test_a_visual_side_above_128_tokens_meets_the_oracle_and_the_padded_kernels(limit):
    _packed_against_padded_and_oracle(limit, False, "sap", 4, 200, 100, min_vis=138)
