"""Not gpu: REVERIE's object-grounding model (vln_hamt_amd/reverie) -- parameter names and order against the reference, the model
factory's checkpoint and config rules, the fixture against its generator, the C-ABI descriptor, the new kernels' registers."""
import ctypes
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

from _util import load_npz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cfg(no_lang_ca=True, **kw):
    from oracle.hamt_oracle import OracleConfig
    from vln_hamt_amd.modeling import HamtConfig
    o = OracleConfig.tiny(hidden_size=128, num_attention_heads=2, intermediate_size=256, image_feat_size=64, max_action_steps=50,
                          no_lang_ca=no_lang_ca)
    d = dict(vars(o))
    d.pop("pretrain_tasks")
    d["obj_feat_size"] = 64
    d.update(kw)
    return HamtConfig(**d)


def _args(**kw):
    d = dict(image_feat_size=64, angle_feat_size=4, obj_feat_size=48, num_l_layers=1, num_h_layers=0, num_x_layers=1,
             hist_enc_pano=True, hist_pano_num_layers=1, fix_lang_embedding=False, fix_hist_embedding=False, fix_obs_embedding=False,
             no_lang_ca=True, feat_dropout=0.4, tokenizer="bert", bert_ckpt_file=None)
    d.update(kw)
    return types.SimpleNamespace(**d)


def test_state_dict_keys_and_order_match_the_reference():
    from vln_hamt_amd.reverie.vlnbert_navref import NavRefCMT
    ref = [str(k) for k in load_npz("reverie_tiny.npz")["keys"]]
    assert len(ref) == 195
    assert list(NavRefCMT(_cfg()).state_dict().keys()) == ref


def test_get_vlnbert_models_config_and_fresh_heads(tmp_path, monkeypatch):
    from vln_hamt_amd.reverie import model_navref
    from vln_hamt_amd.reverie.vlnbert_navref import NavRefCMT
    monkeypatch.setattr(model_navref, "_TEXT_ENCODER", {False: dict(vocab_size=500, max_position_embeddings=64, layer_norm_eps=1e-12),
                                                        True: dict(vocab_size=700, max_position_embeddings=66, layer_norm_eps=1e-5)})
    from vln_hamt_amd.modeling import HamtConfig

    class SmallConfig(HamtConfig):          # (a small trunk: the factory takes the text encoder's structure from the config defaults)
        DEFAULTS = dict(HamtConfig.DEFAULTS, hidden_size=128, num_attention_heads=2, intermediate_size=64)
    monkeypatch.setattr(model_navref, "HamtConfig", SmallConfig)
    src = NavRefCMT(_cfg(vocab_size=500, max_position_embeddings=64, num_l_layers=1, num_x_layers=1, obj_feat_size=48, hidden_size=128,
                         num_attention_heads=2, intermediate_size=64))
    sd = src.state_dict()
    ckpt = {}
    for k, v in sd.items():
        if k.startswith(("ref_object.", "obj_embeddings.")):
            continue                                           # in no pre-training checkpoint
        v = torch.randn_like(v) if v.dtype.is_floating_point else v
        if k.startswith("next_action."):
            ckpt[k] = v                                        # the pre-training wrapper's head: moved under bert. and back
        elif k.startswith("embeddings."):
            ckpt["module.bert." + k] = v                       # a DataParallel prefix
        else:
            ckpt["bert." + k] = v
    path = str(tmp_path / "ckpt.pt")
    torch.save(ckpt, path)
    m = model_navref.get_vlnbert_models(_args(bert_ckpt_file=path, obj_feat_size=48, image_feat_size=64))
    assert isinstance(m, NavRefCMT)
    c = m.config
    assert c.max_action_steps == 50 and c.obj_feat_size == 48 and c.num_r_layers == 0 and c.no_lang_ca is True
    assert not hasattr(c, "act_pred_token") and c.pred_head_dropout_prob == 0.1 and c.update_lang_bert is True
    assert m.hist_embeddings.position_embeddings.weight.shape[0] == 50
    assert m.obj_embeddings.img_linear.weight.shape == (128, 48)
    got = m.state_dict()
    for k, v in ckpt.items():
        name = k[len("module."):] if k.startswith("module.") else k
        name = name[len("bert."):] if name.startswith("bert.") else name
        assert torch.equal(got[name], v), k
    for k, v in got.items():          # init_weights: zero biases, unit LayerNorm gains
        if k.startswith(("ref_object.", "obj_embeddings.")) and k.endswith("bias"):
            assert float(v.abs().max()) == 0.0, k
    assert float(got["obj_embeddings.layer_norm.weight"].min()) == 1.0
    assert float(got["ref_object.net.0.weight"].std()) > 0.0
    # a 100-row history position table (max_action_steps of the other tasks) is refused, naming the key
    ckpt["bert.hist_embeddings.position_embeddings.weight"] = torch.zeros(100, 128)
    torch.save(ckpt, path)
    with pytest.raises(ValueError, match="hist_embeddings.position_embeddings.weight"):
        model_navref.get_vlnbert_models(_args(bert_ckpt_file=path, obj_feat_size=48, image_feat_size=64))
    # xlm tokenizer: the XLM-R text encoder constants
    m = model_navref.get_vlnbert_models(_args(tokenizer="xlm"))
    assert m.embeddings.word_embeddings.weight.shape[0] == 700


def test_navref_model_is_the_agent_import():
    from vln_hamt_amd.models.model_HAMT import Critic as C0
    from vln_hamt_amd.reverie.model_navref import Critic, NavRefModel
    assert Critic is C0
    m = NavRefModel(_args())
    assert m.drop_env.p == 0.4 and m.vln_bert.config.obj_feat_size == 48


def test_synth_inputs_follow_the_agent():
    from vln_hamt_amd.reverie import synth
    x = synth.make_inputs(3, 4, 12, 7, [5, 0, 3, 1], 32, 24)
    assert x["obj_feats"].shape == (4, 5, 24) and x["obj_angles"].shape == (4, 5, 4) and x["obj_poses"].shape == (4, 5, 5)
    assert x["obj_angles"].stride(1) == 28 and x["obj_feats"].stride(1) == 28        # slices of one [B, n, 28] array
    assert x["obj_masks"].tolist()[1] == [True, False, False, False, False]          # no object: one all-zero row, mask True
    assert float(x["obj_feats"][1].abs().sum() + x["obj_angles"][1].abs().sum() + x["obj_poses"][1].abs().sum()) == 0.0
    act, ref = synth.targets(x, seed=1)
    assert ref[1] == -100 and act[-1] == -100
    y = synth.make_inputs(3, 4, 12, 7, [5, 0, 3, 1], 32, 24)
    assert all(torch.equal(x[k], y[k]) for k in x)


def test_obj_embed_descriptor_layout():
    from vln_hamt_amd import _lib
    assert ctypes.sizeof(_lib.ObjEmbedDesc) == 14 * 4
    assert _lib.ObjEmbedDesc.P.offset == 16 and _lib.ObjEmbedDesc.eps_img.offset == 24 and _lib.ObjEmbedDesc.p_drop.offset == 40
    assert _lib.ObjEmbedDesc.call_id.offset == 44 and _lib.ObjEmbedDesc.Mpad16.offset == 52
    assert ctypes.sizeof(_lib.ObjEmbedParams) == 14 * 8 and _lib.ObjEmbedParams.tt.offset == 80 and _lib.ObjEmbedParams.beta_out.offset == 104
    assert ctypes.sizeof(_lib.ObjEmbedGrads) == 14 * 8 and _lib.ObjEmbedGrads.dtt.offset == 80 and _lib.ObjEmbedGrads.dbeta_out.offset == 104
    hdr = open(os.path.join(ROOT, "include", "hamt.h")).read()
    for struct, cls in (("hamt_obj_embed_params", _lib.ObjEmbedParams), ("hamt_obj_embed_grads", _lib.ObjEmbedGrads)):
        body = re.search(r"typedef struct \{([^}]*)\} " + struct + ";", hdr).group(1)
        names = re.findall(r"\*(\w+)", body)
        assert names == [f for f, _ in cls._fields_], struct


def test_obj_embed_workspace_size():
    from vln_hamt_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    assert _lib.WS_OBJ_EMBED_BWD == 8
    assert _lib.workspace_bytes(_lib.WS_OBJ_EMBED_BWD, 160, 768) == 20 * 17 * 768 * 4      # 8 rows per block, 17 partial vectors
    assert _lib.workspace_bytes(_lib.WS_OBJ_EMBED_BWD, 1, 128) == 17 * 128 * 4


@pytest.mark.skipif(not os.path.isdir(os.environ.get("HAMT_REFERENCE", "/root/reference")),
                    reason="needs the reference's source tree (HAMT_REFERENCE), which the repository does not hold")
def test_committed_reverie_golden_matches_its_generator():
    """tools/gen_reverie_golden.py re-run against the reference reproduces tests/golden/reverie_tiny.npz key for key, bit for bit"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_reverie_golden", os.path.join(ROOT, "tools", "gen_reverie_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    new = gen.generate()
    old = load_npz("reverie_tiny.npz")
    assert set(new) == set(old), sorted(set(new) ^ set(old))[:10]
    for k in new:
        a = np.asarray(new[k])
        assert a.dtype == old[k].dtype and np.array_equal(a, old[k], equal_nan=a.dtype.kind == "f"), k


def test_obj_embed_kernels_do_not_spill(tmp_path):
    import test_kernel_resources as tkr
    if not (os.path.exists(tkr.READELF) and os.path.exists(tkr.OBJCOPY)):
        pytest.skip("ROCm LLVM tools not installed")
    from vln_hamt_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    seen = {}
    for co in tkr._code_objects(_lib.LIB_PATH, str(tmp_path)):
        notes = subprocess.run([tkr.READELF, "--notes", co], capture_output=True, text=True).stdout
        for blk in notes.split("- .agpr_count:")[1:]:
            name = re.search(r"\.name:\s+(\S+)", blk)
            if not name or "obj_embed_" not in name.group(1):
                continue
            seen[name.group(1)] = (int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blk).group(1)),
                                   int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)))
    assert sum("obj_embed_fwd_kernel" in n for n in seen) == 4 and sum("obj_embed_bwd_kernel" in n for n in seen) == 4, seen
    assert sum("obj_embed_reduce_kernel" in n for n in seen) == 1, seen
    assert all(sp == 0 and scratch <= 64 for sp, scratch in seen.values()), seen
