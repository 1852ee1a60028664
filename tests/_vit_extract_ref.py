"""Recipe shared by tools/gen_vit_extract_golden.py and the extraction tests: the two model configurations, their weights (the
oracle's PCG64 recipe plus head weights drawn the same way), and the inputs -- eval-transformed views of `SyntheticPanoStore(seed=3)`,
regenerated here and never stored.  tests/golden/vit_extract.npz holds the reference's outputs only."""
import numpy as np
import torch

STORE_SEED = 3
SCANVPS = [("scanA", "vp0"), ("scanB", "vp1")]          # the two synthetic viewpoints of the end-to-end test
# (tag) -> VitConfig fields, classes, weight seed, the views [(key index into SCANVPS, view index)]
CONFIGS = {
    "tiny": dict(vit=dict(img_size=224, patch_size=16, in_chans=3, embed_dim=128, depth=2, num_heads=2, mlp_ratio=2.0), classes=40, seed=31,
                 views=[(0, 0), (0, 17), (0, 35), (1, 0), (1, 6), (1, 35)]),
    "b16": dict(vit=dict(img_size=224, patch_size=16, in_chans=3, embed_dim=768, depth=12, num_heads=12, mlp_ratio=4.0), classes=1000, seed=32,
                views=[(0, 3), (1, 20)]),
}


def vit_config(tag):
    from oracle.hamt_oracle import VitConfig
    return VitConfig(**CONFIGS[tag]["vit"])


def vit_kwargs(tag):
    """constructor arguments of vln_hamt_amd's VisionTransformer"""
    return {k: v for k, v in CONFIGS[tag]["vit"].items() if k != "in_chans"}


def state_dict(tag):
    """timm keys incl. head.*: make_vit_state_dict + N(0, 0.02) head weights from PCG64(seed + 1000)"""
    from oracle.hamt_oracle import make_vit_state_dict
    c = CONFIGS[tag]
    sd = make_vit_state_dict(vit_config(tag), seed=c["seed"])
    rng = np.random.Generator(np.random.PCG64(c["seed"] + 1000))
    D = c["vit"]["embed_dim"]
    sd["head.weight"] = torch.from_numpy(0.02 * rng.standard_normal((c["classes"], D), dtype=np.float32))
    sd["head.bias"] = torch.from_numpy(0.02 * rng.standard_normal((c["classes"],), dtype=np.float32))
    return sd


def views_u8(tag):
    """uint8 (n, 248, 330, 3)"""
    from vln_hamt_amd.data.image_data import SyntheticPanoStore
    store = SyntheticPanoStore(STORE_SEED)
    return np.stack([store.get("%s_%s" % SCANVPS[k])[v] for k, v in CONFIGS[tag]["views"]], 0)


def images(tag):
    """float32 (n, 3, 224, 224): the numpy path of the eval transform"""
    from vln_hamt_amd.data.image_transform import VIEW_DTYPE, draw_eval_params, transform_views
    v = views_u8(tag)
    recs = np.zeros((len(v),), VIEW_DTYPE)
    recs[:] = draw_eval_params(v.shape[1], v.shape[2])
    recs["src"] = np.arange(len(v))
    return transform_views(v, recs)
