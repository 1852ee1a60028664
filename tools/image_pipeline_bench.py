#!/usr/bin/env python3
"""Image-input data pipeline at config-4 shapes (SAP sample: T = 5 history steps -> 5 + 180 + 36 = 221 view slots of 248 x 330, L = 60),
synthetic panoramas (`SyntheticPanoStore`), one JSON line per case into profiles/image_pipeline_<tag>.jsonl:

  host      per sample: the reference's PIL path (if PIL is importable) vs this package's numpy path vs packing uint8 views + records
  h2d       bytes per sample that cross PCIe: prepared fp32 images (the reference) vs the packed buffer
  kernel    hamt_image_prep per view (nchw, patch rows fp32 / bf16) against a plain torch copy_ that moves the same number of bytes
            (bytes read + bytes written = the kernel's input + output)
  step      the config-4 SAP training step (hipGraph replay, RangerLars) on resident prepared inputs vs fed by
            DataLoader -> sap_image_collate -> PrefetchLoader, and tools/e2e_bench.py's figure on the same box

usage: image_pipeline_bench.py [host] [h2d] [kernel] [step] [--batch 1,2] [--steps 12] [--workers 8] [--tag NAME]
A kernel trace of the prep kernels:  rocprofv3 --kernel-trace --stats -d <dir> -- python tools/image_pipeline_bench.py kernel
"""
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from torch.utils.data import Dataset  # noqa: E402

from vln_hamt_amd.data import image_transform as IT  # noqa: E402
from vln_hamt_amd.data.image_data import N_VIEWS, SyntheticPanoStore  # noqa: E402

T, V, L = 5, 36, 60


class SyntheticSapImages(Dataset):
    """SAP items in the form SapImageDataset yields, at fixed config-4 shapes, from synthetic panoramas"""

    def __init__(self, n=64, seed=0, n_panos=12):
        self.n, self.seed = n, seed
        self.store = SyntheticPanoStore(seed, cache=n_panos)
        self.keys = [f"scan{i // 4}_vp{i % 4}" for i in range(n_panos)]
        for k in self.keys:                   # made once, here: generating a panorama is the synthetic store's cost, not the pipeline's
            self.store.get(k)                 # (DataLoader workers inherit the cache)

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        rng = random.Random(self.seed * 100003 + i)
        g = np.random.default_rng(i)
        blocks = [self.store.get(rng.choice(self.keys)) for _ in range(T + 1)]
        recs = np.zeros((T + 1, N_VIEWS), IT.VIEW_DTYPE)
        for b in range(T + 1):
            for v in range(N_VIEWS):
                recs[b, v] = IT.draw_train_params(rng)
            recs[b]["src"] = b * N_VIEWS + np.arange(N_VIEWS)
        vidx = [rng.randrange(N_VIEWS) for _ in range(T)]
        nav = np.zeros((V + 1,), np.int64)
        nav[-1], nav[:4] = 2, 1
        return {"txt_ids": torch.from_numpy(g.integers(1000, 20000, L)), "txt_lens": L,
                "ob_images": recs[T].copy(), "ob_v_exists": True, "ob_ang_fts": torch.from_numpy(g.standard_normal((V + 1, 4), dtype=np.float32)),
                "ob_nav_types": torch.from_numpy(nav), "ob_lens": V + 1, "ob_action_viewindex": int(g.integers(0, 4)),
                "hist_images": recs[np.arange(T), vidx].copy(), "hist_ang_fts": torch.from_numpy(g.standard_normal((T, 4), dtype=np.float32)),
                "hist_pano_images": recs[:T].copy(), "hist_pano_ang_fts": torch.from_numpy(g.standard_normal((T, V, 4), dtype=np.float32)),
                "hist_lens": T, "image_views": blocks}


def _pil_view(view, rec):
    from PIL import Image, ImageEnhance, ImageOps
    l, t, w, h = int(rec["left"]), int(rec["top"]), int(rec["width"]), int(rec["height"])
    im = Image.fromarray(view).crop((l, t, l + w, t + h)).resize((224, 224), Image.BICUBIC)
    if int(rec["flip"]):
        im = ImageOps.mirror(im)
    for op in IT.unpack_order(int(rec["order"])):
        f = float((rec["brightness"], rec["contrast"], rec["saturation"])[op])
        im = (ImageEnhance.Brightness, ImageEnhance.Contrast, ImageEnhance.Color)[op](im).enhance(f)
    return torch.from_numpy(np.asarray(im)).permute(2, 0, 1).float().div(255).sub(0.5).div(0.5)


def bench_host(emit):
    from vln_hamt_amd.data.image_tasks import sap_image_collate
    ds = SyntheticSapImages()
    item = ds[0]
    views = np.concatenate(item["image_views"], 0)
    recs = np.concatenate([item["hist_pano_images"].reshape(-1), item["ob_images"]])
    res = {"case": "host", "views_per_sample": len(recs), "threads": 1}
    try:
        import PIL  # noqa: F401
        t0 = time.perf_counter()
        for r in recs:
            _pil_view(np.ascontiguousarray(views[int(r["src"])]), r)
        res["pil_ms_per_sample"] = round((time.perf_counter() - t0) * 1e3, 1)
    except ImportError:
        res["pil_ms_per_sample"] = None
    t0 = time.perf_counter()
    IT.transform_views(views, recs[:54])
    res["numpy_ms_per_sample"] = round((time.perf_counter() - t0) * 1e3 * len(recs) / 54, 1)
    t0 = time.perf_counter()
    for i in range(4):
        sap_image_collate([ds[i]])
    res["packed_ms_per_sample"] = round((time.perf_counter() - t0) * 1e3 / 4, 1)          # draws + views from the store + the packing copy
    items = [ds[i] for i in range(4)]
    t0 = time.perf_counter()
    for it in items:
        sap_image_collate([it])
    res["packed_collate_only_ms_per_sample"] = round((time.perf_counter() - t0) * 1e3 / 4, 1)
    emit(res)


def bench_h2d(emit):
    from vln_hamt_amd.data.image_tasks import sap_image_collate
    pb = sap_image_collate([SyntheticSapImages()[0]])
    slots = T + T * V + V
    emit({"case": "h2d", "slots_per_sample": slots, "prepared_fp32_bytes_per_sample": slots * 3 * 224 * 224 * 4, "packed_bytes_per_sample": pb.nbytes,
          "ratio": round(slots * 3 * 224 * 224 * 4 / pb.nbytes, 2)})


def _time(fn, reps=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def bench_kernel(emit, batches):
    from vln_hamt_amd import _lib as L_
    from vln_hamt_amd.data.image_prep import image_prep
    from vln_hamt_amd.data.image_tasks import sap_image_collate
    dev = torch.device("cuda", 0)
    ds = SyntheticSapImages()
    for B in batches:
        pb = sap_image_collate([ds[i] for i in range(B)])
        src = torch.from_numpy(pb.host_views().copy()).to(dev)
        recs = np.concatenate([pb.host_records(k) for k in ("hist_images", "hist_pano_images", "ob_images")]).copy()
        n = len(recs)
        rdev = torch.from_numpy(recs.view(np.uint8).copy()).to(dev)
        ws = torch.empty(L_.workspace_bytes(L_.WS_IMAGE_PREP, n), dtype=torch.uint8, device=dev)
        out = torch.empty((n, 3, 224, 224), device=dev)
        rows32 = torch.empty((n * 196, 768), device=dev)
        rows16 = torch.empty((n * 196, 768), dtype=torch.bfloat16, device=dev)
        res = {"case": "kernel", "B": B, "slots": n, "src_views": int(src.shape[0])}
        for name, fn, obytes in (("nchw", lambda: image_prep(src, recs, rdev, "nchw", out=out, ws=ws), out.numel() * 4),
                                 ("patches_fp32", lambda: image_prep(src, recs, rdev, "patches", out=rows32, ws=ws), rows32.numel() * 4),
                                 ("patches_bf16", lambda: image_prep(src, recs, rdev, "patches", out=rows16, ws=ws), rows16.numel() * 2)):
            ms = _time(fn)
            moved = src.numel() + obytes
            a = torch.empty(moved // 2, dtype=torch.uint8, device=dev)
            b = torch.empty_like(a)
            cms = _time(lambda: b.copy_(a))
            res[name] = {"ms": round(ms, 4), "us_per_view": round(ms * 1e3 / n, 3), "in_plus_out_bytes": moved, "copy_ms": round(cms, 4),
                         "kernel_over_copy": round(ms / cms, 2)}
        emit(res)


def bench_step(emit, batches, steps, workers):
    from vln_hamt_amd import data as D
    from vln_hamt_amd import ops
    from vln_hamt_amd.graph import GraphedTrainStep
    from vln_hamt_amd.model.image_pretrain import MultiStepNavImagePreTraining
    from vln_hamt_amd.modeling import HamtConfig
    from vln_hamt_amd.optim import RangerLars
    from vln_hamt_amd.optim.misc import NO_DECAY
    import types
    dev = torch.device("cuda", 0)
    for B in batches:
        ops.manual_seed(7, dev)
        model = MultiStepNavImagePreTraining(HamtConfig(hamt_precision="bf16", pretrain_tasks={"mlm", "sap", "sar", "sprel", "mrc", "itm"})).to(dev).train()
        named = list(model.named_parameters())
        opt = RangerLars([{"params": [p for n, p in named if not any(nd in n for nd in NO_DECAY)], "weight_decay": 0.01},
                          {"params": [p for n, p in named if any(nd in n for nd in NO_DECAY)], "weight_decay": 0.0}], lr=5e-5, betas=(0.9, 0.98))
        opt.materialize()
        graphed = GraphedTrainStep(model, opt, max_grad_norm=5.0)
        opts = types.SimpleNamespace(train_batch_size=B, val_batch_size=B, local_rank=-1, n_workers=workers, pin_mem=True)
        ds = SyntheticSapImages(n=B * (steps + 16))
        loader, _ = D.build_dataloader("sap", ds, D.sap_image_collate, True, opts)
        it = iter(D.PrefetchLoader(loader, dev, image_layout="nchw"))
        first = next(it)
        for _ in range(6):
            graphed.step("sap", first, "sap")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            graphed.step("sap", first, "sap")
        torch.cuda.synchronize()
        resident = (time.perf_counter() - t0) / steps * 1e3
        for _ in range(4):
            graphed.step("sap", next(it), "sap")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            graphed.step("sap", next(it), "sap")
        torch.cuda.synchronize()
        fed = (time.perf_counter() - t0) / steps * 1e3
        # where the loader's time goes, one batch, serialised
        t0 = time.perf_counter()
        items = [ds[i] for i in range(B)]
        item_ms = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        pb = D.sap_image_collate(items).pin_memory()
        pack = (time.perf_counter() - t0) * 1e3
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pb.buf.to(dev, non_blocking=True)
        torch.cuda.synchronize()
        h2d = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        pb.to_device(dev)
        torch.cuda.synchronize()
        todev = (time.perf_counter() - t0) * 1e3
        emit({"case": "step", "B": B, "task": "sap", "optimizer": "RangerLars", "launch": "hipGraph replay", "steps": steps, "workers": workers,
              "resident_ms_per_step": round(resident, 2), "loader_fed_ms_per_step": round(fed, 2), "fed_over_resident": round(fed / resident, 3),
              "serial_ms": {"host_items": round(item_ms, 1), "host_pack_and_pin": round(pack, 1), "h2d_copy": round(h2d, 2), "to_device_total": round(todev, 2)},
              "packed_bytes": pb.nbytes, "state_finite": bool(torch.isfinite(opt._flat_p).all())})
        del graphed, opt, model, it, loader
        torch.cuda.empty_cache()


def main(argv):
    def opt(name, default):
        return argv[argv.index(name) + 1] if name in argv else default
    cases = [c for c in ("host", "h2d", "kernel", "step") if c in argv] or ["host", "h2d", "kernel", "step"]
    batches = [int(b) for b in opt("--batch", "1,2").split(",")]
    steps, workers, tag = int(opt("--steps", "12")), int(opt("--workers", "8")), opt("--tag", "run")
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    path = os.path.join(ROOT, "profiles", f"image_pipeline_{tag}.jsonl")

    def emit(d):
        line = json.dumps(d)
        print(line, flush=True)
        with open(path, "a") as f:
            f.write(line + "\n")
    if "host" in cases:
        bench_host(emit)
    if "h2d" in cases:
        bench_h2d(emit)
    if "kernel" in cases:
        bench_kernel(emit, batches)
    if "step" in cases:
        bench_step(emit, batches, steps, workers)


if __name__ == "__main__":
    main(sys.argv[1:])
