"""Mirror of the reference's ``finetune_src/reverie/data_utils.py`` as far as it is built: loading the object database."""
from __future__ import annotations

import numpy as np


def load_obj_database(obj_feat_file, image_feat_size):
    """{"scan_viewpoint": {'obj_ids': [str, ...], 'fts': float32 [n, <= image_feat_size], 'bboxes': [n, 4] (x1, y1, w, h, at the file's
    dtype), 'viewindexs': [n]}} for every viewpoint of the file, as reverie/data_utils.py:33-43 returns it -- what
    agent.build_obj_tables / agent.ObjStore take.  Backends by file type, as data.r2r_data.ViewFeatureStore:
      `.hdf5` / `.h5`  the reference's own file: one dataset per viewpoint, ids, boxes and view indices in its attributes (h5py);
      `.npz`           a numpy archive with the members `<scan_viewpoint>/fts`, `/obj_ids`, `/bboxes`, `/viewindexs`."""
    size = int(image_feat_size)
    ids = lambda raw: [x.decode() if isinstance(x, bytes) else str(x) for x in np.asarray(raw).tolist()]
    out = {}
    if obj_feat_file.endswith(".npz"):
        with np.load(obj_feat_file) as f:
            for key in sorted({k.rsplit("/", 1)[0] for k in f.files}):
                out[key] = {"obj_ids": ids(f[key + "/obj_ids"]), "fts": np.asarray(f[key + "/fts"]).astype(np.float32)[:, :size],
                            "bboxes": np.asarray(f[key + "/bboxes"]), "viewindexs": np.asarray(f[key + "/viewindexs"])}
        return out
    try:
        import h5py
    except ImportError as e:        # loud: there is no silent substitute for a missing reader
        raise ImportError(f"load_obj_database: '{obj_feat_file}' is an HDF5 file and h5py is not installed; convert it to an .npz "
                          "archive (<scan_viewpoint>/fts, /obj_ids, /bboxes, /viewindexs) on a machine that has h5py, or install h5py") from e
    with h5py.File(obj_feat_file, "r") as f:
        for key in f:
            out[key] = {"obj_ids": ids(f[key].attrs["obj_ids"]), "fts": f[key][...].astype(np.float32)[:, :size],
                        "bboxes": np.asarray(f[key].attrs["bboxes"]), "viewindexs": np.asarray(f[key].attrs["viewindexs"])}
    return out
