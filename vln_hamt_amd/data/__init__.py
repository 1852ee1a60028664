"""Input side of the path, behind the names of pretrain_src/data:

* `r2r_data`  trajectory (jsonl) / view-feature (HDF5, npz, npy) readers, `MultiStepNavData.get_input` (r2r_data.py)
* `r2r_tasks` the six task datasets `MlmDataset` ... `SprelDataset` and `random_word` (r2r_tasks.py)
* `collate`   the six `*_collate` functions (r2r_tasks.py) -- packed transport, padding on the device
* `loader`    `MetaLoader`, `PrefetchLoader`, `move_to_cuda`, `build_dataloader` (loader.py)
* `image_transform` / `image_prep`  the per-view transform of the image-input pipeline: numpy host path + parameter draws / HIP kernel
* `image_data`  `PanoImageStore`, `SyntheticPanoStore`, `MultiStepNavImageData` (image_data.py)
* `image_tasks` the six `*ImageDataset` classes and `*_image_collate` functions (image_tasks.py)
* `device_store` / `device_tasks` / `device_collate`  the same six tasks with the batch built ON THE DEVICE: `PretrainStore` (resident view,
  candidate and step tables), the index-only `*IndexDataset` classes, and the `*_index_collate` functions -> `IndexedBatch`"""
from .collate import (PackedBatch, itm_collate, mlm_collate, mrc_collate, sap_collate, sar_collate, sprel_collate,  # noqa: F401
                      COLLATE)
from .loader import MetaLoader, PrefetchLoader, build_dataloader, move_to_cuda  # noqa: F401
from .r2r_data import MultiStepNavData, ViewFeatureStore, read_jsonl  # noqa: F401
from .r2r_tasks import ItmDataset, MlmDataset, MrcDataset, SapDataset, SarDataset, SprelDataset, random_word  # noqa: F401
from .image_data import MultiStepNavImageData, PanoImageStore, SyntheticPanoStore  # noqa: F401
from .image_prep import PatchRows, image_prep  # noqa: F401
from .image_tasks import (IMAGE_COLLATE, ItmImageDataset, MlmImageDataset, MrcImageDataset, PackedImageBatch, SapImageDataset,  # noqa: F401
                          SarImageDataset, SprelImageDataset, itm_image_collate, mlm_image_collate, mrc_image_collate,
                          sap_image_collate, sar_image_collate, sprel_image_collate)
from .image_transform import draw_eval_params, draw_train_params  # noqa: F401
from .device_store import PretrainStore, build_pretrain_tables, get_store, pretrain_index  # noqa: F401
from .device_tasks import (INDEX_DATASETS, ItmIndexDataset, MlmIndexDataset, MrcIndexDataset, SapIndexDataset, SarIndexDataset,  # noqa: F401
                           SprelIndexDataset)
from .device_collate import (INDEX_COLLATE, IndexedBatch, itm_index_collate, mlm_index_collate, mrc_index_collate, sap_index_collate,  # noqa: F401
                             sar_index_collate, sprel_index_collate)
