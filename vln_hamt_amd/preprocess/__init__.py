"""Offline preprocessing: view-feature extraction (reference: preprocess/precompute_img_features_vit.py) and the stored panorama
views (reference: preprocess/build_image_lmdb.py)."""
from .extract import (ViewFeatureExtractor, ViewFeatureWriter, build_feature_extractor, build_feature_file,  # noqa: F401
                      load_viewpoint_ids)
from .store import PanoImageWriter, build_image_store  # noqa: F401
