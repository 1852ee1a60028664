"""Offline preprocessing: view-feature extraction (reference: preprocess/precompute_img_features_vit.py)."""
from .extract import (ViewFeatureExtractor, ViewFeatureWriter, build_feature_extractor, build_feature_file,  # noqa: F401
                      load_viewpoint_ids)
