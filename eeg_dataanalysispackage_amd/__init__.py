"""MI355X-native epoch-to-feature path of EEG_DataAnalysisPackage.

Host mirror of the reference's hot-path API over the libeegfx C ABI (include/eegfx.h):

* :class:`OffLineDataProvider` -- DataTransformation/OffLineDataProvider.java
* :class:`IFeatureExtraction`, :class:`WaveletTransform` -- FeatureExtraction/*.java (fe=dwt-8)
* :class:`Context` -- device/stream + the batched and fused compute entry points
* :class:`DecisionTreeClassifier`, :func:`dtree_train`, :func:`dtree_predict` -- train_clf=dt
* :class:`RandomForestClassifier`, :func:`rforest_train`, :func:`rforest_predict`,
  :func:`poisson_bag` -- train_clf=rf
* :class:`NeuralNetworkClassifier`, :func:`nn_config_from`, :func:`nn_init_params`,
  :func:`nn_train`, :func:`nn_train_opt`, :func:`nn_predict`, :func:`nn_statistics` --
  train_clf=nn
  (the other classifiers live in :mod:`classification`; :func:`pipeline.run_train_clf` is the
  train/test flow over ``OffLineDataProvider.split`` with the rows resident on the device, and
  with ``sharded=True`` over ``splitShards`` with every row left on its shard's context)
* :mod:`brainvision` -- native .vhdr/.vmrk reader and marker planner
"""
from ._lib import EegfxError, LIB_PATH, lib
from .brainvision import (ChannelInfo, EEGMarker, Header, plan_markers, read_header,
                          read_markers, read_raw, recording_frames)
from .classification import (DecisionTreeClassifier, NeuralNetworkClassifier,
                             RandomForestClassifier, dtree_predict, dtree_train, nn_config_from,
                             nn_init_params, nn_predict, nn_statistics, nn_train, nn_train_opt,
                             poisson_bag, rforest_predict, rforest_train)
from .context import Context, device_count
from .data_provider import OffLineDataProvider
from .feature_extraction import IFeatureExtraction, WaveletTransform

__all__ = [
    "Context", "ChannelInfo", "DecisionTreeClassifier", "EEGMarker", "EegfxError", "Header",
    "IFeatureExtraction", "LIB_PATH", "NeuralNetworkClassifier", "OffLineDataProvider",
    "RandomForestClassifier", "WaveletTransform", "device_count", "dtree_predict", "dtree_train",
    "lib", "nn_config_from", "nn_init_params", "nn_predict", "nn_statistics", "nn_train",
    "nn_train_opt", "plan_markers", "poisson_bag", "read_header", "read_markers", "read_raw", "recording_frames",
    "rforest_predict", "rforest_train",
]
