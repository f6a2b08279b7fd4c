"""The host half of the train/test flow (no GPU): eegfx_java_shuffle against the Python
restatement of Collections.shuffle, and the refusals of a planning-only provider."""
import ctypes

import numpy as np
import pytest

import eeg_dataanalysispackage_amd as fx
from eeg_dataanalysispackage_amd import _lib, classification, pipeline
from conftest import INFO_TRAIN

SIZES = (0, 1, 2, 5, 8, 11, 64, 1000, 100003)  # 8 and 64: nextInt's power-of-two path
SEEDS = (1, 0, -3, 2 ** 48 + 5)


@pytest.mark.parametrize("seed", SEEDS)
def test_java_shuffle_equals_the_python_restatement(seed):
    for n in SIZES:
        perm = pipeline.native_shuffle(n, seed)
        assert perm.dtype == np.int64 and perm.shape == (n,)
        assert perm.tolist() == pipeline.java_shuffle_permutation(n, seed), n


def test_java_shuffle_of_the_golden_provider():
    # the 11 infoTrain epochs split into train [0,7,9,2,5,10,6] and test [3,1,8,4]
    perm = pipeline.native_shuffle(11, 1).tolist()
    assert perm == [0, 7, 9, 2, 5, 10, 6, 3, 1, 8, 4]
    assert (perm[:7], perm[7:]) == pipeline.reference_split(11)


@pytest.mark.parametrize("n", [-1, 2 ** 31])
def test_java_shuffle_refuses_what_a_java_list_cannot_hold(n):
    guard = np.full(4, -7, dtype=np.int64)
    rc = fx.lib().eegfx_java_shuffle(n, 1, ctypes.c_void_p(guard.ctypes.data))
    assert rc == _lib.EEGFX_EINVAL
    assert (guard == -7).all()
    with pytest.raises(fx.EegfxError):
        pipeline.native_shuffle(n)


def test_planning_only_provider_refuses_the_flow():
    odp = fx.OffLineDataProvider([INFO_TRAIN], plan_only=True)
    odp.loadData()
    assert odp.num_epochs() == 11
    for device in (True, False):
        with pytest.raises(fx.EegfxError, match="planning-only") as e:
            odp.split(device=device)
        assert e.value.code == _lib.EEGFX_EINVAL
    n_train = ctypes.c_int64(-5)
    rc = fx.lib().eegfx_odp_split(odp._h, None, 1, 0.7, 8, 512, 175, 16, None, None,
                                  ctypes.byref(n_train), _lib.MEM_HOST)
    assert rc == _lib.EEGFX_EINVAL
    with pytest.raises(fx.EegfxError, match="planning-only"):
        pipeline.run_train_clf(odp, classification.LogisticRegressionClassifier())
    odp.close()
