"""Argument checks of the float32 epoch entries (eegfx_cut_epochs_f32, eegfx_extract_features_f32,
eegfx_process_recording_epochs_f32, eegfx_odp_get_data_f32) and of their Python wrappers.  No GPU:
every check below is made before the library touches a device, and the Python dtype checks are
made before the library is called at all.
"""
import ctypes

import numpy as np
import pytest

import eeg_dataanalysispackage_amd as fx
from conftest import INFO_TRAIN
from eeg_dataanalysispackage_amd._lib import EEGFX_EINVAL, EEGFX_ENOTSUP, EEGFX_ERANGE, EEGFX_OK, ptr

NULL = ctypes.c_void_p(0)
COLS = np.array([0, 1, 2], np.int32)
RES = np.array([0.1, 0.1, 0.1], np.float32)
RAW = np.zeros((1000, 3), np.int16)
POS = np.array([100, 200], np.int64)
EP = np.zeros((2, 3, 750), np.float32)
FEAT = np.zeros((2, 48), np.float64)


@pytest.fixture(scope="module")
def lib():
    return fx.lib()


@pytest.fixture(scope="module")
def ctx_block():
    """Stands in for a context where a call must fail (or return) on its arguments alone: the
    entries validate every argument before they read the context."""
    return ctypes.create_string_buffer(1 << 16)


def cut(lib, ctx, raw=RAW, pos=POS, out=EP, n=2, C=3, fmt=0, mem=0):
    return lib.eegfx_cut_epochs_f32(ctx, ptr(raw), fmt, 1000, 3, ptr(COLS), ptr(RES), C, ptr(pos),
                                    n, ptr(out), mem)


def one_pass(lib, ctx, raw=RAW, pos=POS, feat=FEAT, out=EP, n=2, C=3, fmt=0, mem=0):
    return lib.eegfx_process_recording_epochs_f32(ctx, ptr(raw), fmt, 1000, 3, ptr(COLS), ptr(RES),
                                                  C, ptr(pos), n, ptr(feat), ptr(out), mem)


def extract(lib, ctx, ep=EP, out=FEAT, n=2, C=3, name=8, size=512, skip=175, nf=16, mem=0):
    return lib.eegfx_extract_features_f32(ctx, ptr(ep), n, C, name, size, skip, nf, ptr(out), mem)


def test_null_context(lib):
    assert cut(lib, NULL) == EEGFX_EINVAL
    assert one_pass(lib, NULL) == EEGFX_EINVAL
    assert one_pass(lib, NULL, out=None) == EEGFX_EINVAL  # the eegfx_process_recording form
    assert extract(lib, NULL) == EEGFX_EINVAL
    assert cut(lib, NULL, n=0) == EEGFX_EINVAL
    assert extract(lib, NULL, n=0) == EEGFX_EINVAL
    assert lib.eegfx_odp_get_data_f32(NULL, ptr(EP)) == EEGFX_EINVAL
    assert b"null" in lib.eegfx_last_error()


def test_null_buffers(lib, ctx_block):
    for kw in ({"raw": None}, {"pos": None}, {"out": None}):
        assert cut(lib, ctx_block, **kw) == EEGFX_EINVAL
    for kw in ({"raw": None}, {"pos": None}, {"feat": None}):
        assert one_pass(lib, ctx_block, **kw) == EEGFX_EINVAL
    for kw in ({"ep": None}, {"out": None}):
        assert extract(lib, ctx_block, **kw) == EEGFX_EINVAL


def test_other_argument_errors(lib, ctx_block):
    assert cut(lib, ctx_block, fmt=2) == EEGFX_EINVAL
    assert cut(lib, ctx_block, mem=7) == EEGFX_EINVAL
    assert cut(lib, ctx_block, C=0) == EEGFX_EINVAL
    assert cut(lib, ctx_block, C=65) == EEGFX_EINVAL
    assert cut(lib, ctx_block, n=-1) == EEGFX_EINVAL
    assert one_pass(lib, ctx_block, fmt=2) == EEGFX_EINVAL
    assert extract(lib, ctx_block, n=-1) == EEGFX_EINVAL
    assert extract(lib, ctx_block, C=65) == EEGFX_EINVAL
    assert extract(lib, ctx_block, nf=0) == EEGFX_EINVAL
    assert extract(lib, ctx_block, mem=7) == EEGFX_EINVAL
    # check_fe_params, as eegfx_extract_features_f64
    assert extract(lib, ctx_block, size=256) == EEGFX_ENOTSUP
    assert extract(lib, ctx_block, name=4) == EEGFX_ENOTSUP
    assert extract(lib, ctx_block, nf=513) == EEGFX_ENOTSUP
    assert extract(lib, ctx_block, skip=239) == EEGFX_ERANGE
    assert extract(lib, ctx_block, skip=-1) == EEGFX_ERANGE
    # host positions are checked before any work is enqueued
    bad = np.array([100, 99], np.int64)
    assert cut(lib, ctx_block, pos=bad) == EEGFX_ERANGE
    assert one_pass(lib, ctx_block, pos=bad) == EEGFX_ERANGE
    far = np.array([100, 1101], np.int64)
    assert cut(lib, ctx_block, pos=far) == EEGFX_ERANGE


def test_no_epochs_is_ok(lib, ctx_block):
    assert cut(lib, ctx_block, n=0) == EEGFX_OK
    assert cut(lib, ctx_block, n=0, raw=None, pos=None, out=None) == EEGFX_OK
    assert one_pass(lib, ctx_block, n=0) == EEGFX_OK
    assert extract(lib, ctx_block, n=0) == EEGFX_OK
    assert extract(lib, ctx_block, n=0, ep=None, out=None) == EEGFX_OK


def test_planning_only_provider_holds_no_epochs(lib):
    odp = fx.OffLineDataProvider([INFO_TRAIN], plan_only=True)
    try:
        odp.loadData()
        assert odp.num_epochs() == 11
        out = np.zeros((11, 3, 750), np.float32)
        assert lib.eegfx_odp_get_data_f32(odp._h, ptr(out)) == EEGFX_EINVAL
        assert lib.eegfx_odp_get_data_f32(odp._h, NULL) == EEGFX_EINVAL
        with pytest.raises(fx.EegfxError):
            odp.getData(np.float32)
        with pytest.raises(ValueError):
            odp.getData(np.float16)
        with pytest.raises(ValueError):
            odp.getData(np.int32)
    finally:
        odp.close()


# ---- the Python dtype checks raise before any library call ----------------------------------------
@pytest.fixture()
def dead_ctx():
    """A Context without a handle: any library call through it raises RuntimeError."""
    c = fx.Context.__new__(fx.Context)
    c._h = None
    return c


def test_python_dtype_checks_come_first(dead_ctx):
    with pytest.raises(RuntimeError):  # the fixture itself: a call that reaches the library
        dead_ctx.cut_epochs(RAW, 3, COLS, RES, POS, dtype=np.float32)
    with pytest.raises(ValueError, match="float32"):
        dead_ctx.extract_features_f32(np.zeros((2, 3, 750)))            # doubles: never narrowed
    with pytest.raises(ValueError, match="float32"):
        dead_ctx.extract_features_f32(np.zeros((2, 3, 750), np.int16))
    with pytest.raises(ValueError):
        dead_ctx.extract_features_f32(np.zeros((2, 3, 512), np.float32))
    with pytest.raises(ValueError):
        dead_ctx.extract_features_f32(EP, out=np.zeros((2, 48), np.float32))
    with pytest.raises(ValueError):
        dead_ctx.cut_epochs(RAW, 3, COLS, RES, POS, dtype=np.float16)
    with pytest.raises(ValueError):
        dead_ctx.cut_epochs(RAW, 3, COLS, RES, POS, dtype=np.int32)
    with pytest.raises(ValueError):   # out of the other element type, both ways
        dead_ctx.cut_epochs(RAW, 3, COLS, RES, POS, out=np.zeros((2, 3, 750)), dtype=np.float32)
    with pytest.raises(ValueError):
        dead_ctx.cut_epochs(RAW, 3, COLS, RES, POS, out=np.zeros((2, 3, 750), np.float32))
    with pytest.raises(ValueError):
        dead_ctx.process_recording_epochs(RAW, 3, COLS, RES, POS, epochs_dtype=np.float16)
    with pytest.raises(ValueError):
        dead_ctx.process_recording_epochs(RAW, 3, COLS, RES, POS, epochs_out=np.zeros((2, 3, 750)),
                                          epochs_dtype=np.float32)
    with pytest.raises(ValueError):
        dead_ctx.process_recording_epochs(RAW, 3, COLS, RES, POS,
                                          epochs_out=np.zeros((2, 3, 750), np.float32))
