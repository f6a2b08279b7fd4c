"""The yardstick of test_gpu_pyramid.py: oracle.extract_features for feature sizes above 16 (the
full dwt-8 pyramid, WaveletTransform.java:126-137, :205-212) against a level-by-level periodic
DWT written here with numpy, and the Python class's feature dimension.  No device.

Bound: the rows are unit vectors (L2-normalised), so every value is at most 1 in magnitude.  The
two computations differ only in the order numpy sums the 10 tap products of a coefficient (and
the row's squares); each coefficient is reached through at most 6 levels of 10-term sums of
values no larger than the row's norm, i.e. an error of a few dozen ulps of 1 at the very most
(measured: <= 2.3e-16).  1e-13 absolute leaves two orders of magnitude over that bound and is
twelve orders below a wrong tap, sign, band order or wrap-around.
"""
import numpy as np
import pytest

import eeg_dataanalysispackage_amd as fx
from oracle import oracle

H = np.array([0.160102397974, 0.603829269797, 0.724308528438, 0.138428145901, -0.242294887066,
              -0.032244869585, 0.077571493840, -0.006241490213, -0.012580751999, 0.003335725285])
G = np.array([(-1.0) ** (j + 1) * H[9 - j] for j in range(10)])
SIZES = (17, 33, 257, 512)


def numpy_pyramid(x):
    """In-place pyramid of one 512-sample window: [a6 d6 d5 d4 d3 d2 d1], periodic extension,
    one level while the approximation has at least 10 samples (512 -> ... -> 16 -> 8 + 8)."""
    out = np.array(x, dtype=np.float64)
    n = out.size
    while n >= 10:
        idx = (2 * np.arange(n // 2)[:, None] + np.arange(10)[None, :]) % n
        taps = out[:n][idx]
        out[:n] = np.concatenate([taps @ H, taps @ G])
        n //= 2
    return out


def numpy_rows(ep, nfeat, skip):
    n, C, _ = ep.shape
    rows = np.empty((n, C * nfeat))
    for e in range(n):
        for c in range(C):
            rows[e, c * nfeat:(c + 1) * nfeat] = numpy_pyramid(ep[e, c, skip:skip + 512])[:nfeat]
    return rows / np.sqrt(np.sum(rows * rows, axis=1, keepdims=True))


@pytest.fixture(scope="module")
def epochs():
    ep = 30.0 * np.random.default_rng(17).standard_normal((4, 3, 750))
    ep.setflags(write=False)
    return ep


@pytest.mark.parametrize("nfeat", SIZES)
@pytest.mark.parametrize("skip", [0, 175])
def test_oracle_pyramid_against_numpy(epochs, nfeat, skip):
    got = oracle.extract_features(epochs, nfeat=nfeat, skip=skip, faithful=True)
    want = numpy_rows(epochs, nfeat, skip)
    assert got.shape == (4, 3 * nfeat)
    err = float(np.max(np.abs(got - want)))
    print(f"nfeat={nfeat} skip={skip}: max |oracle - numpy| = {err:.3e}")
    assert err <= 1e-13


@pytest.mark.parametrize("nfeat", SIZES)
def test_oracle_faithful_and_restated_agree(epochs, nfeat):
    a = oracle.extract_features(epochs, nfeat=nfeat, faithful=True)
    b = oracle.extract_features(epochs, nfeat=nfeat, faithful=False)
    assert a.tobytes() == b.tobytes()


def test_wide_rows_extend_the_narrow_ones(epochs):
    """The first 16 coefficients of a channel are a6 ++ d6 whatever the feature size: the wide
    row, cut back to 16 per channel and renormalised, is the nfeat = 16 row (to rounding)."""
    wide = oracle.extract_features(epochs, nfeat=512).reshape(4, 3, 512)[:, :, :16].reshape(4, 48)
    wide = wide / np.sqrt(np.sum(wide * wide, axis=1, keepdims=True))
    assert np.max(np.abs(wide - oracle.extract_features(epochs, nfeat=16))) <= 1e-13


def test_feature_dimension_without_a_device():
    wt = fx.WaveletTransform()
    wt.setFeatureSize(512)
    assert wt.getFeatureDimension() == 1536
    assert fx.WaveletTransform(8, 512, 175, 32).getFeatureDimension() == 96
