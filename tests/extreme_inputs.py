"""Inputs shared by test_oracle_extremes.py (CPU: pins the oracle on them) and
test_gpu_extremes.py (GPU: compares the device with the oracle on them).  Not a test module.

Every recording is small: 9 to 17 markers 1000 frames apart (no two epochs share a frame), at
most 19,000 frames; a sub-tile of the kernels is 8 epochs, so each case has a full and a ragged
one.  All arrays are built from fixed seeds and never modified by the tests (poison() copies).
"""
import numpy as np

SPACING = 1000


def positions(n):
    """n marker positions 1000 (+1 for odd ones: both window alignments) frames apart."""
    return np.arange(1, n + 1, dtype=np.int64) * SPACING + np.arange(n) % 2


def frames(n):
    return SPACING * n + 2000


# ---- A: float32 recordings with one poisoned epoch ------------------------------------------------
N_A = 13                     # sub-tiles of 8 and 5 epochs
SLOTS = (3, 11)              # the poisoned epoch: in the full sub-tile, in the ragged last one
POISONS = ("nan", "inf", "inf_pair", "negzero")
PLACES = ("baseline", "window", "outside", "past")
COLS3, RES3 = [0, 1, 2], [1.0, 0.5, 2.5]
COLS5, RES5 = [6, 1, 3, 0, 4], [0.1, 0.5, 1.0, 0.0488281, 2.5]   # ct = 7


def float_recording(n=N_A, ct=7, seed=5):
    rng = np.random.default_rng(seed)
    return (50.0 * rng.standard_normal((frames(n), ct))).astype(np.float32)


def place_range(p, place):
    """Frames of marker p's cut: the 100 baseline frames, the 512-sample window, a stretch of the
    epoch outside both, and a stretch just past the epoch (read by no epoch)."""
    return {"baseline": (p - 100, p), "window": (p + 175, p + 687),
            "outside": (p + 690, p + 750), "past": (p + 750, p + 790)}[place]


def poison(rec, p, kind, place):
    """A copy of rec with the poison in marker p's `place`: one NaN, one +Inf, a +Inf and a -Inf
    (column 1, selected by every path), or -0.0 over the whole stretch in every column."""
    out = rec.copy()
    lo, hi = place_range(int(p), place)
    a, b = lo + (hi - lo) // 3, lo + 2 * (hi - lo) // 3
    if kind == "negzero":
        out[lo:hi, :] = -0.0
    elif kind == "nan":
        out[a, 1] = np.nan
    elif kind == "inf":
        out[a, 1] = np.inf
    elif kind == "inf_pair":
        out[a, 1] = np.inf
        out[b, 1] = -np.inf
    else:
        raise ValueError(kind)
    return out


# ---- B: float32 magnitudes ------------------------------------------------------------------------
MAGNITUDES = ("subnormal", "near_overflow", "flt_max", "overflow")


def float_magnitude(kind):
    """subnormal: samples ~5e-40, so every product, baseline and difference is an fp32 subnormal;
    near_overflow: peak sample 2e37, products up to 5e37 (FLT_MAX = 3.4e38; the 100-term baseline
    sums stay finite, asserted on the CPU); flt_max: peak sample 3.3e38, finite products in the
    res <= 1 channels whose baseline sums overflow, so the epochs hold +-Inf; overflow: |sample| =
    3e38, so the products of the res = 2.5 channel are +-Inf and its baseline Inf - Inf."""
    base = float_recording()
    if kind == "subnormal":
        return base * np.float32(1e-41)
    if kind == "near_overflow":
        return (base / np.abs(base).max() * np.float32(2e37)).astype(np.float32)
    if kind == "flt_max":
        return (base / np.abs(base).max() * np.float32(3.3e38)).astype(np.float32)
    if kind == "overflow":
        return np.where(base < 0, np.float32(-3e38), np.float32(3e38)).astype(np.float32)
    raise ValueError(kind)


# ---- C: int16 recordings with edge resolutions ----------------------------------------------------
RES_SETS = {   # name -> (resolutions of a 3-channel selection, sample kind)
    "1e-42": ((1e-42,) * 3, "moderate"),
    "subnormal_mix": ((1e-39, 1e-40, 1e-41), "moderate"),
    "zero_one": ((0.0, 0.1, 0.1), "moderate"),
    "zero_all": ((0.0,) * 3, "moderate"),
    "negative": ((-0.1, 0.1, -2.5), "moderate"),
    "1e34": ((1e34,) * 3, "moderate"),
    "2e34_full_scale": ((2e34,) * 3, "full_scale"),
}


def res_for(name, C):
    r = RES_SETS[name][0]
    return [r[i % 3] for i in range(C)]


def int16_recording(n, ct, kind, seed=9):
    """moderate: noise of 100 counts, |raw| <= 400 (1e34 * 400 and its 100-term sums stay finite
    in fp32); full_scale: the same with runs of +32767 / -32768 in the window of epoch 2, the
    baseline of epoch 5 and both in epoch 10 (where n has them): with res = 2e34 those products
    overflow fp32 and the other epochs stay finite."""
    rng = np.random.default_rng(seed + ct)
    raw = np.clip(np.rint(100.0 * rng.standard_normal((frames(n), ct))), -400, 400).astype(np.int16)
    if kind == "full_scale":
        pos = positions(n)
        raw[pos[2] + 300:pos[2] + 310, :] = 32767
        raw[pos[5] - 60:pos[5] - 50, :] = -32768
        if n > 10:
            raw[pos[10] + 200:pos[10] + 204, :] = 32767
            raw[pos[10] + 400:pos[10] + 404, :] = -32768
    return raw


def flat_recording(n, ct, seed=11):
    """A rhythm on a DC level with every second marker's cut held constant: the a-priori test of
    the fma guard fails those rows (more than 1/16 of the launch), which switches the window
    kernels of the next launches on that context to their tracking variant."""
    rng = np.random.default_rng(seed)
    nf = frames(n)
    t = np.arange(nf)[:, None]
    raw = (-25000 + 2000 * np.sin(2 * np.pi * 3 * t / 1000 + np.arange(ct)[None, :])
           + rng.integers(-300, 300, size=(nf, ct))).astype(np.int64)
    pos = positions(n)
    for k in range(0, n, 2):
        raw[pos[k] - 100:pos[k] + 750] = raw[pos[k] - 100]
    return raw.astype(np.int16), pos


# ---- D: double epochs, scaled by powers of two ----------------------------------------------------
D_SHAPES = [(n, C) for C in (1, 3, 32) for n in (9, 33)]
K_INVARIANT = (-400, -100, 100, 400)   # test_oracle_extremes.py shows the oracle invariant here
K_OVERFLOW, K_UNDERFLOW = 505, -530    # the ends: the oracle alone is the judge


def double_epochs(n, C, seed=21):
    rng = np.random.default_rng(seed + 100 * C + n)
    return 50.0 * rng.standard_normal((n, C, 750))


def scaled(ep, k):
    return np.ldexp(ep, k)   # exact: no input is near the ends of the double range


def poisoned_epochs(ep):
    """(epochs, poisoned indices): a NaN in epoch 2's window, an all-zero epoch 5 and a +Inf in the
    last epoch's window (the ragged sub-tile)."""
    out = ep.copy()
    n, C, _ = out.shape
    out[2, 0, 300] = np.nan
    out[5] = 0.0
    out[n - 1, C - 1, 400] = np.inf
    return out, (2, 5, n - 1)
