"""The oracle on non-finite, subnormal and extreme-magnitude inputs (CPU only): the judge of
test_gpu_extremes.py is pinned here, on that module's own inputs (extreme_inputs.py), before it
judges.

* oracle.decode_epochs / process_recording / extract_features equal a plain numpy restatement of
  the same operations bit for bit, NaN positions included: the fp32 decode (multiply, sequential
  sum of 100, / 100f, subtract, widen) and the unfused cascade with the sequential normalisation.
  numpy does not fuse, flush subnormals or reorder, so this shows the C oracle (gcc -O3) does not
  either on these inputs.
* Scaling double epochs by 2^k is exact; the oracle's rows are bit-identical to the unscaled rows
  for the k of K_INVARIANT, on every shape the GPU module uses.
* At the ends the oracle is the only judge, and what it does there is stated as fact: at 2^505
  every row's sum of squares overflows (norm = Inf: every feature exactly 0.0), at 2^-530 the
  squares are subnormal and the rows drift from the unscaled ones.
"""
import numpy as np
import pytest

import extreme_inputs as xi
from oracle import oracle

H_LITERALS = [0.160102397974, 0.603829269797, 0.724308528438, 0.138428145901, -0.242294887066,
              -0.032244869585, 0.077571493840, -0.006241490213, -0.012580751999, 0.003335725285]
H64 = np.array(H_LITERALS)
G64 = np.array([H64[9 - j] if j & 1 else -H64[9 - j] for j in range(10)])


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(got, want):
    """The same NaN positions, and every other value bit-equal (sign of zero, +-Inf)."""
    got, want = np.asarray(got), np.asarray(want)
    nan = np.isnan(want)
    return (got.shape == want.shape and np.array_equal(np.isnan(got), nan)
            and np.array_equal(bits(got)[~nan], bits(want)[~nan]))


# ---- the numpy restatement -----------------------------------------------------------------------
def np_decode(raw, cols, res, pos):
    """double[n][C][750]: fl32(raw * r) for the 850 frames from pos - 100 (0 past the end), the
    sequential fp32 sum of the first 100, / 100f, the subtraction, the widening."""
    pos = np.asarray(pos, dtype=np.int64)
    idx = pos[:, None] - 100 + np.arange(850)[None, :]
    inside = idx < raw.shape[0]
    with np.errstate(all="ignore"):
        smp = raw[np.minimum(idx, raw.shape[0] - 1)][:, :, list(cols)].astype(np.float32)
        seg = smp * np.asarray(res, dtype=np.float32)[None, None, :]
        seg = np.where(inside[:, :, None], seg, np.float32(0.0))
        b = np.zeros((len(pos), len(cols)), dtype=np.float32)
        for i in range(100):
            b = b + seg[:, i, :]
        b = b / np.float32(100)
        seg = seg - b[:, None, :]
    assert seg.dtype == np.float32 and b.dtype == np.float32
    return np.ascontiguousarray(seg[:, 100:, :].transpose(0, 2, 1)).astype(np.float64)


def np_cascade(x):
    """a6 || d6 of windows x[M][512], unnormalised: each tap one rounded multiply and one rounded
    add, j = 0..9, periodic (the form of test_guard_bound.py cascade_unnormalised)."""
    a = np.asarray(x, dtype=np.float64)
    for level in range(6):
        n = a.shape[1]
        idx = (2 * np.arange(n // 2)[:, None] + np.arange(10)[None, :]) % n
        lo = a[:, idx[:, 0]] * H64[0]
        hi = a[:, idx[:, 0]] * G64[0]
        for j in range(1, 10):
            lo = lo + a[:, idx[:, j]] * H64[j]
            hi = hi + a[:, idx[:, j]] * G64[j]
        if level == 5:
            return np.concatenate([lo, hi], axis=1)
        a = lo


def np_features(epochs):
    """Rows [n][16 C]: the cascade per channel, sqrt of the sequential sum of squares, division."""
    n, C, _ = epochs.shape
    with np.errstate(all="ignore"):
        f = np_cascade(epochs[:, :, 175:687].reshape(n * C, 512)).reshape(n, C * 16)
        acc = np.zeros(n)
        for i in range(C * 16):
            acc = acc + f[:, i] * f[:, i]
        return f / np.sqrt(acc)[:, None]


def check_recording(raw, cols, res, pos):
    """The oracle against the restatement on one recording; returns the oracle's (epochs, rows)."""
    ep = oracle.decode_epochs(raw, cols, res, pos)
    assert same(ep, np_decode(raw, cols, res, pos))
    rows = oracle.process_recording(raw, cols, res, pos)
    assert same(rows, np_features(ep))
    assert same(rows, oracle.extract_features(ep))
    return ep, rows


def unit_norm(rows):
    return np.isfinite(rows).all() and np.allclose(np.sum(rows * rows, axis=1), 1.0, atol=1e-12)


# ---- A, B: float32 recordings --------------------------------------------------------------------
@pytest.mark.parametrize("place", xi.PLACES)
@pytest.mark.parametrize("kind", xi.POISONS)
def test_poisoned_float32_recording(kind, place):
    rec7, pos = xi.float_recording(), xi.positions(xi.N_A)
    clean = oracle.process_recording(rec7, xi.COLS3, xi.RES3, pos)
    assert unit_norm(clean)
    for slot in xi.SLOTS:
        bad = xi.poison(rec7, pos[slot], kind, place)
        ep, rows = check_recording(np.ascontiguousarray(bad[:, :3]), xi.COLS3, xi.RES3, pos)
        check_recording(bad, xi.COLS5, xi.RES5, pos)
        others = [e for e in range(xi.N_A) if e != slot]
        assert same(rows[others], clean[others])          # the poison stays in its epoch
        if place == "past":
            assert same(rows, clean)
        elif kind != "negzero" and place != "outside":
            assert np.isnan(rows[slot]).all()             # baseline or window: the whole row
        if kind == "inf" and place == "outside":
            assert np.isinf(ep[slot]).any() and not np.isnan(ep[slot]).any()


def test_negative_zero_reaches_the_epochs():
    """A recording of -0.0 with a negative resolution: +0 products, a +0 baseline, +0 epochs (and
    -0.0 ones with a positive resolution), kept bit for bit; the rows are 0 / 0 = NaN."""
    rec = np.full((xi.frames(9), 3), -0.0, dtype=np.float32)
    pos = xi.positions(9)
    ep, rows = check_recording(rec, xi.COLS3, [1.0, -0.5, 2.5], pos)
    assert np.isnan(rows).all() and not ep.any()
    assert np.signbit(ep[:, 0]).all() and not np.signbit(ep[:, 1]).any()


@pytest.mark.parametrize("kind", xi.MAGNITUDES)
def test_float32_magnitudes(kind):
    rec7, pos = xi.float_magnitude(kind), xi.positions(xi.N_A)
    ep, rows = check_recording(np.ascontiguousarray(rec7[:, :3]), xi.COLS3, xi.RES3, pos)
    _, rows5 = check_recording(rec7, xi.COLS5, xi.RES5, pos)
    if kind == "subnormal":
        assert 0 < np.abs(ep).max() < float(np.finfo(np.float32).tiny)   # fp32 subnormals
        assert unit_norm(rows) and unit_norm(rows5)
    elif kind == "near_overflow":
        assert np.abs(ep).max() > 1e37
        assert unit_norm(rows) and unit_norm(rows5)
    elif kind == "flt_max":
        assert np.abs(rec7).max() > 3e38 and np.isinf(ep).any()   # overflowed baseline sums
    else:
        assert np.isnan(rows).all() and np.isnan(rows5).all()


# ---- C: int16 recordings with edge resolutions ---------------------------------------------------
@pytest.mark.parametrize("name", list(xi.RES_SETS))
def test_int16_edge_resolutions(name):
    kind = xi.RES_SETS[name][1]
    got = {}
    for n, ct, cols in ((xi.N_A, 3, [0, 1, 2]), (xi.N_A, 5, [4, 0, 2]), (9, 32, list(range(32)))):
        raw, pos = xi.int16_recording(n, ct, kind), xi.positions(n)
        got[ct] = check_recording(raw, cols, xi.res_for(name, len(cols)), pos)
    ep, rows = got[3]
    if name in ("1e-42", "subnormal_mix"):
        sub = ep if name == "1e-42" else ep[:, 2]   # 400 * 1e-39 is normal, 400 * 1e-41 is not
        assert 0 < np.abs(sub).max() < float(np.finfo(np.float32).tiny)
        assert all(unit_norm(r) for _, r in got.values())
    elif name == "zero_all":
        assert np.isnan(rows).all() and not ep.any()
    elif name == "zero_one":
        assert unit_norm(rows) and not rows[:, :16].any()
    elif name in ("negative", "1e34"):
        assert all(unit_norm(r) for _, r in got.values())
    else:  # 2e34: the full-scale runs overflow fp32, the other epochs stay finite
        bad = np.isnan(rows).all(axis=1)
        assert bad.tolist() == [e in (2, 5, 10) for e in range(xi.N_A)]
        assert unit_norm(rows[~bad])


# ---- D: double epochs, scaled --------------------------------------------------------------------
@pytest.mark.parametrize("n,C", xi.D_SHAPES)
def test_scale_invariance_and_the_ends(n, C):
    ep = xi.double_epochs(n, C)
    base = oracle.extract_features(ep)
    assert same(base, np_features(ep)) and unit_norm(base)
    for k in xi.K_INVARIANT:
        s = xi.scaled(ep, k)
        assert np.array_equal(np.ldexp(s, -k), ep)        # the scaling is exact
        assert same(oracle.extract_features(s), base), k
    up = oracle.extract_features(xi.scaled(ep, xi.K_OVERFLOW))
    assert same(up, np_features(xi.scaled(ep, xi.K_OVERFLOW)))
    if C >= 3:
        assert not up.any() and not np.isnan(up).any()   # norm = Inf: every feature exactly 0.0
    else:  # 16 squares: not every row's sum overflows; those that do are all-zero rows
        zero = ~up.any(axis=1)
        assert zero.any() and same(up[~zero], base[~zero])
    down = oracle.extract_features(xi.scaled(ep, xi.K_UNDERFLOW))
    assert same(down, np_features(xi.scaled(ep, xi.K_UNDERFLOW)))
    drift = np.abs(down - base).max()
    assert np.isfinite(down).all() and 1e-13 < drift < 1e-6, drift   # subnormal squares
    bad, where = xi.poisoned_epochs(ep)
    rows = oracle.extract_features(bad)
    assert same(rows, np_features(bad))
    assert np.isnan(rows[list(where)]).all()
    others = [e for e in range(n) if e not in where]
    assert same(rows[others], base[others])
