"""Where the conditioning guard's verdict is tested at its decision boundary (DESIGN.md section
10.10).  The fma numerics certify a row when acc = sum f^2 >= K2 * sum_c X_c^2 and recompute it
under EXACT otherwise (csrc/guard.h); the second stage takes X_c = max |x_c| from the row's own
window, and nine kernels measure it with lane arithmetic of their own.  On a flat or a purely
alternating window every subset of lanes, frames, channels and rows gives the same X_c, so this
module builds windows whose verdict depends on a few frames of one channel of one row:

  pair burst      delta + a (-1)^t with frames p, p + 1 raised to delta +- A.  The alternation is in
                  the filters' null space, the step delta gives acc = 512 (delta r)^2 and the pair
                  leaks coef(p) ((A - a) r)^2, coef(p) between 0.36 K2 and 4.2 K2 with period 32 in
                  p.  Tuned so that acc / (K2 X^2) < 1 / m with the true X = A (recomputed) and
                  > m with X = a (a scan that missed the pair would certify).
  single impulse  one frame raised to A at the alternation's own sign: only one of a lane's (min,
                  max) pair carries it.  The bracket is (a / A)^2 wide.

restate() computes (stage 1 fails, stage 2 fails, both ratios) of every row of a call from the
oracle's decode, the float32 baseline fold and tests/test_guard_bound.cascade_unnormalised, in the
form the site's kernel uses; `blind` names one way of measuring less or the wrong thing.  A case is
valid when its verdict under its own blindness differs from its true verdict and every ratio
involved lies at least MARGIN from 1.  Not a test module: tests/test_guard_cases.py proves the
cases, tests/test_gpu_guard_edges.py runs the device on them.
"""
import os
import re
from collections import namedtuple

import numpy as np

import layout_cases as L
import refusal_cases as R
from oracle import oracle
from test_guard_bound import cascade_unnormalised

CSRC = R.CSRC
WIN, SKIP, PRE, POST = L.WIN, 175, R.PRE, R.POST
W0 = PRE + SKIP                    # the window's first frame in a row's block of PRE + POST frames
BLOCK = PRE + POST
SPACING = 1000
MARGIN = 1.05
EPS = 2.0 ** -20
FULL = 32768.0
A_TOP = 30000                      # the burst's amplitude in raw counts


# ---- constants and rules read from the sources ----------------------------------------------------
def _src(name):
    return open(os.path.join(CSRC, name)).read()


def constants():
    guard, fused = _src("guard.h"), _src("fused.hip")

    def one(pattern, text, conv):
        m = re.search(pattern, text)
        assert m, pattern
        return conv(m.group(1))
    sh = re.search(r"const int sh = k <= (\d+) \? (\d+) : k <= (\d+) \? (\d+) : k <= (\d+) \? (\d+) "
                   r": (\d+);", fused)
    assert sh, "channel_x2_rows: lanes-per-row rule"
    v = [int(g) for g in sh.groups()]
    return {
        "k2": one(r"constexpr double kGuardK2Collapsed = ([0-9.eE+-]+);", guard, float),
        "slots": one(r"constexpr int kGuardSlots = (\d+);", guard, int),
        "sub": one(r"constexpr int kSub = (\d+);", fused, int),
        "acc_min": one(r"constexpr double kGuardAccMin = (0x1p[+-]?\d+);", guard, float.fromhex),
        "acc_max": one(r"constexpr double kGuardAccMax = (0x1p[+-]?\d+);", guard, float.fromhex),
        "lanes_rule": [(v[0], 1 << v[1]), (v[2], 1 << v[3]), (v[4], 1 << v[5]), (None, 1 << v[6])],
    }


_C = constants()
K2, SUB, SLOTS = _C["k2"], _C["sub"], _C["slots"]
ACC_MIN, ACC_MAX = _C["acc_min"], _C["acc_max"]


def lanes_per_row(k):
    """fused.hip channel_x2_rows: lanes a flagged row gets when k rows of a sub-tile are flagged."""
    for kmax, lanes in _C["lanes_rule"]:
        if kmax is None or k <= kmax:
            return lanes


# ---- the sites ------------------------------------------------------------------------------------
# form: "sum"      stage 1 a-priori, stage 2 (1 + 2^-20) sum_c X_c^2          (int16)
#       "3max"     stage 1 a-priori, stage 2 3 (1 + 2^-20) max_c X_c^2        (recheck_c3)
#       "measured" the one test is sum_c X_c^2, measured                      (float32 recordings)
#       "epochs"   the same, with guard_acc_out_of_range                      (caller's epochs)
Site = namedtuple("Site", "n kernel form where")
SITES = {
    1: Site(1, "window_kernel", "sum", "fused.hip channel_x2_rows (scan), guard.h ladder_reduce"),
    2: Site(2, "window_kernel", "sum", "fused.hip TRK: ymax, dwt8.h signal_x2 / group8_max"),
    3: Site(3, "cut_features_c3_kernel", "3max", "rows.h recheck_c3 from the recording"),
    4: Site(4, "window_wide_kernel", "sum", "guard.h guard_measured_x2_wave, int16"),
    5: Site(5, "window_wide_kernel", "measured", "wide.hip signal_x2(ym), float32"),
    6: Site(6, "window_c32_kernel", "sum", "guard_measured_x2_wave at C = 32 (scan)"),
    7: Site(7, "window_c32_kernel", "sum", "wide.hip TRACK: sh.gxm[], guard_tracked_x2_wave"),
    8: Site(8, "cut_write_lds*_kernel", "sum", "cut.hip staged_features: gsmp / signal_x2"),
    9: Site(9, "features_from_epochs_kernel", "epochs", "extract.hip group8_max(xm), sx"),
}


def form_of(site, dtype):
    """The form of a site's test for recordings of `dtype`: the one-pass staged writers (site 8)
    take the measured sum alone for float32 recordings, as window_wide_kernel (site 5) does."""
    if site == 8 and dtype is not None and np.dtype(dtype) != np.int16:
        return "measured"
    return SITES[site].form


# ---- the restatement ------------------------------------------------------------------------------
_M = None


def _linear():
    """The EXACT cascade as a 16 x 512 matrix (for the case search only: the restated verdicts
    take acc from cascade_unnormalised itself)."""
    global _M
    if _M is None:
        eye = np.eye(WIN)
        _M = np.stack([cascade_unnormalised(eye[i]) for i in range(WIN)], axis=1)
    return _M


_acc_cache = {}


def window_acc(x):
    key = x.tobytes()
    if key not in _acc_cache:
        with np.errstate(over="ignore", under="ignore", invalid="ignore"):
            f = cascade_unnormalised(x)
            _acc_cache[key] = float(np.sum(f * f))
    return _acc_cache[key]


def baselines(raw, cols, res, pos):
    """The float32 fold of OffLineDataProvider's baseline, operation for operation."""
    r32 = np.asarray(res, dtype=np.float32)
    pos = np.asarray(pos, dtype=np.int64)
    b = np.zeros((len(pos), len(cols)), dtype=np.float32)
    for i in range(PRE):
        v = raw[pos - PRE + i][:, cols].astype(np.float32)
        b = b + v * r32
    return b / np.float32(PRE)


def apriori_x2(res, b):
    """guard.h guard_x2_int16, summed over the channels: [n]."""
    X = (FULL * np.abs(np.asarray(res, np.float32).astype(np.float64))[None, :]
         + np.abs(b.astype(np.float64))) * (1.0 + EPS)
    return np.sum(X * X, axis=1)


def measured_x2(form, x, blind=None):
    """The site's second-stage sum for one row, x = [C][512] decoded samples."""
    kind = blind[0] if blind else None
    if kind == "frames":
        keep = np.ones(WIN, dtype=bool)
        keep[blind[1]:blind[2]] = False
        x = x[:, keep]
    X2 = np.max(np.abs(x), axis=1) ** 2
    if form == "epochs":     # extract.hip: doubles below 2^-537 square to 0, X^2 is kept != 0
        X2 = np.where((X2 == 0) & (np.max(np.abs(x), axis=1) != 0), 2.0 ** -1022, X2)
    if kind == "channel":
        X2 = np.delete(X2, blind[1])
    if kind == "repeat":
        X2 = np.concatenate([X2, [X2[blind[1]]] * blind[2]])
    if kind == "sum_as_3max":
        form = "3max"
    if kind == "3max_as_sum":
        form = "sum"
    if form == "3max":
        return 3.0 * (1.0 + EPS) * float(np.max(X2)) if len(X2) else 0.0
    s = float(np.sum(X2))
    return s * (1.0 + EPS) if form == "sum" else s


def fails(acc, s):
    """guard.h guard_fails: NaN fails."""
    return not (acc >= K2 * s)


def ratio(acc, s):
    with np.errstate(over="ignore", invalid="ignore"):
        return float("inf") if s == 0 else acc / (K2 * s)


def out_of_range(acc, s):
    """guard.h guard_acc_out_of_range."""
    return not ((ACC_MIN <= acc <= ACC_MAX) or (acc == 0.0 and s == 0.0))


Verdict = namedtuple("Verdict", "stage1_fails stage2_fails ratio1 ratio2")


def _row_verdict(form, x, res, b, blind=None, x_other=None, b_other=None):
    """x [C][512] this row's decoded window, b [C] its baselines."""
    acc = sum(window_acc(np.ascontiguousarray(xc)) for xc in x)
    kind = blind[0] if blind else None
    xm = x_other if kind == "row" else x
    s2 = measured_x2(form, xm, blind)
    if form in ("measured", "epochs"):
        f = fails(acc, s2) or (form == "epochs" and out_of_range(acc, s2))
        return Verdict(f, f, ratio(acc, s2), ratio(acc, s2))
    r1 = np.asarray(res, dtype=np.float32)
    if kind == "res":
        r1 = np.full(len(res), r1[blind[1]], dtype=np.float32)
    b1 = b_other if kind == "base" else b
    s1 = float(apriori_x2(r1, b1[None, :])[0])
    f1 = fails(acc, s1)
    return Verdict(f1, f1 and fails(acc, s2), ratio(acc, s1), ratio(acc, s2))


def verdict(site, raw, layout, pos, row, blind=None):
    """The restated verdict of row `row` of a call at site `site`: raw and positions with a
    refusal_cases.Layout, or (layout None, pos None) epochs [n][C][750] for site 9.  blind:
    ("frames", lo, hi) hides those window frames from the measurement; ("channel", c) drops a
    channel; ("repeat", c, k) counts channel c k more times; ("row", e2) measures row e2's
    window; ("res", c2) / ("base", e2) take channel c2's resolution for every channel / epoch e2's
    baselines in stage 1; ("sum_as_3max",) / ("3max_as_sum",) swap the two forms;
    ("past_end", raw2) decodes from the longer recording raw2."""
    form = form_of(site, layout.dtype if layout else None)
    if layout is None:
        ep, b = np.asarray(raw, dtype=np.float64), None
        res = None
    else:
        src = blind[1] if blind and blind[0] == "past_end" else raw
        rows = [row] + ([blind[1]] if blind and blind[0] in ("row", "base") else [])
        p = np.asarray(pos, dtype=np.int64)[rows]
        ep = oracle.decode_epochs(src, layout.cols, layout.res, p)
        b = baselines(src, layout.cols, layout.res, p)
        res = layout.res
        x = ep[:, :, SKIP:SKIP + WIN]
        return _row_verdict(form, x[0], res, b[0], blind, x[-1], b[-1])
    x = ep[:, :, SKIP:SKIP + WIN]
    other = x[blind[1]] if blind and blind[0] == "row" else None
    return _row_verdict(form, x[row], res, None, blind, other)


def restate(group):
    """Every row's true verdict: a list of Verdict, and (checked, rechecked, recomputed)."""
    form = form_of(group.site, group.layout.dtype)
    if group.entry == "extract":
        x = np.asarray(group.epochs, dtype=np.float64)[:, :, SKIP:SKIP + WIN]
        out = [_row_verdict(form, x[e], None, None) for e in range(len(x))]
    else:
        raw = group.raw[:group.n_frames]
        ep = oracle.decode_epochs(raw, group.layout.cols, group.layout.res, group.pos)
        b = baselines(raw, group.layout.cols, group.layout.res, group.pos)
        x = ep[:, :, SKIP:SKIP + WIN]
        out = [_row_verdict(form, x[e], group.layout.res, b[e]) for e in range(len(x))]
    counters = (len(out), sum(v.stage1_fails for v in out), sum(v.stage2_fails for v in out))
    return out, counters


# ---- windows --------------------------------------------------------------------------------------
def _decode32(w, r):
    """fl(fl(raw * r) - 0) as doubles, w [512] raw counts or float32 samples."""
    return (w.astype(np.float32) * np.float32(r)).astype(np.float64)


def burst_window(kind, p, a, delta, A=A_TOP, q=WIN):
    """One channel's window in raw units: delta + a (-1)^t, the pair (p, p + 1) at delta +- A or
    the impulse p at the alternation's sign, zero from frame q on (the recording's end)."""
    t = np.arange(WIN)
    sgn = np.where(t % 2 == 0, 1.0, -1.0)
    w = delta + a * sgn
    if kind == "pair":
        w[p], w[p + 1] = delta + A * sgn[p], delta + A * sgn[p + 1]
    elif kind == "impulse":
        w[p] = delta + A * sgn[p]
    w[q:] = 0.0
    return w


def other_delta(delta, res, cb, c, flt):
    d = min(delta * float(np.float32(res[cb])) / float(np.float32(res[c])), OTHER_MAX)
    return d if flt else float(np.rint(d))


Tuned = namedtuple("Tuned", "win a delta A ratio_true ratio_blind")
_tune_cache = {}
A_PAIR = (0.7, 0.0, 0.8, 0.6, 0.5, 0.9, 0.4, 0.3)     # a / A, in the order tried
DELTA_MAX, OTHER_MAX = 48.0, 2000.0


def tune(form, res, cb, kind, p, blind, flt=False, q=WIN, side="below", A=A_TOP, int16=True):
    """Searches delta >= 1 and a for the burst in channel cb, the other channels carrying the step
    alone (scaled by resolution): the first hit whose true ratio lies MARGIN below 1 and whose
    blind ratio MARGIN above (side "below"; "above": the other way round).  Pair: a from A_PAIR,
    then delta.  Impulse: the bracket is (a / A)^2 wide, so delta, then a count by count below
    A / MARGIN.  None if there is no hit."""
    key = (form, tuple(res), cb, kind, p, blind, flt, q, side, A, int16)
    if key in _tune_cache:
        return _tune_cache[key]
    M = _linear()
    C = len(res)
    deltas = np.arange(1.0, DELTA_MAX, 0.25 if flt else 1.0)
    s1 = float(apriori_x2(res, np.zeros((1, C), np.float32))[0])

    def others(delta, spread=True):
        win = np.stack([burst_window("none", 0, 0.0,
                                     other_delta(delta, res, cb, c, flt) if spread else 0.0, A, q)
                        for c in range(C)])
        x = np.stack([_decode32(win[c], res[c]) for c in range(C)])
        f = np.delete(x, cb, axis=0) @ M.T
        return win, x, float(np.sum(f * f))

    def attempt(a, delta, base):
        win, x, acc = base[0].copy(), base[1].copy(), base[2]
        win[cb] = burst_window(kind, p, a, delta, A, q)
        x[cb] = _decode32(win[cb], res[cb])
        f = M @ x[cb]
        acc += float(f @ f)
        rt = ratio(acc, measured_x2(form, x))
        rb = ratio(acc, measured_x2(form, x, blind))
        lo, hi = (rt, rb) if side == "below" else (rb, rt)
        ok = lo * MARGIN <= 1.0 and hi >= MARGIN
        if ok and int16 and form in ("sum", "3max"):   # stage 1 must fail, with the margin
            ok = ratio(acc, s1) * MARGIN <= 1.0
        return Tuned(win, float(a), float(delta), A, rt, rb) if ok else None

    hit = None
    if kind == "impulse":
        # the step in every channel first; in the burst channel alone where that is too coarse
        for spread, delta in [(True, d) for d in deltas[:8]] + [(False, d) for d in deltas[:16]]:
            base = others(delta, spread)
            for a in range(int(A / MARGIN) - 1, int(0.93 * A), -2):
                hit = attempt(a, delta, base)
                if hit:
                    break
            if hit:
                break
    else:
        bases = {}
        for frac in A_PAIR:
            for delta in deltas:
                if delta not in bases:
                    bases[delta] = others(delta)
                hit = attempt(np.rint(frac * A), delta, bases[delta])
                if hit:
                    break
            if hit:
                break
    _tune_cache[key] = hit
    return hit


def tune_step(res, lo_x2, hi_x2, flt=False):
    """A flat step delta (others scaled by resolution) with MARGIN K2 lo_x2 <= acc <= K2 hi_x2 /
    MARGIN: the probes of stage 1."""
    M = _linear()
    C = len(res)
    for delta in (np.arange(0.25, 4000.0, 0.25) if flt else np.arange(1.0, 4000.0)):
        win = np.stack([burst_window("none", 0, 0.0, other_delta(delta, res, 0, c, flt))
                        for c in range(C)])
        x = np.stack([_decode32(win[c], res[c]) for c in range(C)])
        f = x @ M.T
        acc = float(np.sum(f * f))
        if acc >= MARGIN * K2 * lo_x2 and acc * MARGIN <= K2 * hi_x2:
            return win
    return None


# ---- blocks: the PRE + POST frames of one row, [BLOCK][C] in raw units ----------------------------
def block_from_window(win, res):
    """Window `win` [C][512]; a channel that alternates keeps alternating before and after it (the
    baseline of 50 pairs is exactly 0), the others hold their step after the stimulus."""
    C = win.shape[0]
    blk = np.zeros((BLOCK, C))
    i = np.arange(BLOCK)
    for c in range(C):
        w = win[c]
        amp = (np.median(w[0::2][:8]) - np.median(w[1::2][:8])) / 2.0
        mid = (np.median(w[0::2][:8]) + np.median(w[1::2][:8])) / 2.0
        sgn = np.where((i - W0) % 2 == 0, 1.0, -1.0)
        blk[:, c] = amp * sgn
        blk[PRE:, c] += mid
        blk[W0:W0 + WIN, c] = w
    return blk


def ordinary_block(res, level=0.0):
    """A rhythm and a step a fifth of full scale: certified at stage 1.  level: the pre-stimulus
    DC in raw counts (|b| = level r)."""
    C = len(res)
    i = np.arange(BLOCK)[:, None]
    blk = 1500.0 * np.sin(2 * np.pi * 3 * i / 1000.0 + np.arange(C)[None, :])
    blk[PRE:] += 6000.0
    blk[:PRE] = level
    return np.rint(blk)


def flat_block(res, level):
    """test_gpu_guard.flat_recording's construction: the whole span at one level, which decodes to
    a rounding residue: fails stage 1, certified at stage 2."""
    C = len(res)
    blk = np.full((BLOCK, C), level) * (1.0 + np.arange(C)[None, :] / 512.0)
    return np.rint(blk) if abs(level) >= 1 else blk


# ---- groups ---------------------------------------------------------------------------------------
# A group is one device call.  case: name, site, row, blind, stage (1 or 2: the stage whose verdict
# the blindness flips), what it is for.
Case = namedtuple("Case", "name site row blind stage purpose")
Group = namedtuple("Group", "name site entry layout raw n_frames pos epochs cases track dtype",
                   defaults=(None, (), False, None))
FILL = 31000.0                     # the unselected columns alternate at this amplitude


class Builder:
    def __init__(self, name, site, entry, layout, track=False):
        self.name, self.site, self.entry, self.layout, self.track = name, site, entry, layout, track
        self.blocks, self.cases, self.missing = [], [], []

    @property
    def flt(self):
        return np.dtype(self.layout.dtype) != np.int16

    @property
    def form(self):
        return form_of(self.site, self.layout.dtype)

    def add(self, blk):
        self.blocks.append(blk)
        return len(self.blocks) - 1

    def case(self, name, row, blind, purpose, stage=2):
        self.cases.append(Case("%s/%s" % (self.name, name), self.site, row, blind, stage, purpose))

    def ordinary(self, level=0.0):
        return self.add(ordinary_block(self.layout.res, level))

    def flat(self):
        # caller-supplied epochs have no baseline to cancel the level: a tiny one instead
        return self.add(flat_block(self.layout.res, 1e-3 if self.entry == "extract" else -25000.0))

    def pad_to_tile(self):
        while len(self.blocks) % SUB:
            self.ordinary()

    def burst(self, name, cb, kind, p, blind, purpose, side="below", A=A_TOP, q=WIN, keep=True):
        """A tuned burst row; a search without a hit is recorded (the CPU test fails on it,
        except for the single impulses, which are kept where they reach the margin)."""
        t = tune(self.form, self.layout.res, cb, kind, p, blind, self.flt, q, side, A,
                 int16=not self.flt)
        if t is None:
            if keep:
                self.missing.append("%s/%s" % (self.name, name))
            return None
        row = self.add(block_from_window(t.win, self.layout.res))
        self.case(name, row, blind, purpose)
        return row

    def finish(self, n_frames=None):
        lay = self.layout
        n = len(self.blocks)
        total = SPACING * n + PRE + POST
        i = np.arange(total)[:, None]
        raw = FILL * np.where(i % 2 == 0, 1.0, -1.0) * np.ones((1, lay.ct))
        raw[:, lay.cols] = 0.0
        pos = PRE + SPACING * np.arange(n, dtype=np.int64)
        for k, blk in enumerate(self.blocks):
            raw[pos[k] - PRE:pos[k] + POST, lay.cols] = blk
        if not self.flt:
            assert np.all(np.abs(raw) <= 32767) and np.all(raw == np.rint(raw))
        raw = np.ascontiguousarray(raw.astype(lay.dtype))
        raw.setflags(write=False)
        pos.setflags(write=False)
        return Group(self.name, self.site, self.entry, lay, raw,
                     total if n_frames is None else n_frames, pos, None, tuple(self.cases),
                     self.track, np.dtype(lay.dtype).name)


# ---- layouts --------------------------------------------------------------------------------------
Layout = R.Layout
RES3 = [0.0488281, 1.0, 0.001]                     # three orders apart
LAY_C3 = Layout(np.int16, 3, [2, 0, 1], [0.1, 0.1, 0.1])
LAY_C3_RES = Layout(np.int16, 3, [1, 2, 0], RES3)
LAY_WIDE5 = Layout(np.int16, 7, [6, 1, 3, 0, 4], [0.1, 0.5, 0.001, 0.0488281, 1.0])
LAY_WIDE7 = Layout(np.int16, 7, [6, 1, 3, 0, 4, 2, 5], [0.1, 0.5, 0.001, 0.0488281, 1.0, 0.01, 0.1])
LAY_WIDE_F32 = Layout(np.float32, 4, [3, 1, 0], [1.0, 0.5, 0.001])
LAY_C32 = Layout(np.int16, 32, list(range(32)),
                 [(0.1, 0.5, 0.001, 0.0488281, 1.0)[c % 5] for c in range(32)])
_F32 = R.layouts()
LAY_PACKED = Layout(np.int16, 7, _F32["f32/int16_7"].cols[:5], [0.1, 0.5, 1.0, 0.001, 0.0488281])
LAY_LDS_I16 = Layout(np.int16, 32, _F32["f32/int16_32"].cols[:5], [0.1, 0.5, 1.0, 0.001, 0.0488281])
LAY_LDS_F32 = Layout(np.float32, 7, _F32["f32/float32_7"].cols[:5],
                     [1.0, 0.5, 2.5, 0.001, 0.0488281])


def kernels_of(group):
    """The kernels the restated dispatch gives for a group's call (refusal_cases / layout_cases)."""
    if group.entry == "extract":
        C = group.epochs.shape[1]
        return ("features_from_epochs_kernel", "rows_out" if L.rows_out(C, 16) else "rows_lds")
    lay = group.layout
    fmt = R.fmt_of(lay.dtype)
    if group.entry == "features":
        return R.features_route(fmt, lay.ct, len(lay.cols))
    return R.one_pass_writer(fmt, lay.ct, len(lay.cols))


# ---- where each site's lanes look -----------------------------------------------------------------
LANES = (0, 1, 2, 4, 8, 16, 32)


def slice_lanes(lanes):
    return sorted({l for l in LANES if l < lanes} | {lanes - 1})


def scan_slices(lanes):
    """(lane, p, lo, hi): the first and the last pair of the contiguous run lane `lane` of `lanes`
    scans (channel_x2_rows, recheck_c3 at 64 lanes)."""
    fpl = WIN // lanes
    return [(l, p, l * fpl, (l + 1) * fpl) for l in slice_lanes(lanes)
            for p in (l * fpl, (l + 1) * fpl - 2)]


def segment_slices():
    """Sites 2, 5, 7, 9 (a lane decodes its segment's 64 samples and the next segment's first 8 as
    halo): the pair in each segment outside the first 8 frames, and once more inside them."""
    out = []
    for s in range(8):
        out.append((s, 64 * s + 30, 64 * s + 8, 64 * s + 64, "own"))
        out.append((s, 64 * s + 2, 64 * s, 64 * s + 8, "halo"))
    return out


def strided_pairs():
    """Sites 4, 6, 8 (lane l of a channel's 16 reads frames l, l + 16, ...): the pair at the head
    of each staged segment (lanes 0 and 1) and at frames 510-511 (lanes 14 and 15)."""
    return [64 * s for s in range(8)] + [510]


IMPULSE_LANES = (0, 1, 2, 4, 8, 15)


def impulse_frame(lane):
    """The frame = lane (mod 16) at which a single impulse leaks least."""
    M = _linear()
    f = np.arange(lane, WIN, 16)
    return int(f[np.argmin(np.sum(M[:, f] ** 2, axis=0))])


# ---- the standard rows of a group -----------------------------------------------------------------
def add_row_identity(b, cb=0, p=44):
    """A burst row beside a flat row, both orders: the measurement of the neighbour's window
    would certify the burst row."""
    r1 = b.burst("row/burst-then-flat", cb, "pair", p, ("frames", p, p + 2),
                 "burst row before a flat flagged row")
    f1 = b.flat()
    f2 = b.flat()
    r2 = b.burst("row/flat-then-burst", cb, "pair", p, ("frames", p, p + 2),
                 "burst row after a flat flagged row")
    for name, row, other in (("row/next", r1, f1), ("row/previous", r2, f2)):
        if row is not None:
            b.case(name, row, ("row", other), "the neighbouring flagged row's window measured")


def add_channel_identity(b, channels, p=44):
    for cb in channels:
        b.burst("channel/%d" % cb, cb, "pair", p, ("channel", cb),
                "the burst in channel %d alone: a sum without it certifies" % cb)


def add_stage1_probes(b):
    """Stage 1's own b and r: a probe row with b = 0 certified at stage 1 between neighbours whose
    |b| would flag it, and a row that fails stage 1 unless every channel takes channel c2's
    resolution (or the other way round)."""
    res = b.layout.res
    C = len(res)
    level = 30000.0
    x0 = float(apriori_x2(res, np.zeros((1, C), np.float32))[0])
    bl = (np.float32(level) * np.asarray(res, np.float32))[None, :]
    x1 = float(apriori_x2(res, bl)[0])
    win = tune_step(res, x0, x1, b.flt)
    if win is None:
        b.missing.append(b.name + "/stage1/base")
    else:
        n1 = b.ordinary(level)
        probe = b.add(block_from_window(win, res))
        b.ordinary(level)
        b.case("stage1/base", probe, ("base", n1), "b = 0 certified at stage 1; a neighbour's "
               "|b| = %g r would flag it" % level, stage=1)
    r64 = np.asarray(res, np.float32).astype(np.float64)
    for c2 in sorted({0, int(np.argmin(r64)), int(np.argmax(r64))}):
        xc = float(apriori_x2([res[c2]] * C, np.zeros((1, C), np.float32))[0])
        if max(xc, x0) / min(xc, x0) < MARGIN ** 2 * 1.01:
            continue
        win = tune_step(res, min(xc, x0), max(xc, x0), b.flt)
        if win is None:
            b.missing.append(b.name + "/stage1/res%d" % c2)
            continue
        row = b.add(block_from_window(win, res))
        b.case("stage1/res%d" % c2, row, ("res", c2),
               "stage 1 with channel %d's resolution for every channel decides otherwise" % c2,
               stage=1)


def add_strided(b, cb):
    for p in strided_pairs():
        b.burst("stride/pair-%d" % p, cb, "pair", p, ("frames", p, p + 2),
                "pair at frames %d-%d: lanes %d and %d of the channel's DPP row"
                % (p, p + 1, p % 16, (p + 1) % 16))
    for lane in IMPULSE_LANES:
        f = impulse_frame(lane)
        b.burst("stride/impulse-lane%d" % lane, cb, "impulse", f, ("frames", f, f + 1),
                "single impulse at frame %d: lane %d alone holds the extreme" % (f, lane),
                keep=False)


def add_segments(b, cb_of):
    for s, p, lo, hi, what in segment_slices():
        b.burst("segment%d/%s" % (s, what), cb_of(s), "pair", p, ("frames", lo, hi),
                "pair in segment %d, %s" % (s, "seen by lane %d alone" % s if what == "own"
                                            else "in the first 8 frames (the neighbour's halo)"))


# ---- site 1: the fused window kernel's scan -------------------------------------------------------
FLAGGED = {1: None, 2: (0, 7), 3: (0, 3, 7), 4: (0, 2, 5, 7), 5: (0, 1, 3, 5, 7),
           8: (0, 1, 2, 3, 4, 5, 6, 7)}


def _sub_tile(b, flagged, burst_at, make_burst, ne=SUB):
    """One sub-tile of ne epochs: the flagged epochs are flat rows but burst_at, the rest ordinary."""
    for e in range(ne):
        if e == burst_at:
            if make_burst() is None:
                b.ordinary()
        elif e in flagged:
            b.flat()
        else:
            b.ordinary()


def group_site1_lanes():
    b = Builder("c3-scan-lanes", 1, "features", LAY_C3)
    i = 0
    for k in sorted(FLAGGED):
        lanes = lanes_per_row(k)
        for slot in ("first", "last"):
            flagged = FLAGGED[k] or ((0,) if slot == "first" else (SUB - 1,))
            at = flagged[0] if slot == "first" else flagged[-1]
            for lane, p, lo, hi in scan_slices(lanes):
                cb = i % 3
                i += 1
                name = "k%d/%s/lane%d/p%d" % (k, slot, lane, p)
                _sub_tile(b, flagged, at, lambda: b.burst(
                    name, cb, "pair", p, ("frames", lo, hi),
                    "%d flagged rows (%d lanes a row), burst row in the %s slot, epoch %d: pair in "
                    "lane %d's run [%d, %d)" % (k, lanes, slot, at, lane, lo, hi)))
    # a ragged last sub-tile: three epochs, two flagged, the burst row last
    lanes = lanes_per_row(2)
    fpl = WIN // lanes
    _sub_tile(b, (0, 2), 2, lambda: b.burst(
        "ragged/k2/last/lane%d" % (lanes - 1), 1, "pair", WIN - 2, ("frames", WIN - fpl, WIN),
        "ragged sub-tile (ne = 3): burst row in the last slot, pair in the last lane's run"), ne=3)
    return b


def group_site1_identity(site=1, name="c3-scan-identity", track=False):
    b = Builder(name, site, "features", LAY_C3_RES, track)
    add_channel_identity(b, range(3))
    b.burst("form/sum-certifies", 1, "pair", 44, ("sum_as_3max",),
            "certified by the exact sum, not by 3 max: the window kernel takes the sum",
            side="above", A=12000)
    b.pad_to_tile()
    add_row_identity(b, cb=1)
    b.pad_to_tile()
    add_stage1_probes(b)
    b.pad_to_tile()
    if track:
        add_segments(b, lambda s: s % 3)
    return b


def group_site3():
    b = Builder("c3-one-pass", 3, "one_pass", LAY_C3_RES)
    for i, (lane, p, lo, hi) in enumerate(scan_slices(64)):
        b.burst("lane%d/p%d" % (lane, p), i % 3, "pair", p, ("frames", lo, hi),
                "recheck_c3: pair in lane %d's frames [%d, %d)" % (lane, lo, hi))
    add_channel_identity(b, range(3))
    b.burst("form/3max-recomputes", 1, "pair", 44, ("3max_as_sum",),
            "certified by the exact sum, not by 3 max: recheck_c3 takes 3 max", A=12000)
    add_row_identity(b, cb=1)
    add_stage1_probes(b)
    return b


def groups_end(site, entry, name):
    """The recording's end: the burst row is the last epoch, the pair lies in the last two frames
    before n_frames and the window is clipped after it; and the mirror call, whose n_frames ends
    two frames earlier over the same buffer, so that the pair is past the end and never there."""
    q = 302                            # the pair at window frames 300-301: 300 % 32 = 12, low leak
    out = []
    for variant in ("pair-at-end", "ends-before-pair"):
        b = Builder("%s-%s" % (name, variant), site, entry, LAY_C3)
        for _ in range(SUB + 2):
            b.ordinary()
        hidden = ("frames", q - 8, q)
        t = tune(b.form, LAY_C3.res, 1, "pair", q - 2, hidden, False, q)
        if t is None:
            b.missing.append(b.name)
            out.append(b.finish())
            continue
        blk = block_from_window(t.win, LAY_C3.res)
        row = b.add(blk)
        g = b.finish()
        end = int(g.pos[row]) + SKIP + q
        if variant == "pair-at-end":
            b.case("last-lane", row, hidden, "last epoch, the pair in the last two frames before "
                   "n_frames, zero padding after")
            out.append(b.finish(end))
        else:
            b.case("past-end", row, ("past_end", None), "n_frames two frames earlier: the pair "
                   "lies past the end and must read as zero padding")
            out.append(b.finish(end - 2))
    return out


# ---- sites 4, 6, 8: guard_measured_x2_wave --------------------------------------------------------
def group_wide_int16(name, lay, site=4, entry="features"):
    b = Builder(name, site, entry, lay)
    C = len(lay.cols)
    add_strided(b, C - 1)
    add_channel_identity(b, range(C))
    if site == 4:
        extra = (4 - C % 4) % 4        # clamped duplicates of channel C - 1 in the ragged pass
        b.burst("ragged-pass/weight0", C - 1, "pair", 44, ("repeat", C - 1, extra),
                "certified only if the %d clamped duplicates of channel %d weigh 0" % (extra, C - 1),
                side="above", A=12000)
    add_row_identity(b, cb=C - 1)
    add_stage1_probes(b)
    return b


def group_c32(track):
    b = Builder("c32-track" if track else "c32-scan", 7 if track else 6, "features", LAY_C32, track)
    if track:
        add_segments(b, lambda s: (0, 3, 4, 28, 31)[s % 5])
    else:
        add_strided(b, 31)
    add_channel_identity(b, (0, 3, 4, 28, 31))
    add_row_identity(b, cb=28)
    if not track:
        add_stage1_probes(b)
        # past the counters' slots: a flagged row in a workgroup that shares slot 0's line
        while len(b.blocks) < SLOTS + 2:
            b.ordinary()
        b.burst("slot-wrap", 4, "pair", 44, ("frames", 44, 46),
                "a flagged row at epoch >= kGuardSlots: the counters' slots wrap")
    return b


def group_float32(name, lay, site, entry):
    b = Builder(name, site, entry, lay)
    C = len(lay.cols)
    add_segments(b, lambda s: s % C)
    add_channel_identity(b, range(C))
    add_row_identity(b, cb=C - 1)
    return b


# ---- site 9: caller-supplied epochs ---------------------------------------------------------------
def group_epochs(name, C, dtype):
    """Device epochs [n][C][750]: pairs in every segment, the burst row in epoch slots 0 and 7,
    the burst in channel 0 and C - 1, and (doubles) rows at both ends of guard_acc_out_of_range."""
    res = [1.0] * C
    lay = Layout(np.float32, C, list(range(C)), res)
    b = Builder(name, 9, "extract", lay)
    rows = []
    for slot in (0, SUB - 1):
        for s, p, lo, hi, what in segment_slices():
            while len(b.blocks) % SUB != slot:
                b.ordinary()
            cb = 0 if (s + slot) % 2 == 0 else C - 1
            b.burst("slot%d/segment%d/%s/ch%d" % (slot, s, what, cb), cb, "pair", p,
                    ("frames", lo, hi), "epoch slot %d, burst in channel %d, pair in segment %d (%s)"
                    % (slot, cb, s, what))
    add_channel_identity(b, sorted({0, C // 2, C - 1}))
    add_row_identity(b, cb=C - 1)
    ep = np.stack([blk[PRE:].T for blk in b.blocks])           # [n][C][750]
    cases = list(b.cases)
    if np.dtype(dtype) == np.float64:
        base = ordinary_block(res)[PRE:].T
        acc0 = sum(window_acc(np.ascontiguousarray(c[SKIP:SKIP + WIN])) for c in base)
        extra = []
        for end, bound in (("min", ACC_MIN), ("max", ACC_MAX)):
            k = int(np.floor(np.log2(bound / acc0) / 2.0))
            for side, kk in (("inside", k + 1 if end == "min" else k),
                             ("outside", k if end == "min" else k + 1)):
                extra.append(("range/%s-%s" % (end, side), base * 2.0 ** kk))
        for nm, e in extra:
            cases.append(Case("%s/%s" % (name, nm), 9, len(ep), ("range",), 2,
                              "acc just %s guard_acc_out_of_range's end" % nm.split("-")[-1]))
            ep = np.concatenate([ep, e[None]])
    ep = np.ascontiguousarray(ep.astype(dtype))
    ep.setflags(write=False)
    return Group(name, 9, "extract", lay, None, 0, None, ep, tuple(cases), False,
                 np.dtype(dtype).name), b.missing


# ---- all groups -----------------------------------------------------------------------------------
# name -> the tracking variant (three launches on one context); groups() builds them in this order
GROUP_NAMES = {
    "c3-scan-lanes": False, "c3-scan-identity": False, "c3-track": True, "c3-one-pass": False,
    "wide-int16-c5": False, "wide-int16-c7": False, "wide-float32": False, "c32-scan": False,
    "c32-track": True, "one-pass-packed": False, "one-pass-lds-int16": False,
    "one-pass-lds-float32": False, "c3-scan-end-pair-at-end": False,
    "c3-scan-end-ends-before-pair": False, "c3-one-pass-end-pair-at-end": False,
    "c3-one-pass-end-ends-before-pair": False, "epochs-f64-c3": False, "epochs-f32-c3": False,
    "epochs-f64-c32": False, "epochs-f32-c32": False,
}
_groups = None
MISSING = []


def groups():
    """name -> Group, built once (a few seconds: the searches)."""
    global _groups
    if _groups is not None:
        return _groups
    built = [
        group_site1_lanes(), group_site1_identity(),
        group_site1_identity(2, "c3-track", track=True),
        group_site3(),
        group_wide_int16("wide-int16-c5", LAY_WIDE5), group_wide_int16("wide-int16-c7", LAY_WIDE7),
        group_float32("wide-float32", LAY_WIDE_F32, 5, "features"),
        group_c32(False), group_c32(True),
        group_wide_int16("one-pass-packed", LAY_PACKED, 8, "one_pass"),
        group_wide_int16("one-pass-lds-int16", LAY_LDS_I16, 8, "one_pass"),
        group_float32("one-pass-lds-float32", LAY_LDS_F32, 8, "one_pass"),
    ]
    out = {}
    for b in built:
        MISSING.extend(b.missing)
        out[b.name] = b.finish()
    for site, entry, name in ((1, "features", "c3-scan-end"), (3, "one_pass", "c3-one-pass-end")):
        for g in groups_end(site, entry, name):
            out[g.name] = g
    for name, C, dtype in (("epochs-f64-c3", 3, np.float64), ("epochs-f32-c3", 3, np.float32),
                           ("epochs-f64-c32", 32, np.float64), ("epochs-f32-c32", 32, np.float32)):
        g, missing = group_epochs(name, C, dtype)
        MISSING.extend(missing)
        out[name] = g
    assert {n: g.track for n, g in out.items()} == GROUP_NAMES
    _groups = out
    return out


def case_blind(group, case):
    """A case's blindness with its data filled in."""
    if case.blind[0] == "past_end":
        return ("past_end", group.raw)
    return case.blind


def check_case(group, case, true):
    """(valid, text): the case's verdict under its blindness differs from the true one and every
    ratio involved lies MARGIN from 1."""
    t = true[case.row]
    if case.blind[0] == "range":
        acc_side = t.stage2_fails
        return True, "%s: out of range %s" % (case.name, acc_side)
    if group.entry == "extract":
        bl = verdict(9, group.epochs, None, None, case.row, case_blind(group, case))
    else:
        bl = verdict(group.site, group.raw[:group.n_frames], group.layout, group.pos, case.row,
                     case_blind(group, case))
    if case.stage == 1:
        a, c = t.ratio1, bl.ratio1
        differs = t.stage1_fails != bl.stage1_fails
    else:
        a, c = t.ratio2, bl.ratio2
        differs = t.stage2_fails != bl.stage2_fails
    margin = min(max(a, 1 / a) if a > 0 else np.inf, max(c, 1 / c) if c > 0 else np.inf)
    return bool(differs and margin >= MARGIN), "%s: true %.3f blind %.3f" % (case.name, a, c)


def row_margin(v, form):
    """How far a row's decisive ratios lie from 1 (>= 1; inf for 0 and inf)."""
    def m(r):
        return np.inf if r == 0 or not np.isfinite(r) else max(r, 1 / r)
    if form in ("measured", "epochs") or not v.stage1_fails:
        return m(v.ratio1)
    return min(m(v.ratio1), m(v.ratio2))
