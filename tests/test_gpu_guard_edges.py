"""The conditioning guard's verdict at its decision boundary, at every site that takes it (DESIGN.md
section 10.10).  tests/guard_cases.py builds rows whose verdict depends on a few frames of one
channel of one row -- a pair burst or a single impulse on an alternation, tuned so that
acc / (K2 sum X^2) lies at least 1.05 below 1 with the true X and at least 1.05 above it with what
a scan blind to one lane's frames, one channel or one row would measure -- and restates every
row's verdict on the CPU; tests/test_guard_cases.py has proved the cases valid.  Here one call per
group runs on the device under fma numerics, from host and from device buffers, each on a fresh
context (the scan and track variants depend on a context's launch history), and

- guard_detail() must equal the restatement's (checked, rechecked, recomputed) exactly;
- every row the restatement recomputes must equal the oracle value for value;
- every other row must lie within 1e-9 of the oracle;
- on a counter mismatch the message lists the cases whose rows are, or are not, bit-equal to the
  oracle, so that the verdict can be read row by row.

The tracking variants (sites 2 and 7) run the same call twice more on the same context: the group
flags more than 1/16 of its rows, so the later launches track; counters and bytes of the three
runs must be equal, and each equal to the restatement.  The any-layout window kernel (site 4)
sends its failing rows to exact_rows_kernel: the recomputed counter and the value-identical rows
show that it received exactly the restated ones.
"""
import numpy as np
import pytest
import torch

import eeg_dataanalysispackage_amd as fx
import guard_cases as G
from oracle import oracle

pytestmark = pytest.mark.gpu
TOL = 1e-9

_cache = {}


def reference(name):
    """(group, restated verdicts, counters, oracle rows), computed once and left unchanged."""
    if name not in _cache:
        g = G.groups()[name]
        true, counters = G.restate(g)
        if g.entry == "extract":
            want = oracle.extract_features(np.asarray(g.epochs, dtype=np.float64))
        else:
            want = oracle.process_recording(g.raw[:g.n_frames], g.layout.cols, g.layout.res, g.pos)
        want.setflags(write=False)
        _cache[name] = (g, true, counters, want)
    return _cache[name]


def call(ctx, g, device):
    """One call of the group's entry; the rows as a host array."""
    if g.entry == "extract":
        ep = torch.from_numpy(np.array(g.epochs)).cuda() if device else np.array(g.epochs)
        if g.dtype == "float32":
            out = ctx.extract_features_f32(ep)
        else:
            out = ctx.extract_features(ep)
        return out.cpu().numpy() if device else out
    lay = g.layout
    # the declared frames over the whole buffer: what lies past them must read as zero padding
    raw = (torch.from_numpy(np.array(g.raw)).cuda() if device else g.raw)[:g.n_frames]
    pos = torch.from_numpy(np.array(g.pos)).cuda() if device else g.pos
    if g.entry == "features":
        out = ctx.process_recording(raw, lay.ct, lay.cols, lay.res, pos)
    else:
        out = ctx.process_recording_epochs(raw, lay.ct, lay.cols, lay.res, pos)[0]
    return out.cpu().numpy() if device else out


def row_equal(got, want):
    return np.array([np.array_equal(got[e], want[e], equal_nan=True) for e in range(len(want))])


def per_case(g, got, want, true):
    eq = row_equal(got, want)
    lines = []
    for c in g.cases:
        v = true[c.row]
        lines.append("%s: row %d restated %s, %s the oracle"
                     % (c.name, c.row, "recomputed" if v.stage2_fails else
                        "rechecked" if v.stage1_fails else "certified at stage 1",
                        "bit-equal to" if eq[c.row] else "differs from"))
    return "\n".join(lines)


def check(g, got, detail, true, counters, want, what):
    redo = np.array([v.stage2_fails for v in true])
    assert tuple(detail) == counters, "%s %s: guard_detail %s, restated %s\n%s" % (
        g.name, what, tuple(detail), counters, per_case(g, got, want, true))
    eq = row_equal(got, want)
    assert eq[redo].all(), "%s %s: recomputed rows differ from the oracle\n%s" % (
        g.name, what, per_case(g, got, want, true))
    assert got.shape == want.shape and np.all(np.abs(got[~redo] - want[~redo]) <= TOL), (
        g.name, what)


@pytest.mark.parametrize("name", [n for n, track in G.GROUP_NAMES.items() if not track])
def test_verdict_at_the_boundary(name):
    g, true, counters, want = reference(name)
    runs = []
    for device in (False, True):
        ctx = fx.Context(0, numerics="fma")   # a fresh context: its first launch scans
        try:
            got = call(ctx, g, device)
            ctx.synchronize()
            detail = ctx.guard_detail()
        finally:
            ctx.close()
        check(g, got, detail, true, counters, want, "device" if device else "host")
        runs.append(got)
    assert np.array_equal(runs[0], runs[1], equal_nan=True), g.name
    if g.site == 4:
        # exact_rows_kernel received exactly the restated rows: check() has compared the recomputed
        # counter (its list's length) and found those rows, and only rows of that number, rewritten
        assert counters[2] > 0


@pytest.mark.parametrize("name", [n for n, track in G.GROUP_NAMES.items() if track])
def test_tracking_variants_agree_with_the_scan(name):
    g, true, counters, want = reference(name)
    assert counters[1] * 16 > counters[0]     # the launches after the first one track
    ctx = fx.Context(0, numerics="fma")
    runs = []
    try:
        for i in range(3):
            ctx.guard_detail(reset=True)
            got = call(ctx, g, True)
            ctx.synchronize()
            runs.append((got, ctx.guard_detail()))
    finally:
        ctx.close()
    for i, (got, detail) in enumerate(runs):
        check(g, got, detail, true, counters, want, "launch %d" % (i + 1))
    assert runs[0][1] == runs[1][1] == runs[2][1]
    assert np.array_equal(runs[0][0], runs[1][0], equal_nan=True)
    assert np.array_equal(runs[1][0], runs[2][0], equal_nan=True)
