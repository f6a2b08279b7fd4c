"""The epoch kernels at the first and the last layout of every dispatch bucket: raw recording ->
baselines -> epochs -> dwt-8 rows (cut.hip, extract.hip, small.hip, wide.hip, fused.hip,
guard.hip) at the layouts tests/layout_cases.py names.  tests/test_layout_cases.py has shown off
the GPU that each case takes the kernels, the chunk count and the LDS bytes it is named for --
among them the first launches above 64 KB of static + dynamic LDS -- and that the two layouts of
every edge pair take different kernels; here every case runs, and must

- give epochs equal to oracle.decode_epochs value for value, as float64 and as float32, under
  both numerics;
- give, under exact numerics, the rows of oracle.process_recording / oracle.extract_features
  (np.array_equal, NaN positions equal);
- give, under fma, rows finite where the oracle's are and within 1e-9 of them per feature (the
  contract tests/test_gpu_fuzz.py holds), the null-space rows equal to the oracle's value for
  value, and guard_stats()[1] equal to their count;
- give the same bytes from host buffers as from device buffers;
- leave the sentinels around every output untouched, a features `out` 8 bytes off a 16-byte
  boundary included.

Inputs: 5,000 frames, a random walk (int16) or normal samples (float32) after an alternating
stretch (the filters' null space); n = 2 T + 2 epochs of the baseline tile T at positions
100 + 31 i (both parities, every 16-byte phase), the last one 450 samples past the recording's
end; for int16 also six positions 805 frames apart, which select the non-temporal variants.
"""
import numpy as np
import pytest
import torch

import eeg_dataanalysispackage_amd as fx
import layout_cases as L
from oracle import oracle

pytestmark = pytest.mark.gpu

BAND = 64                    # sentinel elements on either side of an output
SENT = -1234.5               # exact in float32 and float64
EPOCH_TYPES = ("float64", "float32")
RAW_CASES = [c for c in L.CASES if c.entry in ("features", "one_pass", "cut")]
EPOCH_CASES = [c for c in L.CASES if c.entry in ("extract", "small")]


@pytest.fixture(scope="module")
def ctxs():
    both = {"exact": fx.Context(0), "fma": fx.Context(0, numerics="fma")}
    yield both
    for c in both.values():
        c.close()


_cache = {}


def once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def frozen(a):
    a.setflags(write=False)
    return a


def recording(case):
    """(host array, device tensor), shared by the cases of one (sample type, ct, stretch)."""
    key = (case.dtype, case.ct, L.null_frames(case))
    def make():
        raw = frozen(L.recording(*key))
        return raw, torch.from_numpy(raw.copy()).cuda()
    return once(("raw",) + key, make)


def inputs(case, sparse):
    pos = L.sparse_positions() if sparse else L.positions(case)
    return frozen(pos), L.null_rows(case, pos)


def reference(case, sparse):
    """The oracle on a case's input, computed once for both numerics."""
    def make():
        raw = recording(case)[0]
        cols, res = L.selection(case)
        pos, _ = inputs(case, sparse)
        want = {}
        if case.entry in ("features", "one_pass"):
            want["features"] = frozen(oracle.process_recording(raw, cols, res, pos))
        if case.entry in ("cut", "one_pass"):
            want["epochs"] = frozen(oracle.decode_epochs(raw, cols, res, pos))
        return want
    return once(("want", case.name, sparse), make)


class Banded:
    """A device output between two sentinel bands; shift: elements past the band's end."""

    def __init__(self, shape, dtype, shift=0):
        self.count = int(np.prod(shape))
        self.lo = BAND + shift
        self.whole = torch.full((self.count + 2 * BAND + shift,), SENT, dtype=dtype, device="cuda")
        self.view = self.whole[self.lo:self.lo + self.count].view(shape)
        if dtype == torch.float64:
            assert self.view.data_ptr() % 16 == 8 * (shift % 2)

    def host(self):
        h = self.whole.cpu().numpy()
        assert (h[:self.lo] == SENT).all() and (h[self.lo + self.count:] == SENT).all()
        return h[self.lo:self.lo + self.count].reshape(tuple(self.view.shape))


def call(ctx, case, ename, raw, pos, device):
    """One call of the case's entry: {"features": ..., "epochs": ...} as host arrays."""
    cols, res = L.selection(case)
    n, C, ct = len(pos), case.C, case.ct
    edt = np.dtype(ename)
    outs = {}
    if not device:
        if case.entry == "features":
            outs["features"] = ctx.process_recording(raw, ct, cols, res, pos)
        elif case.entry == "one_pass":
            outs["features"], outs["epochs"] = ctx.process_recording_epochs(
                raw, ct, cols, res, pos, epochs_dtype=edt)
        else:
            outs["epochs"] = ctx.cut_epochs(raw, ct, cols, res, pos, dtype=edt)
        return outs
    pos_d = torch.from_numpy(np.array(pos)).cuda()
    if case.entry in ("features", "one_pass"):
        outs["features"] = Banded((n, 16 * C), torch.float64, shift=1 if case.shifted else 0)
    if case.entry in ("cut", "one_pass"):
        outs["epochs"] = Banded((n, C, L.POST), getattr(torch, ename))
    if case.entry == "features":
        ctx.process_recording(raw, ct, cols, res, pos_d, out=outs["features"].view)
    elif case.entry == "one_pass":
        ctx.process_recording_epochs(raw, ct, cols, res, pos_d, out=outs["features"].view,
                                     epochs_out=outs["epochs"].view, epochs_dtype=edt)
    else:
        ctx.cut_epochs(raw, ct, cols, res, pos_d, out=outs["epochs"].view, dtype=edt)
    ctx.synchronize()
    return {k: o.host() for k, o in outs.items()}


def compare(got, want, numerics, nulls, what):
    for name, ref in want.items():
        g = got[name].astype(np.float64)               # float32 epochs widen exactly
        assert g.shape == ref.shape, (what, name)
        if numerics == "exact" or name == "epochs":
            assert np.array_equal(g, ref, equal_nan=True), (what, name)
        else:
            fin = np.isfinite(ref)
            assert np.isfinite(g[fin]).all(), (what, name)
            assert np.max(np.abs(g[fin] - ref[fin]), initial=0.0) <= 1e-9, (what, name)
            assert np.array_equal(g[nulls], ref[nulls]), (what, name, "null space")


def ids(cases):
    return [c.name for c in cases]


@pytest.mark.parametrize("numerics", ["exact", "fma"])
@pytest.mark.parametrize("case", RAW_CASES, ids=ids(RAW_CASES))
def test_raw_entries_at_the_edge_layouts(ctxs, case, numerics):
    ctx = ctxs[numerics]
    raw_h, raw_d = recording(case)
    counted = numerics == "fma" and case.entry != "cut"
    for sparse in (False, True) if case.dtype == L.I16 else (False,):
        pos, nulls = inputs(case, sparse)
        want = reference(case, sparse)
        assert np.isfinite(want.get("features", np.zeros(1))[:-1]).all()
        for ename in EPOCH_TYPES if "epochs" in want else ("float64",):
            what = (case.name, "sparse" if sparse else "dense", ename)
            ctx.guard_stats(reset=True)
            dev = call(ctx, case, ename, raw_d, pos, device=True)
            if counted:     # the null-space rows, and no other, were recomputed under EXACT
                assert ctx.guard_stats(reset=True)[1] == len(nulls), what
            compare(dev, want, numerics, nulls, what)
            host = call(ctx, case, ename, raw_h, pos, device=False)
            if counted:
                assert ctx.guard_stats(reset=True)[1] == len(nulls), what + ("host",)
            compare(host, want, numerics, nulls, what + ("host",))
            for name in want:
                # a shifted `out` takes other fma kernels than the aligned staging of a host call
                if not (case.shifted and numerics == "fma"):
                    assert host[name].tobytes() == dev[name].tobytes(), what + (name,)


def epochs_input(case):
    def make():
        ep, nulls = L.epochs_input(case)
        return frozen(ep), nulls, frozen(oracle.extract_features(ep, nfeat=case.nfeat))
    return once(("epochs", case.name), make)


@pytest.mark.parametrize("numerics", ["exact", "fma"])
@pytest.mark.parametrize("case", EPOCH_CASES, ids=ids(EPOCH_CASES))
def test_extract_at_the_edge_layouts(ctxs, case, numerics):
    ctx = ctxs[numerics]
    ep, nulls, ref = epochs_input(case)
    want = {"features": ref}
    small = case.kernels == (L.FSMALL,)      # EXACT rows under both numerics, outside the guard
    flagged = 0 if small else len(nulls)
    ctx.guard_stats(reset=True)
    host = {"features": ctx.extract_features(ep, feature_size=case.nfeat)}
    if numerics == "fma":
        assert ctx.guard_stats(reset=True)[1] == flagged
    compare(host, want, "exact" if small else numerics, nulls, (case.name, "host"))
    if case.entry == "small":
        return
    out = Banded(ref.shape, torch.float64)
    ctx.extract_features(torch.from_numpy(ep.copy()).cuda(), feature_size=case.nfeat, out=out.view)
    ctx.synchronize()
    dev = {"features": out.host()}
    if numerics == "fma":
        assert ctx.guard_stats(reset=True)[1] == flagged
    compare(dev, want, numerics, nulls, (case.name, "device"))
    assert host["features"].tobytes() == dev["features"].tobytes()


def test_both_neighbours_of_every_edge_are_run():
    run = {c.name for c in RAW_CASES + EPOCH_CASES}
    assert run == set(L.BY_NAME) and all(a in run and b in run for a, b, _ in L.EDGES)
