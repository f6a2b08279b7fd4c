"""eegfx_process_recording_streamed at every seam of its chunk plan and on each route (DESIGN.md
section 10.9).

The cases are tests/stream_cases.py's: positions computed from the restated plan so that epochs end
exactly at a chunk's last frame and start a frame later, plans of 1 to 9 chunks (the short rings,
the first and the second reuse of a buffer), the ramp's sizes, the recording's end (clipped, exact,
tails, a chunk of no frames), chunk starts at every 16-byte phase, gaps that are never uploaded, a
host pointer 2 bytes off a 16-byte boundary, a 24 MB chunk copied by three threads, and chunk sizes
far beyond the recording.  tests/test_stream_cases.py proves on the CPU that each case has its
condition.  The routes: the 3-of-3 fused kernels (plain and permuted), a wide int16 layout, the
32-of-32 montage's window_c32_kernel, a float32 layout, and 70 channels, which neither
fused_supported nor wide_supported takes (cut + extract).

Every streamed call is compared with the resident process_recording of the same context bit for
bit, with oracle.process_recording value for value under EXACT, and within 1e-9 per feature with
the same finite mask under fma.  Sources are pageable and pinned; outputs are pageable and pinned
with sentinel rows around them.  One context per numerics setting for the whole file."""
import numpy as np
import pytest
import torch

import eeg_dataanalysispackage_amd as fx
import stream_cases as S
from oracle import oracle

pytestmark = pytest.mark.gpu
SENTINEL = -7.0


@pytest.fixture(scope="module")
def ctxs():
    a, b = fx.Context(0, numerics="exact"), fx.Context(0, numerics="fma")
    yield a, b
    a.close()
    b.close()


def assert_exact(got, want, what):
    assert np.array_equal(got, want, equal_nan=True), what


def assert_fma(got, want, what):
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), fin), what
    assert np.max(np.abs(got[fin] - want[fin]), initial=0.0) <= 1e-9, what


_RECORDINGS, _PINNED, _WANT = {}, {}, {}


def recording(lay, n_frames):
    """One read-only recording a (layout, length), shared by every test that needs it."""
    key = (lay.name, n_frames)
    if key not in _RECORDINGS:
        raw = S.recording(lay, n_frames)
        raw.setflags(write=False)
        _RECORDINGS[key] = raw
    return _RECORDINGS[key]


def pinned_copy(lay, n_frames):
    key = (lay.name, n_frames)
    if key not in _PINNED:
        t = torch.empty((n_frames, lay.ct), dtype=getattr(torch, lay.dtype), pin_memory=True)
        t.numpy()[:] = recording(lay, n_frames)
        _PINNED[key] = t
    return _PINNED[key].numpy()


def oracle_rows(lay, n_frames, pos, key):
    """The oracle's rows, computed once a (layout, case)."""
    if key not in _WANT:
        want = oracle.process_recording(recording(lay, n_frames), list(lay.cols), list(lay.res), pos)
        want.setflags(write=False)
        _WANT[key] = want
    return _WANT[key]


def framed(n, F, pinned):
    """An output of n rows between two sentinel rows."""
    if pinned:
        buf = torch.full((n + 2, F), SENTINEL, dtype=torch.float64, pin_memory=True).numpy()
    else:
        buf = np.full((n + 2, F), SENTINEL)
    return buf, buf[1:-1]


def check(ctxs, lay, n_frames, chunk_frames, pos, key, raws=None, outs=(False, True)):
    """Streamed == resident bit for bit; == the oracle under EXACT, within 1e-9 under fma."""
    pos = np.ascontiguousarray(pos, dtype=np.int64)
    cols, res = list(lay.cols), list(lay.res)
    want = oracle_rows(lay, n_frames, pos, key)
    if raws is None:
        raws = (recording(lay, n_frames), pinned_copy(lay, n_frames))
    for c, assert_close in zip(ctxs, (assert_exact, assert_fma)):
        resident = c.process_recording(raws[0], lay.ct, cols, res, pos)
        assert_close(resident, want, (key, "resident"))
        for raw, pinned_out in zip(raws, outs):
            buf, out = framed(len(pos), 16 * len(cols), pinned_out)
            got = c.process_recording_streamed(raw, lay.ct, cols, res, pos,
                                               chunk_frames=chunk_frames, out=out)
            assert got is out
            assert_exact(out, resident, (key, "streamed against resident"))
            assert_close(out, want, (key, "streamed against the oracle"))
            assert np.all(buf[0] == SENTINEL) and np.all(buf[-1] == SENTINEL), key


def ids(cases):
    return [c.name for c in cases]


# ---- exact fit, chunk counts and the recording's end, on each route -----------------------------
@pytest.mark.parametrize("lay", S.LAYOUTS, ids=[lay.name for lay in S.LAYOUTS])
@pytest.mark.parametrize("case", S.cases("routes"), ids=ids(S.cases("routes")))
def test_seams_on_each_route(ctxs, case, lay):
    """A pageable source into a pageable output and a pinned source into a pinned output.  The
    70-channel layout has a route (the cut kernels and the batch extract), so its rows are the
    oracle's like every other layout's."""
    check(ctxs, lay, case.n_frames, case.chunk_frames, case.pos, (lay.name, case.name))


def test_the_route_cases_are_the_ones_named():
    names = set(ids(S.cases("routes")))
    assert {"fit-1600", "fit-dup-1600", "fit-dup-shuffled-1600", "end-clipped", "end-equal",
            "end-tails", "end-empty-only", "end-empty-mid"} <= names
    assert {"count-%d" % K for K in (1, 2, 3, 4, 5, 9)} <= names


# ---- the fused kernels at the other chunk sizes, the ramp and the gaps --------------------------
@pytest.mark.parametrize("case", S.cases("c3"), ids=ids(S.cases("c3")))
def test_seams_on_the_fused_kernels(ctxs, case):
    lay = S.LAYOUT["i16-3x3"]
    check(ctxs, lay, case.n_frames, case.chunk_frames, case.pos, (lay.name, case.name))
    # and the other way round: pinned rows from a pageable source, pageable from a pinned one
    check(ctxs, lay, case.n_frames, case.chunk_frames, case.pos, (lay.name, case.name),
          outs=(True, False))


# ---- chunk starts at every 16-byte phase a frame size allows -------------------------------------
@pytest.mark.parametrize("lay", S.LAYOUTS + [S.LAYOUT_4CH],
                         ids=[lay.name for lay in S.LAYOUTS + [S.LAYOUT_4CH]])
def test_quad_phases(ctxs, lay):
    case = S.BY_NAME["phases"]
    check(ctxs, lay, case.n_frames, case.chunk_frames, case.pos, (lay.name, case.name))


# ---- a host pointer 2 bytes past a 16-byte boundary ----------------------------------------------
@pytest.mark.parametrize("name", ["i16-3x3", "i16-8x5"])
def test_pageable_source_two_bytes_off_a_quad(ctxs, name):
    lay, case = S.LAYOUT[name], S.BY_NAME["fit-dup-1600"]
    src = recording(lay, case.n_frames)
    store = np.empty(src.nbytes + 32, dtype=np.uint8)
    off = (2 - store.ctypes.data) % 16
    raw = store[off:off + src.nbytes].view(np.int16).reshape(src.shape)
    raw[:] = src
    assert raw.ctypes.data % 16 == 2
    check(ctxs, lay, case.n_frames, case.chunk_frames, case.pos, (lay.name, case.name),
          raws=(raw, raw))


# ---- the threaded host copy ----------------------------------------------------------------------
def test_a_24_mb_chunk_copied_by_three_threads(ctxs):
    """32-channel int16, 1.1 M frames, chunk_frames = 393,216: the third chunk is 24 MB of a
    pageable source, copied into the pinned staging by three threads; epochs straddle each thread
    boundary and sit at both ends of that chunk (tests/test_stream_cases.py::test_threaded_case)."""
    lay = S.LAYOUT[S.THREADED["layout"]]
    n_frames = S.THREADED["n_frames"]
    pos = S.threaded_case()[0]
    rng = np.random.default_rng(64)
    raw = rng.integers(-3000, 3000, size=(n_frames, lay.ct), dtype=np.int16)
    _RECORDINGS[(lay.name, n_frames)] = raw
    try:
        check(ctxs, lay, n_frames, S.THREADED["chunk_frames"], pos, (lay.name, "threaded"),
              raws=(raw, raw))
    finally:
        del _RECORDINGS[(lay.name, n_frames)]
        _WANT.pop((lay.name, "threaded"), None)


def test_a_chunk_whose_bytes_three_threads_do_not_divide(ctxs):
    """3-channel int16, chunk_frames = 2^22: the third chunk uploads 24 MB + 2 bytes of a pageable
    source, and the epoch at its exact fit reads the last of them (the copy split once left them
    out; tests/test_stream_cases.py::test_remainder_case)."""
    lay = S.LAYOUT[S.REMAINDER["layout"]]
    n_frames = S.REMAINDER["n_frames"]
    pos = S.remainder_case()[0]
    raw = np.random.default_rng(6).integers(-3000, 3000, size=(n_frames, lay.ct), dtype=np.int16)
    _RECORDINGS[(lay.name, n_frames)] = raw
    try:
        check(ctxs, lay, n_frames, S.REMAINDER["chunk_frames"], pos, (lay.name, "remainder"),
              raws=(raw, raw))
    finally:
        del _RECORDINGS[(lay.name, n_frames)]
        _WANT.pop((lay.name, "remainder"), None)


# ---- chunk sizes far beyond the recording ----------------------------------------------------------
@pytest.mark.parametrize("chunk_frames", S.LARGE_CHUNK_FRAMES, ids=["2^40", "2^62"])
def test_chunk_frames_beyond_the_recording(ctxs, chunk_frames):
    """One chunk, sized by the recording: the resident call's rows (before the bound on
    chunk_frames 2^40 asked for terabytes and 2^62 * FB wrapped)."""
    lay, case = S.LAYOUT_4CH, S.BY_NAME["count-3"]
    assert S.frame_bytes(lay) == 8
    assert len(S.plan(np.sort(case.pos), case.n_frames, chunk_frames)) == 1
    check(ctxs, lay, case.n_frames, chunk_frames, case.pos, (lay.name, case.name))
