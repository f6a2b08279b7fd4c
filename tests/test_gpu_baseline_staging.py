"""baseline_kernel's LDS-DMA staging (fused.hip): every way an epoch's pre-stimulus run can lie
in the recording, on the 3-channel int16 fused path.

An epoch's 100-frame run (600 B) is staged as 39 quads from floor16 of its first byte: by one
LDS-DMA when all 39 lie inside the recording, through registers with zero fill otherwise.  The
cases vary what decides between the two and what the DMA's addresses depend on:
- epoch counts around the 64-epoch tile (waves take epochs round-robin, partial tiles);
- the eight 16-byte phases of the run's first quad, at byte 0 and in mid-recording;
- runs against the end of the recording (its last quad whole or partial), pos - 100 = n_frames,
  windows past the end, a recording shorter than one quad;
- unsorted and duplicate markers, dense markers (cached reads) and sparse ones (streaming reads);
- permuted channels with different resolutions;
- the streamed path, whose chunk pointers put runs against a chunk's first and last bytes;
- positions the reference would not cut.

Every case is checked against oracle.process_recording (Baseline.java:29-42 is order-exact):
EXACT equal value for value, fma within 1e-9 per feature."""
import numpy as np
import pytest
import torch

import eeg_dataanalysispackage_amd as fx
import stream_cases as S
from eeg_dataanalysispackage_amd import _lib
from oracle import oracle

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
COLS, RES = [0, 1, 2], [0.1, 0.1, 0.1]


@pytest.fixture(scope="module")
def ctxs():
    a, b = fx.Context(0, numerics="exact"), fx.Context(0, numerics="fma")
    yield a, b
    a.close()
    b.close()


def synth_raw(seed, n_frames):
    rng = np.random.default_rng(seed)
    base = rng.integers(-20000, 20000, size=(1, 3))
    return np.clip(base + np.cumsum(rng.integers(-80, 81, size=(n_frames, 3)), axis=0), -32768,
                   32767).astype(np.int16)


def assert_exact(got, want, what):
    assert np.array_equal(got, want, equal_nan=True), what


def assert_fma(got, want, what):
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), fin), what
    assert np.max(np.abs(got[fin] - want[fin]), initial=0.0) <= 1e-9, what


def check(ctxs, raw, pos, cols=COLS, res=RES, what=None):
    exact, fma = ctxs
    pos = np.asarray(pos, dtype=np.int64)
    want = oracle.process_recording(raw, cols, res, pos)
    assert_exact(exact.process_recording(raw, 3, cols, res, pos), want, what)
    assert_fma(fma.process_recording(raw, 3, cols, res, pos), want, what)
    return want


@pytest.fixture(scope="module")
def recording():
    return synth_raw(1, 12_000)


# ---- epoch counts: partial and full 64-epoch tiles ----------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 129])
def test_epoch_counts(ctxs, recording, n):
    rng = np.random.default_rng(n)
    pos = rng.integers(100, recording.shape[0] - 700, size=n)
    check(ctxs, recording, pos, what=n)


# ---- the eight 16-byte phases of the run's first quad -------------------------------------------
@pytest.mark.parametrize("first", [100, 5003])
def test_first_quad_phases(ctxs, recording, first):
    """pos = first .. first + 7: the run starts at byte 6 (pos - 100), whose offsets in its quad
    are the eight even phases 0, 6, 12, 2, 8, 14, 4, 10 in some rotation; first = 100 puts the
    first quad at byte 0 of the recording.  As one batch and one epoch at a time."""
    pos = np.arange(first, first + 8, dtype=np.int64)
    assert sorted((6 * (p - 100)) % 16 for p in pos) == [0, 2, 4, 6, 8, 10, 12, 14]
    want = check(ctxs, recording, pos, what=first)
    exact, fma = ctxs
    for i, p in enumerate(pos):
        assert_exact(exact.process_recording(recording, 3, COLS, RES, pos[i:i + 1]), want[i:i + 1], p)
        assert_fma(fma.process_recording(recording, 3, COLS, RES, pos[i:i + 1]), want[i:i + 1], p)


# ---- the end of the recording -------------------------------------------------------------------
@pytest.mark.parametrize("n_frames", [2000, 2001, 2002])
def test_runs_against_the_end(ctxs, n_frames):
    """The recording's byte count leaves its last quad whole (n_frames * 6 % 16 = 0) or partial
    (6, 12).  Runs that end in the last quad (pos = n_frames, n_frames - 1, n_frames - 2), runs
    whose 39th quad is the first one not wholly inside, the empty run at pos - 100 = n_frames, runs
    cut by the end, and windows past the end (every position above n_frames - 687)."""
    assert n_frames * 6 % 16 == {2000: 0, 2001: 6, 2002: 12}[n_frames]
    raw = synth_raw(n_frames, n_frames)
    last = [n_frames - d for d in range(0, 12)]
    cut = [n_frames + d for d in (1, 2, 3, 50, 97, 98, 99, 100)]
    past = [n_frames - 687, n_frames - 686, n_frames - 300]
    check(ctxs, raw, last + cut + past + [100, 700], what=n_frames)
    for p in (n_frames, n_frames + 100, n_frames - 300):
        check(ctxs, raw, [p], what=(n_frames, p))


def test_recording_shorter_than_a_quad(ctxs):
    raw = synth_raw(3, 2)  # 12 bytes
    check(ctxs, raw, [100, 101, 102, 101, 100], what="2 frames")
    for p in (100, 101, 102):
        check(ctxs, raw, [p], what=p)


# ---- markers ------------------------------------------------------------------------------------
def test_unsorted_and_duplicate_markers(ctxs, recording):
    rng = np.random.default_rng(17)
    pos = rng.integers(100, recording.shape[0] - 700, size=90)
    pos[5] = pos[40]
    pos[41] = pos[40]
    pos[89] = pos[0]
    assert np.any(np.diff(pos) < 0)
    check(ctxs, recording, pos)


@pytest.mark.parametrize("spacing,n", [(60, 200), (1000, 70)])
def test_marker_density(ctxs, spacing, n):
    """Markers 60 frames apart (runs and windows shared between epochs: cached reads) and 1,000
    frames apart (disjoint: streaming reads)."""
    n_frames = 100 + spacing * n
    raw = synth_raw(spacing, n_frames)
    assert (n_frames // n >= 787) == (spacing == 1000)  # the launch's streaming test
    check(ctxs, raw, 100 + spacing * np.arange(n, dtype=np.int64), what=spacing)


# ---- channels -----------------------------------------------------------------------------------
@pytest.mark.parametrize("cols", [[2, 0, 1], [1, 2, 0], [2, 1, 0]])
def test_permuted_channels_with_their_own_resolutions(ctxs, recording, cols):
    rng = np.random.default_rng(23)
    pos = np.concatenate([rng.integers(100, recording.shape[0] + 100, size=66), [100, 12_000]])
    check(ctxs, recording, pos, cols=cols, res=[0.1, 0.0488281, 2.5], what=cols)


# ---- the streamed path --------------------------------------------------------------------------
def with_seams(pos, n_frames, chunk_frames, seams=6):
    """pos and, for the first chunks of the restated plan (tests/stream_cases.py), an epoch at the
    last position that still fits the chunk and one a frame later, which opens the next chunk.
    Both lie below the highest position, so no earlier chunk moves."""
    pos = sorted(int(p) for p in pos)
    for k in range(seams):
        ch = S.plan(pos, n_frames, chunk_frames)[k]
        assert ch.hi < n_frames and ch.hi - S.TAIL + 1 < pos[-1]
        pos = sorted(pos + [ch.hi - S.TAIL, ch.hi - S.TAIL + 1])
    chunks = S.plan(pos, n_frames, chunk_frames)
    for a, b in zip(chunks[:seams], chunks[1:]):
        assert pos[a.j - 1] == a.hi - S.TAIL and pos[b.i] == a.hi - S.TAIL + 1 == b.lo + S.PRE
    return np.array(pos, dtype=np.int64)


@pytest.mark.parametrize("chunk_frames", [787, 1000])
def test_streamed_chunks_equal_the_resident_call(ctxs, chunk_frames):
    """A 5,000-frame host recording streamed in chunks, the kernels reading through each chunk's
    own pointer and byte count.  Runs start at, end at and straddle every multiple of
    chunk_frames; the plan puts no chunk boundary there (a chunk starts at the first unprocessed
    epoch's pos - 100), so the first six seams of the plan itself are added: an epoch that ends
    exactly at its chunk's last frame and one a frame later.  tests/test_gpu_streamed_seams.py
    has the seams case by case."""
    raw = synth_raw(41, 5000)
    edges = np.arange(chunk_frames, 5000, chunk_frames)
    near = np.concatenate([edges + d for d in (-1, 0, 1, 99, 100, 101)])
    pos = np.concatenate([np.arange(100, 5101, 37), near[(near >= 100) & (near <= 5100)]])
    pos = pos.astype(np.int64)
    pos = np.concatenate([pos, np.setdiff1d(with_seams(pos, 5000, chunk_frames), pos)])
    want = oracle.process_recording(raw, COLS, RES, pos)
    for c, assert_close in zip(ctxs, (assert_exact, assert_fma)):
        resident = c.process_recording(raw, 3, COLS, RES, pos)
        streamed = c.process_recording_streamed(raw, 3, COLS, RES, pos, chunk_frames=chunk_frames)
        assert_exact(streamed, resident, chunk_frames)
        assert_close(streamed, want, chunk_frames)


# ---- positions the reference would not cut ------------------------------------------------------
def test_invalid_positions_are_reported_and_the_rest_is_exact(ctxs):
    n_frames = 30_000
    raw = synth_raw(7, n_frames)
    rng = np.random.default_rng(7)
    good = rng.integers(100, n_frames + 101, size=70).astype(np.int64)
    pos = good.copy()
    pos[13] = 99
    pos[66] = n_frames + 101
    keep = np.ones(70, dtype=bool)
    keep[[13, 66]] = False
    want = oracle.process_recording(raw, COLS, RES, good[keep])
    for c, assert_close in zip(ctxs, (assert_exact, assert_fma)):
        out = c.process_recording(torch.from_numpy(raw).to(DEV), 3, COLS, RES,
                                  torch.from_numpy(pos).to(DEV))
        with pytest.raises(IndexError) as e:
            c.synchronize()
        assert e.value.code == _lib.EEGFX_ERANGE
        c.synchronize()  # the flag was cleared
        assert_close(out.cpu().numpy()[keep], want, "valid rows")
