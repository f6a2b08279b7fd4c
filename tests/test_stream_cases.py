"""The streamed entry's chunk plan and copy split (csrc/stream_plan.h) off the GPU (DESIGN.md
section 10.9).

tests/c_abi/stream_plan_check.cpp includes that header alone and makes no HIP call.  It is built
with AddressSanitizer + UBSan, the runtimes linked statically, and run directly as a plain program:
- its plan equals the Python restatement (tests/stream_cases.py) on every named case at every
  frame size, on the threaded-copy case and at the large chunk sizes;
- the plan's properties hold on those and on a seeded sweep of 2,400 inputs with chunk_frames up
  to 2^62 (on the arithmetic before the bound on chunk_frames the buffer-size property and UBSan
  fail there: a wrapped chunk_frames * FB gave a 256-byte buffer for a whole recording);
- the copy split tiles its bytes, the copy equals memcpy and leaves the sentinels alone;
- every named case has the condition it exists for.
EEGFX_STREAM_PLAN_INCLUDE names another directory to take stream_plan.h from (the mutants of
tools/stream_plan_mutants.py)."""
import os
import re
import subprocess

import numpy as np
import pytest

import stream_cases as S
from conftest import REPO

SRC = os.path.join(REPO, "tests", "c_abi", "stream_plan_check.cpp")
INCLUDE = os.environ.get("EEGFX_STREAM_PLAN_INCLUDE", S.CSRC)
FBS = (2, 4, 6, 10, 12, 16, 64, 128, 280)
MB = 1 << 20


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("stream_plan") / "stream_plan_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-Wall", "-Werror",
                    "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan",
                    "-fno-sanitize-recover=all", "-I", INCLUDE, "-I", os.path.join(REPO, "include"),
                    SRC, "-o", out], check=True)
    return out


def run(exe, lines):
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, \
        (r.stdout[-2000:] + r.stderr[-4000:])
    out = r.stdout.splitlines()
    assert out[-1] == "stream_plan_check ok"
    return out[:-1]


def plan_line(n_frames, fb, chunk_frames, spos):
    return "plan %d %d %d %d %s" % (n_frames, fb, chunk_frames, len(spos),
                                    " ".join(str(int(p)) for p in spos))


def parse_plans(out):
    """[(head dict, [chunk tuples (k, i, j, lo, hi, Lb, Hb, bytes, slot, staging)])] of the output."""
    plans = []
    for line in out:
        w = line.split()
        if w[0] == "plan":
            plans.append(({k: int(v) for k, v in (x.split("=") for x in w[1:])}, []))
        else:
            assert w[0] == "chunk", line
            plans[-1][1].append(tuple(int(x) for x in w[1:]))
    return plans


def restated(n_frames, fb, chunk_frames, spos):
    chunks = S.plan(spos, n_frames, chunk_frames)
    R = S.ring(len(chunks))
    head = dict(chunks=len(chunks), c=S.chunk_frames_used(chunk_frames, n_frames),
                cbytes=S.buffer_bytes(chunks, fb), R=R)
    return head, [(k, *ch, *S.chunk_bytes(ch, fb), S.slot(k, R), S.staging(k))
                  for k, ch in enumerate(chunks)]


def named_inputs():
    """(what, n_frames, FB, chunk_frames, sorted positions): every case at every frame size, the
    threaded case, and the large chunk sizes over the smallest case and over the longest."""
    inputs = []
    for c in S.CASES:
        for fb in FBS + (140,):
            inputs.append((c.name, c.n_frames, fb, c.chunk_frames, np.sort(c.pos)))
    pos = S.threaded_case()[0]
    inputs.append(("threaded", S.THREADED["n_frames"], 64, S.THREADED["chunk_frames"], pos))
    for big in S.LARGE_CHUNK_FRAMES + (1 << 61, (1 << 63) - 1):
        for c in (S.BY_NAME["count-3"], S.BY_NAME["ramp-8192"]):
            for fb in (8, 6, 280):
                inputs.append(("%s at %d" % (c.name, big), c.n_frames, fb, big, np.sort(c.pos)))
    return inputs


def sweep_inputs(count=2400, seed=20240611):
    rng = np.random.default_rng(seed)
    powers = [1 << k for k in range(10, 63)]      # every power of two from 1,024 to 2^62
    inputs = []
    for t in range(count):
        n = int(rng.integers(1, 301))
        n_frames = int(rng.integers(1, 200_001)) if t % 7 else int(rng.integers(1, 2000))
        fb = int(FBS[t % len(FBS)])
        kind = t % 4
        if kind == 0:
            cf = powers[(t // 4) % len(powers)]
        elif kind == 1:
            cf = int(rng.integers(787, max(788, 2 * n_frames)))
        elif kind == 2:
            cf = int(2.0 ** rng.uniform(np.log2(787), 62))
        else:
            cf = (787, 788, 1573, 1574, 1575, 3148, (1 << 62) - 1, 1 << 62)[(t // 4) % 8]
        cf = min(max(cf, 787), 1 << 62)
        if t % 3 == 0:    # clustered: many epochs a chunk, duplicates
            centre = rng.integers(100, n_frames + 101, size=max(1, n // 40))
            pos = rng.choice(centre, size=n) + rng.integers(0, 900, size=n)
            pos = np.clip(pos, 100, n_frames + 100)
        else:
            pos = rng.integers(100, n_frames + 101, size=n)
        inputs.append(("sweep %d" % t, n_frames, fb, cf, np.sort(pos).astype(np.int64)))
    assert {i[3] for i in inputs} >= set(powers) and {i[2] for i in inputs} == set(FBS)
    assert min(i[3] for i in inputs) == 787 and max(i[3] for i in inputs) == 1 << 62
    return inputs


def check_properties(inp, head, chunks):
    what, n_frames, fb, chunk_frames, spos = inp
    n, K = len(spos), len(chunks)
    assert head["chunks"] == K >= 1, what
    # the chunks partition [0, n) in order and none is empty
    assert chunks[0][1] == 0 and chunks[-1][2] == n, what
    for a, b in zip(chunks, chunks[1:]):
        assert a[2] == b[1], what
    most = 0
    for k, i, j, lo, hi, Lb, Hb, nbytes, slot, staging in chunks:
        assert i < j, (what, k)
        # every epoch's frames lie in its chunk's [lo, hi)
        assert 0 <= lo <= hi <= n_frames, (what, k)
        assert lo <= int(spos[i]) - S.PRE, (what, k)
        assert min(int(spos[j - 1]) + S.TAIL, n_frames) <= hi, (what, k)
        assert hi - lo <= chunk_frames, (what, k)
        # the upload: from the 16-byte floor of the first frame to the end of the last
        assert Lb % 16 == 0 and 0 <= lo * fb - Lb < 16 and Hb == hi * fb, (what, k)
        assert nbytes == max(Hb - Lb, 0), (what, k)
        assert 64 + nbytes <= head["cbytes"], (what, k)
        assert slot == k % head["R"] and staging == k % 2, (what, k)
        most = max(most, nbytes)
    # a buffer is sized by what is uploaded, never by the caller's chunk_frames
    assert head["cbytes"] % 256 == 0 and head["cbytes"] <= most + 128 + 255, what
    # the ring: every buffer of it is used, R consecutive chunks never share one
    assert head["R"] == min(K, 4), what
    assert {c[8] for c in chunks} == set(range(head["R"])), what
    assert head["c"] <= chunk_frames and head["c"] >= min(chunk_frames, n_frames), what


@pytest.fixture(scope="module")
def named(exe):
    inputs = named_inputs()
    return inputs, parse_plans(run(exe, [plan_line(*i[1:]) for i in inputs]))


def test_the_restated_constants_are_the_sources():
    h = open(os.path.join(S.CSRC, "stream_plan.h")).read()
    assert "kStreamSpan = EEGFX_PRESTIMULUS + EEGFX_DWT8_SKIP + EEGFX_DWT8_EPOCH_SIZE;" in h
    assert int(re.search(r"constexpr size_t kStreamRing = (\d+);", h).group(1)) == S.RING
    assert int(re.search(r"constexpr size_t kStreamStagings = (\d+);", h).group(1)) == S.STAGINGS
    assert (S.PRE, S.TAIL, S.SPAN) == (100, 687, 787)
    s = open(os.path.join(S.CSRC, "streamed.cpp")).read()
    for call in ("stream_plan(spos, n, n_frames, chunk_frames)", "stream_buffer_bytes(plan, FB)",
                 "stream_ring(plan.size())", "stream_slot(k, R)", "stream_staging(k)",
                 "stream_chunk_bytes(plan[k], FB)", "parallel_memcpy(pin[st], src, bytes)"):
        assert call in s, call
    assert re.findall(r'#include [<"]([^>"]+)', h) == [
        "algorithm", "cstddef", "cstdint", "cstring", "thread", "vector", "eegfx.h"]  # no HIP


def test_the_plans_agree(named):
    inputs, plans = named
    assert len(plans) == len(inputs)
    for inp, (head, chunks) in zip(inputs, plans):
        assert (head, chunks) == restated(*inp[1:]), inp[0]


def test_the_plan_for_a_chunk_size_the_recording_can_use_is_unchanged():
    """chunk_frames <= n_frames is never cut, and from 4 n_frames up every value plans alike."""
    for c in S.CASES:
        assert S.chunk_frames_used(c.chunk_frames, c.n_frames) == c.chunk_frames
        one = S.plan(np.sort(c.pos), c.n_frames, 4 * c.n_frames)
        assert len(one) == 1 and one[0].hi == c.n_frames
        for big in (4 * c.n_frames + 1, 1 << 40, 1 << 62):
            assert S.plan(np.sort(c.pos), c.n_frames, big) == one


def test_properties_of_the_named_plans(named):
    for inp, (head, chunks) in zip(*named):
        check_properties(inp, head, chunks)


def test_properties_of_a_sweep(exe):
    inputs = sweep_inputs()
    plans = parse_plans(run(exe, [plan_line(*i[1:]) for i in inputs]))
    assert len(plans) == len(inputs) >= 2000
    for inp, (head, chunks) in zip(inputs, plans):
        check_properties(inp, head, chunks)
    # the sweep reaches what it is for: short rings, reused buffers, clipped and empty chunks
    counts = {len(c) for _, c in plans}
    assert {1, 2, 3, 4, 5} <= counts and max(counts) >= 9
    assert any(c[-1][4] == c[-1][3] for _, c in plans)          # a last chunk of no frames


COPY_BYTES = [0, 1, 63, 8 * MB - 1, 16 * MB - 64, 16 * MB - 1, 16 * MB, 16 * MB + 1,
              24 * MB - 1, 24 * MB, 24 * MB + 1, 24 * MB + 4097, 17 * MB + 12345, 64 * MB + 191]


def test_the_copy_split(exe):
    sizes = COPY_BYTES + [S.chunk_bytes(S.threaded_case()[1][2], 64)[2],
                          S.chunk_bytes(S.remainder_case()[1][2], 6)[2]]
    assert any(b % 64 for b in sizes if b >= 16 * MB)
    lines = []
    for b in sizes:
        for hw in (0, 1, 2, 3, 8, 64):
            lines.append("split %d %d" % (b, hw))
    out = run(exe, lines)
    it = iter(out)
    for b in sizes:
        for hw in (0, 1, 2, 3, 8, 64):
            w = next(it).split()
            nt, per = int(w[1]), int(w[2])
            assert w[0] == "split" and (nt, per) == S.copy_split(b, hw), (b, hw)
            assert nt == min(8, max(1, hw), max(1, b // (8 * MB))), (b, hw)
            pieces = [tuple(int(x) for x in next(it).split()[1:]) for _ in range(nt)]
            assert [p[1:] for p in pieces] == S.copy_pieces(b, hw), (b, hw)
            # the pieces tile [0, bytes) exactly, and every piece but the last starts on a line
            at = 0
            for t, a, ln in pieces:
                assert a == at and (a % 64 == 0 or ln == 0) and ln <= per, (b, hw, t)
                at += ln
            assert at == b, (b, hw)
    assert S.copy_split(16 * MB - 1, 8) == (1, 16 * MB - 1) and S.copy_split(16 * MB, 8)[0] == 2
    assert S.copy_split(24 * MB - 1, 8)[0] == 2 and S.copy_split(24 * MB, 8) == (3, 8 * MB)


def test_the_threaded_copy_equals_memcpy(exe):
    """parallel_memcpy itself, with 8 threads allowed whatever this machine has, between buffers
    with sentinels on both sides."""
    lines = ["copy %d 8" % b for b in COPY_BYTES + [24 * MB + 2]]
    lines += ["copy %d 3" % (24 * MB), "copy %d 1" % (24 * MB)]
    out = run(exe, lines)
    assert out == ["copy ok"] * len(lines), out


# ---- every case has the condition it exists for ----------------------------------------------------
def plans_of(names):
    return {n: S.plan(np.sort(S.BY_NAME[n].pos), S.BY_NAME[n].n_frames,
                      S.BY_NAME[n].chunk_frames) for n in names}


@pytest.mark.parametrize("case", S.CASES, ids=[c.name for c in S.CASES])
def test_every_case_has_the_chunks_it_was_built_for(case):
    chunks = S.plan(np.sort(case.pos), case.n_frames, case.chunk_frames)
    assert tuple((ch.lo, ch.hi) for ch in chunks) == case.opens
    assert case.pos.min() >= S.PRE and case.pos.max() <= case.n_frames + S.PRE
    assert case.n_frames <= 60_000 and case.chunk_frames in (787, 1600, 8192)


@pytest.mark.parametrize("c", [787, 1600, 8192])
def test_exact_fit_cases(c):
    for name, copies in (("fit-%d" % c, 1), ("fit-dup-%d" % c, 3), ("fit-dup-shuffled-%d" % c, 3)):
        case = S.BY_NAME[name]
        spos = np.sort(case.pos)
        chunks = S.plan(spos, case.n_frames, c)
        seams = 0
        for a, b in zip(chunks, chunks[1:]):
            if spos[a.j - 1] == a.hi - S.TAIL and spos[b.i] == spos[a.j - 1] + 1:
                assert b.lo == spos[a.j - 1] + 1 - S.PRE and a.hi < case.n_frames
                assert np.count_nonzero(spos == spos[a.j - 1]) == copies
                assert np.count_nonzero(spos == spos[b.i]) == copies
                seams += 1
        assert seams >= 3
        assert ("shuffled" in name) == bool(np.any(np.diff(case.pos) < 0))
    sizes = {ch.hi - ch.lo for ch in S.plan(np.sort(S.BY_NAME["fit-8192"].pos), 60_000, 8192)}
    assert {2048, 4096, 8192} <= sizes         # the one ordered size above 6,296 has ramp shapes


def test_chunk_count_cases():
    for K in (1, 2, 3, 4, 5, 9):
        case = S.BY_NAME["count-%d" % K]
        assert len(S.plan(np.sort(case.pos), case.n_frames, case.chunk_frames)) == K
        assert S.ring(K) == min(K, 4)
    for K in (5, 9):
        case = S.BY_NAME["count-%d-787" % K]
        chunks = S.plan(np.sort(case.pos), case.n_frames, 787)
        assert len(chunks) == K and all(ch.hi - ch.lo == 787 for ch in chunks)


def test_ramp_case():
    case = S.BY_NAME["ramp-8192"]
    spos = np.sort(case.pos)
    chunks = S.plan(spos, case.n_frames, 8192)
    sizes = [ch.hi - ch.lo for ch in chunks]
    assert sizes[:3] == [2048, 4096, 8192] and sizes[-1] == 2048
    assert any(2048 < s < 4096 for s in sizes) and any(4096 < s < 8192 for s in sizes)
    for ch in chunks[:-1]:      # epochs at the first and the last frame of each
        assert spos[ch.i] - S.PRE == ch.lo and spos[ch.j - 1] + S.TAIL == ch.hi
    assert spos[chunks[-1].i] - S.PRE == chunks[-1].lo


def test_recording_end_cases():
    p = plans_of(["end-clipped", "end-equal", "end-tails", "end-empty-only", "end-empty-mid"])
    N = S.BY_NAME["end-clipped"].n_frames
    assert N * 6 % 16 != 0
    last = p["end-clipped"][-1]
    assert last.hi == N and last.lo + S.chunk_at(2, last.lo, N, 1600) > N   # clipped
    assert S.BY_NAME["end-clipped"].pos.max() + S.TAIL == N                 # and no tail past it
    last = p["end-equal"][-1]
    assert last.hi == N == last.lo + 787 and last.j - last.i == 1
    for name in ("end-tails", "end-empty-mid"):
        case, chunks = S.BY_NAME[name], p[name]
        spos = np.sort(case.pos)
        assert np.all(spos[:chunks[-1].i] + S.TAIL <= N)     # tails in the last chunk only
        assert np.count_nonzero(spos[chunks[-1].i:] + S.TAIL > N) >= 3
    tails = np.sort(S.BY_NAME["end-tails"].pos)
    assert {N - S.TAIL + 1, N, N + 1, N + 99} <= set(tails.tolist())
    last = p["end-empty-only"][-1]
    assert last.lo == last.hi == N and last.j - last.i == 1
    assert S.chunk_bytes(last, 6) == (N * 6 & ~15, N * 6, 6)     # the floor's bytes alone
    assert S.chunk_bytes(last, 64)[2] == 0
    mid = S.BY_NAME["end-empty-mid"].pos
    at = np.nonzero(mid == N + S.PRE)[0]
    assert len(at) == 3 and at.min() > 0 and at.max() < len(mid) - 1 and np.any(np.diff(mid) < 0)
    assert p["end-empty-mid"][-1].lo < N


def test_phase_and_gap_cases():
    case = S.BY_NAME["phases"]
    chunks = S.plan(np.sort(case.pos), case.n_frames, case.chunk_frames)
    assert chunks[0].lo == 0
    for lay in S.LAYOUTS + [S.LAYOUT_4CH]:
        fb = S.frame_bytes(lay)
        can = {(f * fb) % 16 for f in range(16)}
        assert {(ch.lo * fb) % 16 for ch in chunks} == can, lay.name
    assert {S.frame_bytes(lay) for lay in S.LAYOUTS} == {6, 16, 64, 140}
    case = S.BY_NAME["gaps"]
    chunks = S.plan(np.sort(case.pos), case.n_frames, case.chunk_frames)
    assert all(b.lo - a.hi >= 5000 for a, b in zip(chunks, chunks[1:])) and len(chunks) == 8


def test_threaded_case():
    pos, chunks, k, bounds = S.threaded_case()
    assert len(pos) == 200 and np.all(np.diff(pos) >= 0)
    Lb, Hb, nbytes = S.chunk_bytes(chunks[k], 64)
    assert nbytes == 24 * MB == S.THREADED["chunk_frames"] * 64
    assert S.copy_split(nbytes, 8) == (3, 8 * MB) and len(bounds) == 2
    assert [S.chunk_bytes(ch, 64)[2] >> 23 for ch in chunks[:2]] == [0, 1]   # one thread before it
    inside = pos[chunks[k].i:chunks[k].j]
    assert inside[0] - S.PRE == chunks[k].lo and inside[-1] + S.TAIL == chunks[k].hi
    assert pos[chunks[k].j] == inside[-1] + 1
    for b in bounds:
        assert (b * 64 - Lb) % (8 * MB) == 0
        assert np.any((inside - S.PRE < b) & (b < inside))                    # a run straddles it
        assert np.any((inside + 175 < b) & (b < inside + S.TAIL))             # a window does
        assert np.any(inside - S.PRE == b) and np.any(inside + S.TAIL == b)


def test_remainder_case():
    pos, chunks, k = S.remainder_case()
    Lb, Hb, nbytes = S.chunk_bytes(chunks[k], 6)
    assert nbytes == 24 * MB + 2 and chunks[k].lo % 8 == 3 and chunks[k].hi < S.REMAINDER["n_frames"]
    nt, per = S.copy_split(nbytes, 8)
    assert nt == 3 and nbytes % nt != 0 and (nbytes // nt) % 64 == 0
    assert nt * ((nbytes // nt + 63) & ~63) == nbytes - 2      # the floored quotient's loss
    assert nt * per >= nbytes
    assert pos[chunks[k].j - 1] + S.TAIL == chunks[k].hi       # an epoch reads the last frame
    assert len(pos) <= 40
