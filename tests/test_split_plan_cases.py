"""The host plan of the split kept per shard (csrc/split_plan.h through eegfx_split_shard_plan; CPU
only) against pipeline.java_shuffle_permutation / reference_split and the
shard ranges of eegfx_shard_range: every row in exactly one list of exactly one shard, positions
increasing, the training rows summing to (int)(n * fraction), and the rows scattered by position
giving back the reference's two lists.  Ranges clipped as a failed load clips them, and the
entry's refusals, follow.  tests/c_abi/split_plan_check.cpp includes the header alone: built with
AddressSanitizer + UBSan, the runtimes linked statically, and run as a plain program, it must give
the entry's lists on every case."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import eeg_dataanalysispackage_amd as fx
from eeg_dataanalysispackage_amd import _lib
from eeg_dataanalysispackage_amd.pipeline import java_shuffle_permutation, reference_split
from eeg_dataanalysispackage_amd.sharding import native_shard_range
from conftest import REPO

N = (0, 1, 2, 3, 11, 27, 64, 65, 1000)
SHARDS = (1, 2, 3, 5, 64)
FRACTIONS = (0.0, 0.7, 1.0)


def plan(n, first, count, seed=1, fraction=0.7):
    """(train idx, train pos, test idx, test pos) of the rows [first, first + count)."""
    idx = np.full(max(count, 1), -7, dtype=np.int64)
    pos = np.full(max(count, 1), -7, dtype=np.int64)
    a, b = ctypes.c_int64(-1), ctypes.c_int64(-1)
    _lib.check(fx.lib().eegfx_split_shard_plan(n, first, count, seed, fraction, _lib.ptr(idx),
                                               _lib.ptr(pos), ctypes.byref(a), ctypes.byref(b)))
    a, b = a.value, b.value
    assert a >= 0 and b >= 0 and a + b == count
    return idx[:a], pos[:a], idx[a:count], pos[a:count]


def check_ranges(n, ranges, seed, fraction):
    train, test = reference_split(n, seed, fraction)
    got_train = np.full(len(train), -1, dtype=np.int64)
    got_test = np.full(len(test), -1, dtype=np.int64)
    seen = np.zeros(n, dtype=np.int64)
    n_train = 0
    for first, count in ranges:
        ti, tp, ei, ep = plan(n, first, count, seed, fraction)
        n_train += len(ti)
        for idx, pos, into in ((ti, tp, got_train), (ei, ep, got_test)):
            assert np.all((idx >= 0) & (idx < count))
            assert np.all(np.diff(pos) > 0)                  # strictly increasing within a list
            assert np.all((pos >= 0) & (pos < len(into)))
            assert np.all(into[pos] == -1)                   # no position twice
            into[pos] = first + idx
            np.add.at(seen, first + idx, 1)
    covered = np.zeros(n, dtype=np.int64)
    for first, count in ranges:
        covered[first:first + count] += 1
    assert np.array_equal(seen, covered)                     # every row of a range exactly once
    assert n_train == sum(1 for g in train if covered[g])
    if covered.all():
        assert n_train == int(n * fraction)
        assert got_train.tolist() == train and got_test.tolist() == test


@pytest.mark.parametrize("fraction", FRACTIONS)
@pytest.mark.parametrize("k", SHARDS)
@pytest.mark.parametrize("n", N)
def test_plan_reproduces_the_reference_split(n, k, fraction):
    ranges = []
    for r in range(k):
        s, e = native_shard_range(n, r, k)
        ranges.append((s, e - s))
    assert sum(c for _, c in ranges) == n
    if k > n:
        assert any(c == 0 for _, c in ranges)                # more shards than rows
    check_ranges(n, ranges, 1, fraction)


def test_other_seeds_and_the_permutation_itself():
    for seed in (0, 1, 42, -3, 2 ** 40 + 5):
        n = 65
        perm = java_shuffle_permutation(n, seed)
        ti, tp, ei, ep = plan(n, 0, n, seed, 0.7)
        cut = int(n * 0.7)
        assert tp.tolist() == list(range(cut)) and ep.tolist() == list(range(n - cut))
        assert ti.tolist() == perm[:cut] and ei.tolist() == perm[cut:]
        check_ranges(n, [(0, 20), (20, 1), (21, 44)], seed, 0.7)


def test_clipped_ranges():
    """The ranges a failed load leaves: the planned ranges of 27 rows over 5 shards clipped to the
    11 rows kept -- the split is of the 11 rows, the later shards hold nothing."""
    planned, kept, k = 27, 11, 5
    ranges = []
    for r in range(k):
        s, e = native_shard_range(planned, r, k)
        ranges.append((min(s, kept), min(e, kept) - min(s, kept)))
    assert [c for _, c in ranges] == [6, 5, 0, 0, 0]
    for fraction in FRACTIONS:
        check_ranges(kept, ranges, 1, fraction)


def test_a_range_inside_the_list():
    """One shard alone: its rows and no other, wherever it lies."""
    for first, count in ((0, 0), (3, 0), (27, 0), (5, 1), (26, 1), (9, 13)):
        check_ranges(27, [(first, count)], 1, 0.7)


def test_refusals():
    def rc(n, first, count, fraction=0.7, null=False):
        buf = np.zeros(max(count, 1), dtype=np.int64)
        a, b = ctypes.c_int64(), ctypes.c_int64()
        p = None if null else _lib.ptr(buf)
        return fx.lib().eegfx_split_shard_plan(n, first, count, 1, fraction, p, p,
                                               ctypes.byref(a), ctypes.byref(b))
    assert rc(10, 0, 10) == _lib.EEGFX_OK
    assert rc(10, 0, 0, null=True) == _lib.EEGFX_OK
    for bad in ((10, -1, 2), (10, 0, 11), (10, 9, 2), (10, 11, 0), (10, 0, -1), (-1, 0, 0)):
        assert rc(*bad) == _lib.EEGFX_EINVAL, bad
    for fraction in (-0.1, 1.1, float("nan")):
        assert rc(10, 0, 10, fraction) == _lib.EEGFX_EINVAL
        assert b"train_fraction" in fx.lib().eegfx_last_error()
    assert rc(10, 0, 10, null=True) == _lib.EEGFX_EINVAL


def test_header_alone_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "split_plan_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror",
                    "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan",
                    "-fno-sanitize-recover=all",
                    "-I", os.path.join(REPO, "eeg_dataanalysispackage_amd", "csrc"),
                    os.path.join(REPO, "tests", "c_abi", "split_plan_check.cpp"), "-o", exe],
                   check=True)
    cases, lines = [], []
    for n in N:
        perm = java_shuffle_permutation(n, 1)
        for k in SHARDS:
            for fraction in FRACTIONS:
                for r in range(k):
                    s, e = native_shard_range(n, r, k)
                    cases.append((n, s, e - s, fraction))
                    lines.append(" ".join(map(str, [n, int(n * fraction), s, e - s] + perm)))
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, \
        r.stdout[-2000:] + r.stderr[-4000:]
    out = r.stdout.splitlines()
    assert out[-1] == "split_plan_check ok" and len(out) == len(cases) + 1
    for (n, first, count, fraction), line in zip(cases, out):
        got = [int(v) for v in line.split()]
        ti, tp, ei, ep = plan(n, first, count, 1, fraction)
        assert got[:2] == [len(ti), len(ei)]
        assert got[2:2 + count] == ti.tolist() + ei.tolist()
        assert got[2 + count:] == tp.tolist() + ep.tolist()
