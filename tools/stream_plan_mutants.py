#!/usr/bin/env python3
"""One-edit mutants of csrc/stream_plan.h against tests/test_stream_cases.py, on the CPU only (they
change which bytes a kernel may address, so none is ever run on a device): each mutant is a copy of
the header with one textual edit in a temporary directory, which the test module takes through
EEGFX_STREAM_PLAN_INCLUDE.  Prints, for each, the tests that fail; exits 1 if any mutant passes.
    tools/stream_plan_mutants.py > profiles/streamed_seams/mutants.log
"parent" restores the arithmetic from before the bound on chunk_frames (the buffer sized by
chunk_frames * FB, no cap) and "per-floored" the copy split from before its fix."""
import os
import re
import subprocess
import sys
import tempfile

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HEADER = os.path.join(REPO, "eeg_dataanalysispackage_amd", "csrc", "stream_plan.h")

MUTANTS = {
    "bisection bound one frame later": [
        ("hi + EEGFX_PRESTIMULUS - kStreamSpan) - spos",
         "hi + EEGFX_PRESTIMULUS - kStreamSpan + 1) - spos")],
    "Lb not floored": [("(c.lo * FB) & ~(int64_t)15", "(c.lo * FB)")],
    "hi not clipped to n_frames": [
        ("std::min(lo + stream_chunk_at((int64_t)plan.size(), lo, last, chunk_frames), n_frames);",
         "lo + stream_chunk_at((int64_t)plan.size(), lo, last, chunk_frames);")],
    "per not rounded up": [
        ("((bytes + nt - 1) / nt + 63) & ~(size_t)63", "(bytes / nt) & ~(size_t)63")],
    "R taken as 4 for a 3-chunk plan": [
        ("return std::min(chunks, kStreamRing);",
         "return chunks == 3 ? 4 : std::min(chunks, kStreamRing);")],
    "per-floored (the copy split before its fix)": [
        ("((bytes + nt - 1) / nt + 63) & ~(size_t)63", "(bytes / nt + 63) & ~(size_t)63")],
    "parent (chunk_frames unbounded, buffers sized by it)": [
        ("return std::min(chunk_frames, cap);", "(void)cap; return chunk_frames;"),
        ("struct StreamChunk {", "inline int64_t g_chunk_frames = 0;\nstruct StreamChunk {"),
        ("  const int64_t last = spos[n - 1]",
         "  g_chunk_frames = chunk_frames;\n  const int64_t last = spos[n - 1]"),
        ("return (most + 128 + 255) & ~(size_t)255;",
         "(void)most; return ((size_t)(g_chunk_frames * FB) + 128 + 255) & ~(size_t)255;")],
}


def main():
    text = open(HEADER).read()
    survived = []
    for name, edits in MUTANTS.items():
        mutated = text
        for old, new in edits:
            assert mutated.count(old) == 1, (name, old)
            mutated = mutated.replace(old, new)
        with tempfile.TemporaryDirectory() as d:
            open(os.path.join(d, "stream_plan.h"), "w").write(mutated)
            env = dict(os.environ, EEGFX_STREAM_PLAN_INCLUDE=d)
            r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-p", "no:cacheprovider",
                                os.path.join(REPO, "tests", "test_stream_cases.py")],
                               env=env, capture_output=True, text=True)
        failed = re.findall(r"^(?:FAILED|ERROR) \S+::(\S+)", r.stdout, re.M)
        ubsan = sorted(set(re.findall(r"runtime error: ([^\n\\']+)", r.stdout)))
        print("mutant: %s" % name)
        for t in failed:
            print("    fails: %s" % t)
        for u in ubsan[:4]:
            print("    UBSan: %s" % u.strip())
        if not failed:
            print("    PASSES EVERY TEST")
            survived.append(name)
        print()
    print("%d mutants, %d survived" % (len(MUTANTS), len(survived)))
    return 1 if survived else 0


if __name__ == "__main__":
    sys.exit(main())
