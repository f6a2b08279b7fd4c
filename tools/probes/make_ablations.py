#!/usr/bin/env python3
"""Regenerates tools/probes/ablations/*.patch against the current product sources.

Each ablation is a list of exact text replacements in fused.hip / wide.hip / dwt8.h.  When the
product changes, rerun this script; a replacement whose text no longer exists fails loudly.
build_probes.sh applies the patches to copies of the sources and builds window_probe_<name>;
tools/ablation_study.sh measures them.

  python3 tools/probes/make_ablations.py
"""
import difflib
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "..", "eeg_dataanalysispackage_amd", "csrc")
FILES = ("fused.hip", "wide.hip", "dwt8.h")

DMA_ISSUE = """  if (dma_issue<CT, C, NT>(raw, nbytes, wb, e0, ne, win, w, lane, rows))
    dma_fixup<CT, C>(raw, nbytes, wb, e0, ne, win, w, lane, rows);"""

SIGNAL_CASCADE = """  signal_cascade<FAST, TRACKABLE>([&](int k) { return (float)own[k * CT]; }, r, b, lane & ~7, s,
                                  a6, d6, &ymax);"""

FMA_BODY = """#pragma unroll
  for (int q = 0; q < 3; ++q) {
    A0[q] = n == 0 ? x1 * R[q] : __builtin_fma(x1, R[q], A0[q]);
    if (n + 32 * (3 * q + 2) < 280)
      Ai[q] = n == 0 ? x0 * R[3 + q] : __builtin_fma(x0, R[3 + q], Ai[q]);
    Bp[q] = n == 0 ? xp * R[6 + q] : __builtin_fma(xp, R[6 + q], Bp[q]);
    Bm[q] = n == 0 ? xm * R[9 + q] : __builtin_fma(xm, R[9 + q], Bm[q]);
  }"""

def baseline_tile(t):
    return [("fused.hip", "  constexpr int kTile = 64;",
             f"  constexpr int kTile = {t};  // ablation: {t}-epoch tiles")]


ABLATIONS = {
    "baseline32": (
        "baseline_kernel on 32-epoch tiles (2 waves, 20 KB of LDS per workgroup)",
        baseline_tile(32)),
    "baseline128": (
        "baseline_kernel staging whole 128-byte lines: each epoch's DMA starts at floor128 of its "
        "600-byte run and its lanes cover only the lines the run touches (VERDICT r03 item 5), "
        "32-epoch tiles",
        baseline_tile(32) + [
            ("fused.hip",
             "  static constexpr int BASEQ = (kPre * FB + 15) / 16 + 1;    // 39 quads (600 B + misalignment)",
             "  static constexpr int BASEQ = (kPre * FB + 127) / 128 * 8 + 8;  // ablation: whole lines"),
            ("fused.hip",
             "    tB[tid] = R | (((R & ~(int64_t)15) + 16 * G::BASEQ <= nbytes) ? 0 : 1);",
             "    tB[tid] = R | (((R & ~(int64_t)127) + 16 * G::BASEQ <= nbytes) ? 0 : 1);"),
            ("fused.hip",
             "        const int64_t Rq = (int64_t)(((uint64_t)whi << 32) | (wlo & ~15u));\n"
             "        dma16_s<STREAM>(",
             "        const int64_t Rq = (int64_t)(((uint64_t)whi << 32) | (wlo & ~127u));\n"
             "        if (16 * lane < (int)(((wlo & 126u) + kPre * G::FB + 127) & ~127u))  // lines touched\n"
             "          dma16_s<STREAM>("),
            ("fused.hip",
             "                   load16(raw, nbytes, (W & ~(int64_t)15) + 16 * lane));",
             "                   load16(raw, nbytes, (W & ~(int64_t)127) + 16 * lane));"),
            ("fused.hip",
             "  const int16_t* src = (const int16_t*)((const uint8_t*)(stage + e * G::BSTR) + (tB[e] & 14)) +",
             "  const int16_t* src = (const int16_t*)((const uint8_t*)(stage + e * G::BSTR) + (tB[e] & 126)) +"),
        ]),
    "baseline_t128": (
        "baseline_kernel on 128-epoch tiles (6 waves, 81 KB of LDS: two workgroups per CU)",
        baseline_tile(128)),
    "noguard": (
        "the fma conditioning guard compiled out of the window kernels (no per-signal X^2, no "
        "per-row check, no rare path): A/B of its cost (round 4)",
        [("dwt8.h", "#define EEGFX_GUARD 1", "#define EEGFX_GUARD 0")]),
    "cascade": (
        "fma filter bank as the round-2 level-by-level cascade with partial-sum halos "
        "(A/B against the collapsed filter)",
        [("dwt8.h", "#define EEGFX_COLLAPSED 1", "#define EEGFX_COLLAPSED 0")]),
    "direct": (
        "each pair's update in the direct form (18 multiply-adds) instead of the four-point Toom "
        "form (12 + two adds): A/B of the change",
        [("dwt8.h", "#define EEGFX_TOOM 1", "#define EEGFX_TOOM 0")]),
    "nodma": (
        "no window DMA: removes the HBM window reads and the LDS writes; LDS reads, decode and "
        "fp64 kept (wrong results)",
        [("fused.hip", DMA_ISSUE,
          "  (void)rows;  // ablation: no window DMA (no HBM window reads, no LDS writes)")]),
    "l2src": (
        "window DMA from a 2 MB L2-resident region (same addresses mod 2 MB): removes HBM reads "
        "only (wrong results)",
        [("fused.hip", "    const uint8_t* sb = raw + Bq;",
          "    const uint8_t* sb = raw + (Bq & 0x1FFFF0);  // ablation: L2-resident source")]),
    "regdirect": (
        "no LDS staging: each lane loads its 64 samples (128 B, L2-resident region) into VGPRs; "
        "no window DMA, no LDS sample reads (wrong results)",
        [("fused.hip", DMA_ISSUE,
          "  (void)rows;  // ablation: no LDS staging; the lane's 64 samples come from VGPRs"),
         ("fused.hip", SIGNAL_CASCADE,
          """  (void)own;
  u32x4_a4 q[8];
  {
    const int64_t wv = mine ? wb[e0 + el] : 0;
    const u32x4_a16* src = (const u32x4_a16*)(raw + ((wv + 384 * s + 128 * w) & 0x1FFFF0));
#pragma unroll
    for (int i = 0; i < 8; ++i) q[i] = src[i];
  }
  dwt8_collapsed_cascade([&](int k) {
    const uint32_t v = q[k >> 3][(k >> 1) & 3];
    return (float)(int16_t)((k & 1) ? (v >> 16) : (v & 0xffffu));
  }, r, b, lane & ~7, s, a6, d6);""")]),
    "noldsread": (
        "no LDS sample reads: each sample is an opaque per-lane float plus its index (one fp32 "
        "add in place of the int16 conversion); window DMA, decode and fp64 kept (wrong results)",
        [("fused.hip", SIGNAL_CASCADE,
          "  float q = (float)((int)(uintptr_t)own & 1023);  // ablation: no LDS sample reads\n"
          "  asm volatile(\"\" : \"+v\"(q));\n"
          "  signal_cascade<FAST, TRACKABLE>([&](int k) { return q + (float)k; }, r, b, lane & ~7, s,\n"
          "                                  a6, d6, &ymax);")]),
    "nofp64": (
        "fp64 filter bank removed: the 440 multiply-adds and adds per lane become 64 fp64 adds; "
        "DMA, LDS reads and decode kept (wrong results)",
        [("dwt8.h", FMA_BODY, """  (void)R;  // ablation: no fp64 filter work, the decoded samples are summed
  if (n == 0) {
    for (int q = 0; q < 3; ++q) { A0[q] = x1; Ai[q] = x0; Bp[q] = xp; Bm[q] = xm; }
  } else { A0[n % 3] += x1; Ai[n % 3] += x0; }""")]),
}


def main():
    src = {f: open(os.path.join(CSRC, f)).read() for f in FILES}
    out_dir = os.path.join(HERE, "ablations")
    os.makedirs(out_dir, exist_ok=True)
    for old in os.listdir(out_dir):
        if old.endswith(".patch"):
            os.remove(os.path.join(out_dir, old))
    for name, (what, edits) in ABLATIONS.items():
        new = dict(src)
        for f, a, b in edits:
            if a not in new[f]:
                sys.exit(f"ablation {name}: text not found in {f}:\n{a}")
            new[f] = new[f].replace(a, b, 1)
        lines = [f"# ablation: {what}\n"]
        for f in FILES:
            if new[f] != src[f]:
                lines += difflib.unified_diff(src[f].splitlines(True), new[f].splitlines(True),
                                              f"a/{f}", f"b/{f}")
        with open(os.path.join(out_dir, name + ".patch"), "w") as fh:
            fh.writelines(lines)
        print(name)


if __name__ == "__main__":
    main()
