"""Inputs shared by tests/test_odp_multi.py and tests/test_gpu_odp_multi.py: the two-file info
file over copies of the golden recordings, and a synthetic directory of BrainVision recordings
(int16 and float32, MULTIPLEXED and VECTORIZED) whose markers hit the corners a sharded load has to
keep: skipped positions, zero-padded tails, pos - 100 == n_frames, a file whose markers are all
rejected by the balance, a listed file that does not exist."""
import os
import shutil

import numpy as np

from conftest import DATA
from oracle import oracle

CHANNELS7 = ("O1", "Cz", "F3", "Pz", "O2", "Fz", "C4")  # Fz, Cz, Pz outside the first 3 columns
RES7 = (0.1, 0.25, 0.1, 0.5, 0.1, 0.125, 0.1)
FZ_CZ_PZ = [CHANNELS7.index(n) for n in ("Fz", "Cz", "Pz")]
SYN_ORDER = ["a_int16", "missing", "b_float", "c_vector", "d_rejected", "e_tail"]


def two_file_info(tmp_path):
    """Copies of the two golden recordings under tmp_path/DoD and an info file that lists both:
    the target / non-target balance carries from the first file into the second."""
    dst = tmp_path / "DoD"
    dst.mkdir()
    for base in ("DoD2015_01", "DoD_2015_02"):
        for ext in (".eeg", ".vhdr", ".vmrk"):
            shutil.copy(os.path.join(DATA, "DoD", base + ext), str(dst / (base + ext)))
    info = tmp_path / "info2.txt"
    info.write_text("DoD/DoD2015_01.eeg 1 1\nDoD/DoD_2015_02.eeg 4\n")
    return str(info)


def write_brainvision(dirpath, name, rec, marks, fmt="INT_16", vectorized=False,
                      channels=CHANNELS7, res=RES7):
    """One .eeg / .vhdr / .vmrk triple.  rec: [n_frames][len(channels)]; marks: (stimulus number,
    position) pairs, or a ready marker line (str) written as it is."""
    rec = np.asarray(rec)
    data = rec.astype("<i2" if fmt == "INT_16" else "<f4")
    (np.ascontiguousarray(data.T) if vectorized else data).tofile(str(dirpath / (name + ".eeg")))
    chans = "".join(f"Ch{i + 1}={nm},,{r},µV\n" for i, (nm, r) in enumerate(zip(channels, res)))
    (dirpath / (name + ".vhdr")).write_text(
        "Brain Vision Data Exchange Header File Version 1.0\n\n[Common Infos]\nCodepage=UTF-8\n"
        f"DataFile={name}.eeg\nMarkerFile={name}.vmrk\nDataFormat=BINARY\n"
        f"DataOrientation={'VECTORIZED' if vectorized else 'MULTIPLEXED'}\n"
        f"NumberOfChannels={len(channels)}\nSamplingInterval=1000\n\n"
        f"[Binary Infos]\nBinaryFormat={fmt}\n\n[Channel Infos]\n" + chans, encoding="utf-8")
    lines = []
    for i, m in enumerate(marks):
        lines.append(m if isinstance(m, str) else f"Mk{i + 2}=Stimulus,S  {m[0]},{int(m[1])},1,0\n")
    (dirpath / (name + ".vmrk")).write_text(
        "Brain Vision Data Exchange Marker File, Version 1.0\n\n[Common Infos]\nCodepage=UTF-8\n"
        f"DataFile={name}.eeg\n\n[Marker Infos]\nMk1=New Segment,,1,1,0,20150128095308551177\n"
        + "".join(lines), encoding="utf-8")


def synth(rng, n_frames, fmt):
    walk = np.cumsum(rng.integers(-40, 41, size=(n_frames, 7)), axis=0)
    rec = rng.integers(-3000, 3000, size=(1, 7)) + walk + rng.integers(-300, 300, size=(n_frames, 7))
    if fmt == "INT_16":
        return np.clip(rec, -32768, 32767).astype(np.int16)
    return (rec * 0.37).astype(np.float32)


def alternating(positions, first=1):
    """Markers that alternate target (stimulus 1) / non-target (2): with guessed number 1 the
    balanced selection keeps every one that has a legal position."""
    return [(1 + (i + first + 1) % 2, p) for i, p in enumerate(positions)]


def synthetic_directory(tmp_path):
    """Five recordings of 3,000-6,000 frames x 7 channels plus one listed file that does not
    exist; guessed number 1 everywhere.  35 epochs: 6 + 9 + 8 + 0 + 12.  Returns the info path."""
    d = tmp_path / "syn"
    d.mkdir()
    rng = np.random.default_rng(20260)
    specs = [  # name, frames, format, vectorized, markers
        # pos 40 < 100 is skipped; 2900 runs past the end (zero padded); 3100 - 100 == n_frames:
        # an all-zero epoch, a NaN row.  6 accepted, the balance is back at 0.
        ("a_int16", 3000, "INT_16", False, alternating([40, 100, 431, 1200, 1999, 2900, 3100])),
        # 9 accepted, the last a target: the balance leaves at +1
        ("b_float", 4100, "IEEE_FLOAT_32", False,
         alternating([150, 777, 1500, 2222, 3000, 3349, 3351, 3900, 4150])),
        # the leading target is rejected (balance +1), 8 accepted, the balance leaves at +1
        ("c_vector", 5003, "INT_16", True,
         alternating([101, 900, 1701, 2500, 3300, 4100, 4253, 4900, 5102])),
        # targets only at balance +1: every marker is rejected
        ("d_rejected", 3500, "INT_16", False, [(1, p) for p in (500, 900, 1300, 1700)]),
        # starts with a non-target; 12 accepted; 6100 - 100 == n_frames
        ("e_tail", 6000, "INT_16", False,
         alternating([100, 600, 1333, 2048, 2800, 3500, 4200, 4800, 5251, 5600, 5900, 6100],
                     first=0)),
    ]
    for name, nf, fmt, vec, marks in specs:
        write_brainvision(d, name, synth(rng, nf, fmt), marks, fmt, vec)
    info = tmp_path / "syn_info.txt"
    info.write_text("".join(f"syn/{n}.eeg 1\n" for n in SYN_ORDER))
    return str(info)


def oracle_plan(info, balance=0):
    """What loadData selects from the files an info file lists, by the oracle alone: read_vmrk and
    plan_markers per file in list order, the balance carried from file to file (and in from an
    earlier load), a listed file that does not exist skipped.  The frames of a file come from its
    size.  Returns (positions, labels, file indices, balance)."""
    pos, lab, fid = [], [], []
    for f, (name, guessed) in enumerate(oracle.load_info_txt(info).items()):
        eeg = os.path.join(os.path.dirname(info), name)
        if not os.path.isfile(eeg):
            continue
        h = oracle.read_vhdr(eeg[:-4] + ".vhdr")
        frame = h["n_channels"] * (2 if h["binary_format"] == "INT_16" else 4)
        p, l, balance = oracle.plan_markers(oracle.read_vmrk(eeg[:-4] + ".vmrk"),
                                            os.path.getsize(eeg) // frame, guessed, balance)
        pos += p
        lab += l
        fid += [f] * len(p)
    return pos, lab, fid, balance
