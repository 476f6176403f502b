"""The file-end cut of the burst stages' records (tfrec_amd/host/job.h: cut_at_file_end, which device_worker applies to what -M, -Q
and -C read) through tests/merge_driver.cpp, a stand-alone program under the address and undefined-behaviour sanitizers.  The
expected lines are the restatements' line() of records cut by this module's own few lines."""
import os
import subprocess

import numpy as np
import pytest

import parity
from tfrec_amd import burst, capture, clock, envelope

B = 8192
OPEN = capture.RUN_OPEN
FILES = [("a.iq", 1), ("b.iq", 2)]
SLOTS = [1, -1, 0]  # the batch's map: slot 0 holds b.iq, slot 1 is idle, slot 2 holds a.iq
# (file, start_sample, n_samples) in table order -- by slot --, and what becomes of each
RECORDS = [(1, 100, 500),             # inside b.iq: kept whole
           (1, 2 * B - 300, 1000),    # reaches over b.iq's end: 300 samples are kept
           (-1, 0, 700),              # an idle slot's: dropped
           (0, B - 400, 400),         # ends exactly at a.iq's end: kept whole, its flags as they were
           (0, B, 50),                # starts at a.iq's end: dropped
           (0, B + 900, 50),          # starts behind it: dropped
           (7, 0, 700)]               # of a file no slot holds -- a stream index beyond the map: dropped


@pytest.fixture(scope="module")
def merge_driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("burst_cut") / "merge_driver")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(parity.ROOT, "tests", "merge_driver.cpp")])
    return exe


def cut(r, cut_opens):
    """This module's statement of the cut: the record as the job keeps it, or None."""
    f = int(r["stream"])
    if f not in [s for s in SLOTS if s >= 0]:
        return None
    start, n, end = int(r["start_sample"]), int(r["n_samples"]), FILES[f][1] * B
    if start >= end:
        return None
    o = r.copy()
    if start + n > end:
        o["n_samples"] = end - start
        if cut_opens:
            o["flags"] |= OPEN
    return o


def burst_records():
    r = np.zeros(len(RECORDS), dtype=burst.BURST_DTYPE)
    r["pwr_max"], r["n_products"], r["thresh"] = 900, 320, 500
    r["hist"][:, 3], r["hist"][:, 60] = 200, 120  # two occupied bins: a centre and a deviation
    return r


def envelope_records():
    r = np.zeros(len(RECORDS), dtype=envelope.ENVELOPE_DTYPE)
    r["n_over"], r["last_over"], r["energy_head"], r["energy_tail"], r["thresh"] = 150, 199, 4000000, 900, 500
    return r


def clock_records():
    r = np.zeros(len(RECORDS), dtype=clock.CLOCK_DTYPE)
    r["n_segments"], r["thresh"] = 3, 500
    r["spec"][:, 40], r["spec"][:, 41], r["spec"][:, 39] = 1000, 700, 300
    return r


STAGES = {"burst": (burst_records, burst.line, False,
                    ("flags", "start_sample", "n_samples", "thresh", "pwr_max", "n_products", "sum_dot", "sum_crs", "energy", "hist")),
          "envelope": (envelope_records, envelope.line, True,
                       ("flags", "start_sample", "n_samples", "thresh", "n_over", "last_over", "energy_head", "energy_tail", "n_gaps", "max_gap",
                        "lead_not_over", "nprod_head", "dot_head", "crs_head", "dot_tail", "crs_tail", "nprod_tail")),
          "clock": (clock_records, clock.line, True, ("flags", "start_sample", "n_samples", "thresh", "n_segments", "n_silent", "spec"))}


@pytest.mark.parametrize("stage", sorted(STAGES))
def test_the_host_cuts_a_record_at_its_files_end(merge_driver, stage):
    """Two files of 1 and 2 blocks in one batch of 2 blocks.  A record that is not OPEN ends its burst where it stands in the table;
    one that the cut made OPEN -- the envelope's and the clock's, not the meter's -- is flushed with its file, behind the table."""
    make, line, cut_opens, fields = STAGES[stage]
    recs = make()
    lines = ["file %s %d" % f for f in FILES] + ["batch 2 " + " ".join("%d" % s for s in SLOTS)]
    for r, (f, start, n) in zip(recs, RECORDS):
        r["start_sample"], r["n_samples"] = start, n
        lines.append("rec %d " % f + " ".join("%d" % int(x) for k in fields for x in np.atleast_1d(r[k])))
        r["stream"] = f if f >= 0 else 0xffffffff
    kept = [o for o in (cut(r, cut_opens) for r in recs) if o is not None]
    assert [(int(o["stream"]), int(o["start_sample"]), int(o["n_samples"])) for o in kept] == [(1, 100, 500), (1, 2 * B - 300, 300), (0, B - 400, 400)]
    assert [int(o["flags"]) for o in kept] == [0, OPEN if cut_opens else 0, 0]
    want = [line(FILES[int(o["stream"])][0], o) for o in kept if not int(o["flags"]) & OPEN]
    want += [line(FILES[f][0], o) for f in SLOTS for o in kept if f == int(o["stream"]) and int(o["flags"]) & OPEN]
    out = subprocess.run([merge_driver, stage], input="".join(ln + "\n" for ln in lines), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.splitlines() == want and len(want) == 3
    assert [w.split()[1] for w in want] == (["b.iq", "a.iq", "b.iq"] if cut_opens else ["b.iq", "b.iq", "a.iq"])
    assert all(w.split()[-1] != "-" for w in want[:2])  # the whole records have their summaries
    if stage == "envelope":  # ... and the cut one, OPEN, has no ratio: its tail is not whole
        assert want[2].split()[3:5] == ["300", "200"] and want[2].endswith(" - -")
