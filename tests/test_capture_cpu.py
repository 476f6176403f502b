"""The squelched recorder without a GPU (tfrec_amd_enable_capture, tfrec_gpu -S): the restatement
tfrec_amd/capture.py against a per-sample simulation of the reference's loops and against levels.py, its behaviour under cutting,
the struct and the exports, and what tfrec_gpu decides before it opens a device.

Everything is an exact integer; nothing here has a tolerance."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import parity
from tfrec_amd import api, capture, levels
from meter_rows import SUBSETS, crafted_dec

B = levels.BLOCK_DEC
PAIR_GAPS = lambda W: (W - 1, W, W + 1, W + 2)  # noqa: E731  (crafted_dec's trigger pairs, from sample 200 on)


def sample_set(runs, pool, base=0):
    """{(n, I, Q)} over all runs of one stream; base: the stream's samples ahead of these runs' start_sample origin."""
    out = set()
    for r in runs:
        o, n = int(r["pool_offset"]), int(r["n_samples"])
        for k in range(n):
            out.add((base + int(r["start_sample"]) + k, int(pool[o + k][0]), int(pool[o + k][1])))
    return out


def assert_layout(runs, pool, dec):
    """The table is ordered, its offsets are the exclusive prefix sum of the lengths, and the pool holds dec's pairs."""
    d = np.asarray(dec).reshape(-1, 2)
    assert np.array_equal(runs["pool_offset"], np.concatenate([[0], np.cumsum(runs["n_samples"])[:-1]]).astype(np.uint64))
    assert len(pool) == int(runs["n_samples"].sum())
    assert (np.diff(runs["start_sample"]) > runs["n_samples"][:-1]).all()  # maximal: at least one sample between two runs
    for r in runs:
        a, o, n = int(r["start_sample"]), int(r["pool_offset"]), int(r["n_samples"])
        assert n >= 1 and np.array_equal(pool[o:o + n], d[a:a + n])


@pytest.mark.parametrize("types", SUBSETS, ids=["%02x" % t for t in SUBSETS])
def test_captures_equal_the_per_sample_simulation(types):
    W = max(levels.windows(types))
    dec, loud = crafted_dec(W, types)
    M = len(dec)
    for thresh in (500, 0, 60):
        runs, pool, _ = capture.captures(dec, types, thresh)
        want, want_pool, _ = capture.captures_bruteforce(dec, types, thresh)
        assert np.array_equal(runs, want) and np.array_equal(pool, want_pool), (types, thresh)
        assert_layout(runs, pool, dec)
    runs, pool, st = capture.captures(dec, types, 500)  # fixed threshold 500: only the loud samples trigger
    assert (runs["thresh"] == 500).all() and (runs["stream"] == 0).all() and st["n"] == M
    start, end = runs["start_sample"], runs["start_sample"] + runs["n_samples"]
    # Pairs of triggers d apart, at p and p + d: the first covers [p, p + W), the second [p + d, p + d + W).  They are one run iff
    # no sample lies between them uncovered, p + d <= p + W; otherwise a run of W samples and one that starts at p + d.
    pos = 200
    for d in PAIR_GAPS(W):
        assert pos in loud and pos + d in loud
        here = runs[(start >= pos) & (start < pos + d + W)]
        derived = 1 if pos + d <= pos + W else 2
        assert len(here) == derived, (d, W)
        assert here["start_sample"].tolist() == [pos, pos + d][:derived]
        assert here["n_samples"].tolist() == ([d + W] if derived == 1 else [W, W])
        assert (here["flags"] == 0).all()
        pos += d + W + 100
    assert [1 if d <= W else 2 for d in PAIR_GAPS(W)] == [1, 1, 2, 2]  # (what the derivation amounts to for these distances)
    # a trigger at block 0's last sample: its run begins there (no pre-roll) and crosses into block 1; the one W / 2 ahead of
    # the boundary between blocks 1 and 2 crosses that
    r = runs[start == B - 1]
    assert len(r) == 1 and r["n_samples"][0] == W and r["flags"][0] == 0
    r = runs[start == 2 * B - W // 2]
    assert len(r) == 1 and r["n_samples"][0] == W and end[start == 2 * B - W // 2][0] > 2 * B
    # ... and one at the input's last sample: a run of that sample, open
    last = runs[-1]
    assert M - 1 in loud and int(last["start_sample"] + last["n_samples"]) == M and last["flags"] & capture.RUN_OPEN
    assert (runs[:-1]["flags"] == 0).all()


def test_a_silent_stream_and_one_triggered_throughout():
    quiet = np.zeros((2 * B, 2), dtype=np.int16)
    for f in (capture.captures, capture.captures_bruteforce):
        runs, pool, st = f(quiet, 0x2F, 500)
        assert len(runs) == 0 and pool.shape == (0, 2) and runs.dtype == capture.RUN_DTYPE
    loud = np.full((2 * B, 2), 900, dtype=np.int16)
    loud[:, 1] = np.arange(2 * B) % 1000
    for f in (capture.captures, capture.captures_bruteforce):
        runs, pool, st = f(loud, 0x2F, 500)
        assert len(runs) == 1 and runs[0]["start_sample"] == 0 and runs[0]["n_samples"] == 2 * B
        assert runs[0]["flags"] == capture.RUN_OPEN and np.array_equal(pool, loud)
        more, pool2, _ = f(loud[:B], 0x2F, 500, st)
        assert len(more) == 1 and more[0]["flags"] == capture.RUN_CONTINUES | capture.RUN_OPEN and more[0]["start_sample"] == 2 * B
    # the auto threshold: a run reports the threshold of the block it starts in
    runs, _, _ = capture.captures(np.concatenate([quiet] * 3 + [loud]), 0x2F, 0)
    lv, _ = levels.levels(np.concatenate([quiet] * 3 + [loud]), 0x2F, 0)
    assert len(runs) == 1 and runs[0]["start_sample"] == 6 * B and runs[0]["thresh"] == lv["thresh"][6] == 498


def _shifted(runs, by):
    r = runs.copy()
    r["start_sample"] += by
    return r


@pytest.mark.parametrize("thresh", [500, 0])
def test_cutting_changes_only_the_split_and_the_flags(thresh):
    types = 0x2F
    W = max(levels.windows(types))
    dec, loud = crafted_dec(W, 77, n_blocks=4)
    one, pool, _ = capture.captures(dec, types, thresh)
    whole = sample_set(one, pool)
    assert len(whole) == len(pool) > 0
    for sizes in ((1, 3), (2, 2)):
        for f in (capture.captures, capture.captures_bruteforce):
            got, st, pos, parts = set(), None, 0, []
            for nb in sizes:
                r, p, st = f(dec[pos * B:(pos + nb) * B], types, thresh, st)
                assert_layout(_shifted(r, -pos * B), p, dec[pos * B:(pos + nb) * B])
                got |= sample_set(r, p)
                parts.append(r)
                pos += nb
            assert got == whole, sizes
            cut = sizes[0] * B
            # crafted_dec puts a trigger at B - 1 and one at 2 B - W / 2: both cuts fall inside a run
            a, b = parts[0][-1], parts[1][0]
            assert int(a["start_sample"] + a["n_samples"]) == cut and a["flags"] & capture.RUN_OPEN
            assert b["start_sample"] == cut and b["flags"] & capture.RUN_CONTINUES
            joined = one[(one["start_sample"] <= cut - 1) & (one["start_sample"] + one["n_samples"] > cut)]
            assert len(joined) == 1 and joined[0]["n_samples"] == a["n_samples"] + b["n_samples"]
            assert (parts[0][:-1]["flags"] == 0).all() and not (parts[1][1:]["flags"] & capture.RUN_CONTINUES).any()
    # a window that ends exactly at a cut: the run is open, and nothing continues behind it
    dec2 = np.zeros((2 * B, 2), dtype=np.int16)
    dec2[B - W] = (3000, 0)
    r0, _, st = capture.captures(dec2[:B], types, 500)
    r1, _, _ = capture.captures(dec2[B:], types, 500, st)
    assert len(r0) == 1 and r0[0]["flags"] == capture.RUN_OPEN and r0[0]["n_samples"] == W and len(r1) == 0
    # ... and a fresh trigger right behind it continues it: uncut, the two are one run
    dec2[B] = (3000, 0)
    r1, _, _ = capture.captures(dec2[B:], types, 500, st)
    b1, _, _ = capture.captures_bruteforce(dec2[B:], types, 500, capture.captures_bruteforce(dec2[:B], types, 500)[2])
    assert np.array_equal(r1, b1) and r1[0]["flags"] == capture.RUN_CONTINUES and r1[0]["start_sample"] == B


@pytest.mark.parametrize("thresh", [500, 0, 60])
def test_captured_samples_are_the_levels_triggered(thresh):
    for types in (0x2F, 0x01, 0x02):
        W = max(levels.windows(types))
        dec, _ = crafted_dec(W, types + 1000)
        runs, _, _ = capture.captures(dec, types, thresh)
        lv, _ = levels.levels(dec, types, thresh)
        per_block = np.zeros(len(lv), dtype=np.int64)
        for r in runs:
            n = np.arange(int(r["start_sample"]), int(r["start_sample"] + r["n_samples"]))
            per_block += np.bincount(n // B, minlength=len(lv))
            assert r["thresh"] == lv["thresh"][int(r["start_sample"]) // B]
        assert per_block.tolist() == lv["triggered"].tolist()


def test_table_and_prefix():
    W = 694
    a = capture.captures(crafted_dec(W, 1)[0], 0x2F, 500)
    z = capture.captures(np.zeros((3 * B, 2), dtype=np.int16), 0x2F, 500)
    b = capture.captures(crafted_dec(W, 2)[0], 0x2F, 500)
    runs, pool = capture.table([z[:2], a[:2], b[:2]])
    assert runs["stream"].tolist() == [1] * len(a[0]) + [2] * len(b[0]) and len(pool) == len(a[1]) + len(b[1])
    assert np.array_equal(runs["pool_offset"], np.concatenate([[0], np.cumsum(runs["n_samples"])[:-1]]).astype(np.uint64))
    r, p, ov = capture.prefix(runs, pool, len(runs), len(pool))
    assert not ov and len(r) == len(runs) and len(p) == len(pool)
    r, p, ov = capture.prefix(runs, pool, len(runs) - 1, len(pool))
    assert ov and len(r) == len(runs) - 1 and len(p) == len(pool) - int(runs[-1]["n_samples"])
    r, p, ov = capture.prefix(runs, pool, len(runs), len(pool) - 1)
    assert ov and len(r) == len(runs) - 1 and len(p) == len(pool) - int(runs[-1]["n_samples"])
    assert capture.idx_line(3, runs[0]) == "3 1 %d %d 500 0" % (runs[0]["start_sample"], runs[0]["n_samples"])


def test_the_struct_and_the_exports(tmp_path):
    assert capture.RUN_DTYPE.itemsize == 32 and api.RUN_DTYPE is capture.RUN_DTYPE
    assert [capture.RUN_DTYPE.fields[f][1] for f in capture.RUN_DTYPE.names] == [0, 4, 8, 16, 20, 24]
    src = tmp_path / "run.c"
    src.write_text('#include <stddef.h>\n#include "tfrec_amd.h"\n'
                   "_Static_assert(sizeof(tfrec_amd_run) == 32, \"size\");\n"
                   "_Static_assert(offsetof(tfrec_amd_run, stream) == 0 && offsetof(tfrec_amd_run, flags) == 4 && "
                   "offsetof(tfrec_amd_run, start_sample) == 8 && offsetof(tfrec_amd_run, n_samples) == 16 && "
                   "offsetof(tfrec_amd_run, thresh) == 20 && offsetof(tfrec_amd_run, pool_offset) == 24, \"layout\");\n"
                   "_Static_assert(TFREC_AMD_RUN_CONTINUES == 1 && TFREC_AMD_RUN_OPEN == 2, \"flags\");\n")
    subprocess.check_call(["cc", "-std=c11", "-fsyntax-only", "-I", os.path.join(parity.ROOT, "include"), str(src)])
    assert capture.RUN_CONTINUES == 1 and capture.RUN_OPEN == 2
    assert "tfrec_amd_enable_capture" in api.EXPORTS and "tfrec_amd_read_captures" in api.EXPORTS
    L = api.load_library()
    for sym in ("tfrec_amd_enable_capture", "tfrec_amd_read_captures"):
        getattr(L, sym)
    # no GPU is needed to be refused
    assert L.tfrec_amd_enable_capture(None, 16, 1024) == api.E_INVAL
    n, p = C.c_uint32(7), C.c_uint64(7)
    assert L.tfrec_amd_read_captures(None, None, 0, C.byref(n), None, 0, C.byref(p)) == api.E_INVAL and n.value == 7


# ---- tfrec_gpu -S: what is decided before a device is opened
def test_cli_capture_usage_errors(tmp_path):
    parity.build_cli()
    f = str(tmp_path / "missing.iq")
    pre = str(tmp_path / "cap")

    out = parity.run_cli(["-S", pre, "-X", f])
    assert out.returncode == 1 and "-S records" in out.stderr
    out = parity.run_cli(["-S", "", "-L", f])
    assert out.returncode == 1 and "bad -S" in out.stderr
    out = parity.run_cli(["-S"])
    assert out.returncode == 1
    for args in (["-S", pre, "-L", f], ["-S", pre, "-s", "50", "-L", f]):  # accepted: the file is looked for
        out = parity.run_cli(args)
        assert out.returncode == 2 and "missing.iq" in out.stderr, args
    assert not os.path.exists(pre + ".idx")


def test_cli_capture_index_that_cannot_be_written(tmp_path):
    """<prefix>.idx is opened before a device is: a prefix in a directory that does not exist ends the run there, with the path on
    stderr."""
    cli = parity.build_cli()
    f = tmp_path / "one.iq"
    f.write_bytes(bytes([128]) * api.BLOCK_BYTES)
    pre = str(tmp_path / "nowhere" / "cap")
    out = subprocess.run([cli, "-S", pre, "-L", str(f)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 2 and out.stderr.startswith(pre + ".idx: "), out.stderr
    assert out.stdout == ""
