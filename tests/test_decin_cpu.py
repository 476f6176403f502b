"""Channel-rate input without a GPU (tfrec_amd_create_decimated, tfrec_amd_enable_capture_pre, tfrec_amd_submit_runs, tfrec_gpu -R;
DESIGN.md 6n): the restatement tfrec_amd/decin.py against capture.py and levels.py -- a capture, expanded, triggers and levels as
the samples it was taken from --, its cutter, its rule list, the exports, and what tfrec_gpu -R decides before it opens a device.

Everything is an exact integer; nothing here has a tolerance."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import parity
from tfrec_amd import api, capture, decin, levels
from meter_rows import crafted_dec

B = levels.BLOCK_DEC
TYPE_SETS = (0x2F, 0x01, 0x02, 0x24)


def captured(dec, types, thresh, sizes=None):
    """One stream's capture over the submits `sizes` (blocks; default: one submit) with absolute start_sample, the pool offsets
    into one pool, and the pre samples -> (runs, pool, pre)."""
    sizes = sizes or (len(dec) // B,)
    tabs, pools, pres, st, pos, off = [], [], [], None, 0, 0
    prev = np.zeros((1, 2), dtype=np.int16)
    for nb in sizes:
        part = dec[pos * B:(pos + nb) * B]
        runs, pool, st = capture.captures(part, types, thresh, st)
        pres.append(decin.pre_samples(part[None], runs, prev, base=pos * B))
        runs = runs.copy()
        runs["pool_offset"] += off
        off += len(pool)
        tabs.append(runs)
        pools.append(pool)
        prev = part[None, -1]
        pos += nb
    return np.concatenate(tabs), np.concatenate(pools), np.concatenate(pres)


@pytest.mark.parametrize("thresh", [500, 0])
@pytest.mark.parametrize("types", TYPE_SETS, ids=["%02x" % t for t in TYPE_SETS])
def test_an_expanded_capture_holds_the_captured_and_the_pre_positions_and_triggers_alike(types, thresh):
    W = max(levels.windows(types))
    dec, loud = crafted_dec(W, types + 7, n_blocks=4)
    nb = len(dec) // B
    runs, pool, pre = captured(dec, types, thresh)
    assert decin.check(runs, len(pool), nb, 1) is None
    rows, override = decin.expand(runs, pool, pre, nb, 1)
    keep = np.zeros(len(dec), dtype=bool)
    for r in runs:
        a, n = int(r["start_sample"]), int(r["n_samples"])
        keep[max(a - 1, 0):a + n] = True
    assert np.array_equal(rows[0][keep], dec[keep]) and not rows[0][~keep].any() and 0 < keep.sum() < len(dec)
    assert override == {}  # crafted_dec's first trigger lies at 200
    # exactly one sample between two runs: the triggers W + 1 apart
    gaps = runs["start_sample"][1:] - (runs["start_sample"][:-1] + runs["n_samples"][:-1])
    assert 1 in gaps.tolist() and (gaps >= 1).all()
    k = int(np.flatnonzero(gaps == 1)[0]) + 1
    assert np.array_equal(pre[k], dec[int(runs[k]["start_sample"]) - 1])
    # the capture of the expanded row is the capture, and its levels' trigger bookkeeping the original's
    again, pool2, _ = capture.captures(rows[0], types, thresh)
    assert np.array_equal(again, runs) and np.array_equal(pool2, pool)
    lv, _ = levels.levels(dec, types, thresh)
    lx, _ = levels.levels(rows[0], types, thresh)
    for f in ("triggered", "n_over", "thresh", "triggered_avg"):
        assert lv[f].tolist() == lx[f].tolist(), f
    assert lv["triggered"].sum() == len(pool)


def test_a_run_at_the_first_sample_brings_its_predecessor():
    dec = np.zeros((B, 2), dtype=np.int16)
    dec[0] = (3000, 0)
    runs, pool, _ = capture.captures(dec, 0x2F, 500)
    pre = decin.pre_samples(dec[None], runs, np.array([[11, -12]], dtype=np.int16))
    assert pre.tolist() == [[11, -12]] and decin.pre_samples(dec[None], runs).tolist() == [[0, 0]]
    rows, override = decin.expand(runs, pool, pre, 1, 2)
    assert override == {0: (11, -12)} and np.array_equal(rows[0], dec) and not rows[1].any()


@pytest.mark.parametrize("thresh", [500, 0])
def test_rebase_cuts_like_the_recorder_and_joins_what_touches(thresh):
    types = 0x2F
    W = max(levels.windows(types))
    dec, _ = crafted_dec(W, 77, n_blocks=4)
    whole = decin.expand(*captured(dec, types, thresh), 4, 1)[0][0]
    for recorded in ((4,), (1, 3), (2, 2)):
        runs, pool, pre = captured(dec, types, thresh, recorded)
        for sizes in ((4,), (1, 3), (2, 2)):
            pos, parts = 0, []
            for nb in sizes:
                t, p, q = decin.rebase(runs, pool, pre, pos * B, nb * B)
                assert decin.check(t, len(p), nb, 1) is None, (recorded, sizes)
                rows, override = decin.expand(t, p, q, nb, 1)
                parts.append(rows[0])
                # crafted_dec puts a trigger at B - 1 and one at 2 B - W / 2: both cuts fall inside a run, whose second part
                # starts at the submit's first sample with the first part's last pair ahead of it
                if pos:
                    assert t[0]["start_sample"] == 0 and override == {0: tuple(int(v) for v in dec[pos * B - 1])}
                pos += nb
            assert np.array_equal(np.concatenate(parts), whole), (recorded, sizes)
    # recorded in two submits, the touching halves are one run again
    runs, pool, pre = captured(dec, types, thresh, (2, 2))
    one = captured(dec, types, thresh)
    t, p, q = decin.rebase(runs, pool, pre, 0, 4 * B)
    assert len(t) == len(one[0]) == len(runs) - 1
    for f in ("start_sample", "n_samples", "pool_offset"):
        assert np.array_equal(t[f], one[0][f])
    assert np.array_equal(p, one[1]) and np.array_equal(q, one[2])


def test_check_refuses_each_rule_violated_by_one():
    M = 2 * B
    good = np.zeros(3, dtype=capture.RUN_DTYPE)
    good["stream"] = [0, 0, 1]
    good["start_sample"] = [0, 11, M - 5]
    good["n_samples"] = [10, 20, 5]  # a gap of one sample; a run that ends with the submit
    good["pool_offset"] = [0, 10, 30]
    good["flags"], good["thresh"] = 3, -7  # ignored
    ok = dict(n_pairs=35, n_blocks=2, n_streams=2, max_runs=3, max_samples=35)
    assert decin.check(good, **ok) is None
    assert decin.check(good[:0], **dict(ok, n_pairs=0)) is None

    def bad(word, field=None, index=None, value=None, **kw):
        r = good.copy()
        if field:
            r[field][index] = value
        assert decin.check(r, **dict(ok, **kw)) == word, word

    bad("stream", "stream", 2, 2)
    bad("start", "start_sample", 0, -1)
    bad("start", "start_sample", 2, M)
    bad("length", "n_samples", 2, 6)
    bad("length", "n_samples", 0, 0)
    bad("order", "stream", 0, 1)  # (1, 0, 1)
    bad("gap", "start_sample", 1, 10)
    bad("pool_offset", "pool_offset", 1, 11)
    bad("n_pairs", n_pairs=36, max_samples=36)
    bad("limits", max_runs=2)
    bad("limits", max_samples=34)
    bad("mapped", mapped=True)
    swapped = good[[1, 0, 2]].copy()
    swapped["pool_offset"] = [0, 20, 30]
    assert decin.check(swapped, **ok) == "order"


def test_clamp_and_mask():
    x = np.array([-32768, -32767, 32767, 0, -1], dtype=np.int16)
    assert decin.clamp(x).tolist() == [-32767, -32767, 32767, 0, -1] and decin.clamp(x).dtype == np.int16
    d = np.array([[300, -200], [300, -201], [-32767, -32767]], dtype=np.int16)
    assert decin.mask(d, 500).tolist() == [False, True, True] and decin.mask(d.reshape(-1), 500).tolist() == [False, True, True]


def test_the_exports(tmp_path):
    new = ("tfrec_amd_create_decimated", "tfrec_amd_enable_capture_pre", "tfrec_amd_read_capture_pre", "tfrec_amd_enable_runs_input",
           "tfrec_amd_submit_runs")
    L = api.load_library()
    for sym in new:
        assert sym in api.EXPORTS
        getattr(L, sym)
    src = tmp_path / "decin.c"
    src.write_text('#include "tfrec_amd.h"\n_Static_assert(TFREC_AMD_FMT_DEC16 == 16, "format");\n'
                   "int (*a)(const tfrec_amd_config *, tfrec_amd_ctx **) = tfrec_amd_create_decimated;\n"
                   "int (*b)(tfrec_amd_ctx *) = tfrec_amd_enable_capture_pre;\n"
                   "int (*c)(tfrec_amd_ctx *, int16_t *, size_t, uint32_t *) = tfrec_amd_read_capture_pre;\n"
                   "int (*d)(tfrec_amd_ctx *, uint32_t, uint64_t) = tfrec_amd_enable_runs_input;\n"
                   "int (*e)(tfrec_amd_ctx *, const tfrec_amd_run *, uint32_t, const int16_t *, uint64_t, const int16_t *, int) = "
                   "tfrec_amd_submit_runs;\n")
    subprocess.check_call(["cc", "-std=c11", "-fsyntax-only", "-I", os.path.join(parity.ROOT, "include"), str(src)])
    assert decin.FMT_DEC16 == 16 and decin.BLOCK_BYTES == 32768
    # no GPU is needed to be refused
    n = C.c_uint32(7)
    out = C.c_void_p(1)
    assert L.tfrec_amd_create_decimated(None, C.byref(out)) == api.E_INVAL
    assert L.tfrec_amd_enable_capture_pre(None) == api.E_INVAL
    assert L.tfrec_amd_read_capture_pre(None, None, 0, C.byref(n)) == api.E_INVAL and n.value == 7
    assert L.tfrec_amd_enable_runs_input(None, 1, 1) == api.E_INVAL
    assert L.tfrec_amd_submit_runs(None, None, 0, None, 0, None, 1) == api.E_INVAL
    cfg = api.Config(1, 0x2F, 500, 0, 0, 1, 16, api.F_INPUT_10X)
    assert L.tfrec_amd_create_decimated(C.byref(cfg), C.byref(out)) == api.E_INVAL and not out.value


# ---- tfrec_gpu -R: what is decided before a device is opened
def write_capture(pre, lines, pairs, pres):
    """A capture of one file: its .idx lines, `pairs` pairs of .cs16 and `pres` pairs of .pre."""
    open(pre + ".idx", "w").write("".join(ln + "\n" for ln in lines))
    np.arange(2 * pairs, dtype="<i2").tofile(pre + ".0.cs16")
    np.arange(2 * pres, dtype="<i2").tofile(pre + ".0.pre")


def test_cli_replay_usage_errors(tmp_path):
    parity.build_cli()
    f = str(tmp_path / "some.iq")
    pre = str(tmp_path / "cap")
    write_capture(pre, ["0 0 100 10 500 0", "0 0 400 20 500 0"], 30, 2)

    for extra in (["-L", f], ["-x"], ["-r", "2048000"], ["-F", "s16"], ["-f", "868300"], ["-c", "868250"], ["-s", "50"], ["-A"],
                  ["-P", "64"], ["-z"], ["-S", str(tmp_path / "other")], ["-X", f], ["-p", "t=500"]):
        out = parity.run_cli(["-R", pre] + extra)
        assert out.returncode == 2 and "-R replays" in out.stderr and out.stdout == "", extra
    out = parity.run_cli(["-R", ""])
    assert out.returncode == 2 and "bad -R" in out.stderr
    assert parity.run_cli(["-R"]).returncode == 1  # (getopt's: the argument is missing)
    assert not os.path.exists(str(tmp_path / "other") + ".idx")


def test_cli_replay_of_a_missing_or_inconsistent_capture(tmp_path):
    cli = parity.build_cli()
    pre = str(tmp_path / "cap")
    good = ["0 0 100 10 500 0", "0 0 400 20 500 2", "0 0 420 5 500 1"]  # (the last two touch: a run cut by a submit)

    def run():
        out = subprocess.run([cli, "-T", "2f", "-t", "500", "-R", pre], capture_output=True, text=True, timeout=120)
        assert out.returncode == 2 and out.stdout == "" and "tfrec_amd_create" not in out.stderr, out.stderr
        return out.stderr

    assert run().startswith(pre + ".idx: ")  # missing
    write_capture(pre, good, 34, 3)
    assert run().startswith(pre + ".0.cs16: 34 pairs") and "ask for 35" in run()
    write_capture(pre, good, 35, 2)
    assert run().startswith(pre + ".0.pre: 2 pairs")
    os.remove(pre + ".0.pre")
    assert run().startswith(pre + ".0.pre: ")
    for lines, where, word in ((good[:1] + ["0 0 109 20 500 0"], 2, "overlaps"), ([good[1], good[0]], 2, "out of order"),
                               (good + ["0 0 500 0 500 0"], 4, "empty run"), (good + ["0 0 -5 3 500 0"], 4, "negative"),
                               (good + ["0 0 500 3 500"], 4, "want '<file index>"), (good + ["0 0 500 3 500 0 7"], 4, "want '<file index>"),
                               (["zero"], 1, "want '<file index>")):
        write_capture(pre, lines, 64, 8)
        err = run()
        assert err.startswith("%s.idx:%d: " % (pre, where)) and word in err, (lines, err)
