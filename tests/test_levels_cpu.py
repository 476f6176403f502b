"""The level meter and the scan mode without a GPU (TFREC_AMD_F_LEVELS, tfrec_gpu -s): the restatement
tfrec_amd/levels.py against a per-sample simulation of the reference's loops and against the oracle's auto threshold, the carry
of its state, and what tfrec_gpu decides before it opens a device.

Everything is an exact integer; nothing here has a tolerance."""
import re

import numpy as np
import pytest

import parity
from meter_rows import SUBSETS, crafted_dec
from oracle import oracle as O
from tfrec_amd import api, levels, synth

B = levels.BLOCK_DEC


def test_windows_are_the_reference_values():
    assert levels.windows(0x2F) == [400, 356, 640, 694, 512]  # tfa1.cpp:148; tfa2.cpp:355 at 17240, 9600, 8842 baud; whb.cpp:641
    assert levels.windows(0x20) == [512] and levels.windows(0x05) == [400, 640]
    for bad in (0, 0x10, 0x40, 0x3F):
        with pytest.raises(ValueError):
            levels.windows(bad)
    assert levels.LEVEL_DTYPE.itemsize == 32 and api.LEVEL_DTYPE is levels.LEVEL_DTYPE
    assert api.F_LEVELS == 32 and "tfrec_amd_read_levels" in api.EXPORTS


@pytest.mark.parametrize("types", SUBSETS, ids=["%02x" % t for t in SUBSETS])
def test_levels_equal_the_per_sample_simulation(types):
    W = max(levels.windows(types))
    dec, loud = crafted_dec(W, types)
    for thresh in (500, 0, 60):
        got, _ = levels.levels(dec, types, thresh)
        want, _ = levels.levels_bruteforce(dec, types, thresh)
        assert np.array_equal(got, want), (types, thresh)
    # the input holds what it is meant to hold (fixed threshold 500: only the loud samples trigger)
    got, st = levels.levels(dec, types, 500)
    assert got["n_over"].sum() == len(loud) and got["thresh"].tolist() == [500] * 3 and got["pwr_max"].tolist() == [6000] * 3
    in_block0 = [p for p in loud if p < B]
    # block 0: the single at its last sample counts once; the pairs at distance d cover min(d, W) + W samples
    assert got["triggered"][0] == 1 + sum(min(d, W) + W for d in (W - 1, W, W + 1, W + 2)) and len(in_block0) == 9
    # block 1: the rest of that window (W - 1 samples) and the half of the straddling one; block 2 begins with its other half
    assert got["triggered"][1] == (W - 1) + W // 2
    assert got["triggered"][2] >= W - W // 2
    assert st["last_trig"] == -1  # the last sample of the input


def oracle_streams(n_blocks):
    """u8 streams at 1.536 MS/s for the auto threshold: near-silence, loud noise, the synthetic sensor traffic, and short loud
    bursts that come more and more often (the triggered count passes through the range in which fm_demod.cpp:64-68 decides)."""
    rng = np.random.default_rng(2024)
    n = n_blocks * api.BLOCK_BYTES
    quiet = rng.integers(126, 131, n, dtype=np.uint8)
    loud = rng.integers(0, 256, n, dtype=np.uint8)
    traffic = synth.gen_stream(11, 3, n_blocks)
    bursts = rng.integers(126, 131, n, dtype=np.uint8)
    pos, gap = 5000, 60000
    while pos + 400 < n // 2:
        bursts[2 * pos:2 * pos + 400] = rng.integers(0, 256, 400, dtype=np.uint8)
        pos += gap
        gap = max(1500, gap * 9 // 10)
    return {"quiet": quiet, "loud": loud, "traffic": traffic, "bursts": bursts}


def test_thresholds_equal_the_oracles_block_by_block():
    """fsk_demod::process in auto mode, fed one block at a time: the threshold after block b is the restatement's thresh of
    block b + 1.  The restatement derives it from its own `triggered`, so this pins `triggered` to the reference wherever the
    recurrence is sensitive to it."""
    n_blocks = 24
    moves = {}
    for name, iq in oracle_streams(n_blocks).items():
        o = O.Oracle(0x2F, 0, 0, keep_dec=True)
        after = []
        for b in range(n_blocks):
            o.process(iq[b * api.BLOCK_BYTES:(b + 1) * api.BLOCK_BYTES])
            after.append(o.thresh())
        dec = o.dec()
        assert len(dec) == 2 * n_blocks * B
        moves[name] = after
        rec, st = levels.levels(dec, 0x2F, 0)
        assert rec["thresh"][0] == 500
        assert rec["thresh"][1:].tolist() == after[:-1], name
        assert st["thresh"] == after[-1] == levels.next_thresh(rec[-1], True, n_blocks), name
        # ... and a fixed threshold stays, while triggered_avg still advances (the reference computes it unconditionally)
        fixed, _ = levels.levels(dec, 0x2F, 500)
        assert set(fixed["thresh"].tolist()) == {500}
        if name == "loud":
            assert fixed["triggered_avg"][-1] > 4000
    # the precondition, on the oracle alone: a threshold that rises, one that falls, and one that does both or neither
    assert any(a[-1] > 500 for a in moves.values()) and any(a[-1] < 500 for a in moves.values()), moves
    assert max(moves["loud"]) == 500 + 2 * (n_blocks // 4) and min(moves["quiet"]) == 500 - 2 * (n_blocks // 4)
    assert len({tuple(a) for a in moves.values()}) >= 3, moves


@pytest.mark.parametrize("thresh", [500, 0])
def test_cutting_a_stream_into_calls_changes_nothing(thresh):
    o = O.Oracle(0x2F, thresh, 0, keep_dec=True)
    o.process(oracle_streams(9)["bursts"])
    dec = o.dec().reshape(-1, 2)
    one, st_one = levels.levels(dec, 0x2F, thresh)
    assert one["triggered"].sum() > 0
    for sizes in ((1, 8), (4, 1, 4), (1,) * 9):
        parts, st, pos = [], None, 0
        for nb in sizes:
            r, st = levels.levels(dec[pos * B:(pos + nb) * B], 0x2F, thresh, st)
            parts.append(r)
            pos += nb
        assert np.array_equal(np.concatenate(parts), one) and st == st_one, sizes
    # the simulation carries its own kind of state the same way
    a, sa = levels.levels_bruteforce(dec[:2 * B], 0x2F, thresh)
    b, _ = levels.levels_bruteforce(dec[2 * B:4 * B], 0x2F, thresh, sa)
    assert np.array_equal(np.concatenate([a, b]), one[:4])


# ---- tfrec_gpu -s: what is decided before a device is opened
@pytest.fixture(scope="module")
def cli():
    return parity.build_cli()


def test_cli_scan_usage_errors(cli, tmp_path):
    f = str(tmp_path / "missing.iq")
    for extra in (["-n", "2"], ["-p", "t=100"], ["-f", "868300"], ["-e", "true"], ["-E", "cat"], ["-X", f], ["-L", f],
                  ["-d", "0,1"]):
        out = parity.run_cli(["-s", "50", "-L", f] + extra)
        assert out.returncode == 1 and "-s scans one -L file" in out.stderr, extra
    for bad in ("0", "-5", "x", "", "2.5"):
        out = parity.run_cli(["-s", bad, "-L", f])
        assert out.returncode == 1 and "bad -s" in out.stderr, bad
    # 1.536 MS/s: 1153 channels at 1 kHz; -x: 14977 at 1 kHz are too many, 4 kHz gives 3745
    out = parity.run_cli(["-s", "1", "-x", "-L", f])
    assert out.returncode == 1 and "14977 channels" in out.stderr and "at most 4096" in out.stderr
    out = parity.run_cli(["-s", "1", "-r", "9600000", "-L", f])
    assert out.returncode == 1 and "at most 4096" in out.stderr
    for args in (["-s", "1"], ["-s", "4", "-x"], ["-s", "50", "-r", "2400000", "-F", "s16"]):
        out = parity.run_cli(args + ["-L", f])  # accepted: the file is looked for
        assert out.returncode == 2 and "missing.iq" in out.stderr, args
    out = parity.run_cli(["-s", "50"])
    assert out.returncode == 1 and "need -L" in out.stderr


@pytest.mark.parametrize("args,fs_in,place", [
    ([], 1536000, "in the front end"),
    (["-x"], 15360000, "ahead of the 10:1 stage"),
    (["-r", "2400000"], 2400000, None),
])
def test_cli_scan_channel_list(cli, tmp_path, args, fs_in, place):
    """-s 50: the channels c + 50 k with |50000 k| <= fs_in / 2 - 192000, ascending, each with the tune -f would give it -- at
    2.4 MS/s behind the resampler within +-767 kHz and ahead of it beyond (listed before a device is opened; the run itself
    then needs one)."""
    f = tmp_path / "empty.iq"
    f.write_bytes(b"")
    c = 868300
    out = parity.run_cli(args + ["-s", "50", "-c", str(c), "-L", str(f)])
    assert out.returncode in (0, 2)
    got = re.findall(r"^scan channel (\d+) kHz: tune (-?\d+) Hz (.*)$", out.stderr, re.M)
    want = levels.scan_channels(c, 50, fs_in)
    half = (fs_in // 2 - 192000) // 1000
    assert want == [k for k in range(c - 50 * 400, c + 50 * 400 + 1, 50) if abs(k - c) <= half] and want[len(want) // 2] == c
    assert len(want) == {1536000: 23, 15360000: 299, 2400000: 41}[fs_in]
    assert [int(k) for k, _, _ in got] == want
    assert [int(hz) for _, hz, _ in got] == [(k - c) * 1000 for k in want]
    assert "scan: %d channels, input rate %d S/s" % (len(want), fs_in) in out.stderr
    for k, hz, where in got:
        hz = int(hz)
        if hz == 0:
            assert where == "(none)"
        elif place:
            assert where == place
        else:
            assert where == ("ahead of the resampler" if abs(hz) >= 768000 else "behind the resampler")
    if not place:
        assert sum(1 for _, hz, _ in got if abs(int(hz)) >= 768000) == 10
