"""The burst band on the GPU (tfrec_amd_enable_burst_band, tfrec_amd_read_burst_bands, tfrec_gpu -I), bit for bit.

Every record is compared, byte for byte, with band.bands run on the context's OWN decimated samples and run table.  Channel-rate
contexts take hand-made samples, so the segment edges, the normalising shift's steps, the accumulators' extremes and the tile edges
of the matrix product (H = 32 rows a workgroup) are placed exactly.  Everything is an exact integer; nothing here has a tolerance
but the half bin the issue sets for a tone's peak."""
import functools

import numpy as np
import pytest

import parity
import recorder as R
from recorder import B, CONT, OPEN, TABLE_FIELDS, W, cli_lines, hand_receiver, raises, same_chains, same_records
from recorder_rows import golden_iq, quiet
from tfrec_amd import api, band, decin

pytestmark = pytest.mark.gpu
SEG = band.SEG
H = 32  # band.h: kBandTile


def band_receiver(n, nb, **kw):
    r = hand_receiver(n, nb, (), levels=False, **kw)
    r.enable_burst_band()
    return r


def read_band(r, nb, base, decs=None):
    """The oldest undrained submit's records against the restatement."""
    decs, runs, _ = R.submit_view(r, nb, decs, levels=None)
    got = r.read_burst_bands()
    assert len(got) == r.band_total and (len(got) == len(runs) or r.capture_overflow)  # (a pool of one pair cuts the table, not the records)
    same_records(got, band.bands(decs, got[list(TABLE_FIELDS)], base=base), "band")
    return got


def tone(n, j, amp=3000):
    """n pairs of a complex tone at bin j (750 j Hz) whose largest component is amp, clipped to int16."""
    ph = 2 * np.pi * j * np.arange(n) / SEG
    return np.clip(np.rint(amp * np.stack([np.cos(ph), np.sin(ph)], axis=1)), -32768, 32767).astype(np.int16)


# ---- hand-made rows: int16 [streams, blocks * B, 2].  A tone on [a, b) gives the run [a, b + W - 1)
TONES = (40, -40, -128, 127, 160)  # (160: +120 kHz, outside the band)


@functools.lru_cache(maxsize=None)
def hand_rows(kind):
    if kind == "tones":
        rows = np.stack([quiet(1, 30 + s) for s in range(len(TONES))])
        for s, j in enumerate(TONES):
            rows[s, :4 * SEG - W + 1] = tone(4 * SEG - W + 1, j)
    elif kind == "edges":
        # stream 0: [0, 4 SEG), from a boundary to a boundary; then 1022 samples from 5 SEG + 1, the longest run without a segment.
        # Stream 1: from a sample behind a boundary across the block's end to a boundary: 3 segments; then a run open at the submit's end
        rows = np.stack([quiet(2, 21), quiet(2, 22)])
        for s, a, n, j in ((0, 0, 4 * SEG, 17), (0, 5 * SEG + 1, 1022, -60), (1, B - 2 * SEG + 1, 4 * SEG - 1, -3), (1, 2 * B - 1500, 1500 + W - 1, 90)):
            rows[s, a:a + n - W + 1] = tone(n - W + 1, j)
    else:
        # the shift's steps: tones at bin 64, whose components reach +-amp exactly: mx = 8191, 8192, 16384, 32767 and 32768 (of -32768);
        # and segments that are all (8191, -8192) and all (32767, -32768)
        rows = np.stack([quiet(2, 23), quiet(2, 24)])
        for k, amp in enumerate((8191, 8192, 16384, 32767, 32768)):
            rows[0, k * SEG:(k + 1) * SEG] = tone(SEG, 64, amp)
        rows[1, :2 * SEG] = (8191, -8192)
        rows[1, 2 * SEG:4 * SEG] = (32767, -32768)
    rows.setflags(write=False)
    return rows


@functools.lru_cache(maxsize=None)
def hand_uncut(kind):
    rows = hand_rows(kind)
    n, nb = len(rows), rows.shape[1] // B
    with band_receiver(n, nb) as r:
        r.submit(np.ascontiguousarray(rows))
        got = read_band(r, nb, [0] * n)
        assert r.read_burst_bands().tobytes() == got.tobytes()  # reading pops nothing
        r.drain()
        raises(api.E_STATE, r.read_burst_bands)  # nothing undrained
    return got


def test_segment_edges_of_hand_made_runs():
    got = hand_uncut("edges")
    seg = {(int(r["stream"]), int(r["start_sample"])): (int(r["n_samples"]), int(r["n_segments"]), int(r["n_silent"])) for r in got}
    assert seg == {(0, 0): (4 * SEG, 4, 0), (0, 5 * SEG + 1): (1022, 0, 0), (1, B - 2 * SEG + 1): (4 * SEG - 1, 3, 0), (1, 2 * B - 1500): (1500, 2, 0)}
    assert got[-1]["flags"] == OPEN and band.summary(got[1]) is None and band.summary(got[0])[0] == 750 * 17


def test_the_shifts_steps_and_the_accumulators_extremes():
    got = hand_uncut("levels")
    assert [int(r["n_segments"]) for r in got] == [6, 5] and not got["n_silent"].any()  # (the hold's W - 1 quiet samples: one more segment)
    assert band.summary(got[0])[0] == 750 * 64 and band.summary(got[1])[0] == 0  # (stream 1 is DC alone)


def test_tones_read_at_their_bins_with_the_stated_sign():
    got = hand_uncut("tones")
    peak = [band.summary(r)[0] for r in got]
    assert abs(peak[0] - 750 * 40) <= 375 and abs(peak[1] + 750 * 40) <= 375  # half a bin; a tone that advances in phase: positive
    assert peak[2] == 750 * -128 and peak[3] == 750 * 127  # the end bins: no refinement
    assert peak[4] == 750 * 127  # outside the band: only the window's leakage shows, strongest in the nearest bin


@pytest.mark.parametrize("kind", ["edges", "levels"])
def test_the_same_rows_in_two_submits_queued_before_the_first_read(kind):
    rows = hand_rows(kind)
    with band_receiver(2, 1) as r:
        for k in range(2):
            r.submit(np.ascontiguousarray(rows[:, k * B:(k + 1) * B]))
        got = []
        for k in range(2):
            part = decin.clamp(rows[:, k * B:(k + 1) * B])
            got.append(read_band(r, 1, [k * B] * 2, decs=[part[s].reshape(-1) for s in range(2)]))
            r.drain()
    assert (got[1]["flags"] & CONT).any() == (kind == "edges")
    key = lambda c: (int(c["stream"]), int(c["start_sample"]))  # noqa: E731
    same_chains("band", sorted(band.chains(got), key=key), sorted(band.chains([hand_uncut(kind)]), key=key), "1 + 1")


# ---- the work list's tiles: a stream that never leaves its window holds 16 segments a block; the last stream starts late
@pytest.mark.parametrize("n, late, entries", [(2, 1, H - 1), (2, 0, H), (3, 15 * SEG - 5, H + 1), (65, 0, 65 * 16)])
def test_work_lists_that_end_beside_a_tiles_edge(n, late, entries):
    x = np.stack([tone(B, 3 * s - 100, 3000 + 37 * s) for s in range(n)])
    x[n - 1, :late] = quiet(1, 5)[:late]
    with band_receiver(n, 1) as r:
        r.submit(x)
        got = read_band(r, 1, [0] * n)
        r.drain()
    assert got["stream"].tolist() == list(range(n)) and int(got["n_segments"].sum()) == entries and not got["n_silent"].any()


# ---- beside the other stages, a context without the call, the refusals, and tfrec_gpu -I
def test_the_golden_scene_beside_the_other_stages_the_refusals_and_the_cli(tmp_path):
    x = golden_iq()
    with api.Receiver(1, 0x2F, 500, 0, max_blocks=4, all_flushes=True, levels=True) as r:
        plain_mem = r.memory()
        raises(api.E_INVAL, r.enable_burst_band)  # no recorder
        raises(api.E_INVAL, r.read_burst_bands)
        assert r.memory() == plain_mem
        r.enable_capture(256, 4 * B)
        rec_mem = r.memory()
        r.submit(x)
        raises(api.E_STATE, r.enable_burst_band)  # after the first submit
        raises(api.E_INVAL, r.read_burst_bands)  # the recorder alone
        plain_runs = r.read_captures()
        plain = r.drain()
    with api.Receiver(1, 0x2F, 500, 0, max_blocks=4, all_flushes=True, levels=True) as r:
        r.enable_capture(256, 4 * B)
        assert r.memory() == rec_mem  # a recorder without the call holds what it held
        r.enable_burst_band()
        m = r.memory()
        # per set the records; the work list, its length, and B's planes
        assert m["device_bytes"] - rec_mem["device_bytes"] == api.FIFO_DEPTH * 256 * 2080 + 128 * 4 * 1 + 4 + (1 << 20)
        assert m["pinned_host_bytes"] == rec_mem["pinned_host_bytes"]
        raises(api.E_INVAL, r.enable_burst_band)  # a second call: refused, and nothing changes
        assert r.memory() == m
        r.enable_burst_keying()
        r.enable_burst_clock()
        r.enable_burst_meter()
        r.submit(x)
        got = read_band(r, 4, [0])
        R.read_clock(r, 4, [0])
        assert len(r.read_burst_keyings()) == len(r.read_bursts()) == len(got) >= 2
        tab = r.read_captures()
        ev = r.drain()
    R.assert_tables(tab, plain_runs)
    R.same_events(ev, plain)
    assert len(ev) >= 1
    parity.build_cli()
    f = str(tmp_path / "tfa_2.iq")
    x[0].tofile(f)
    base = ["-T", "2f", "-t", "500", "-L", f]
    lines, alone = cli_lines(["-I", "-C"] + base, "band", "clock"), cli_lines(["-C"] + base, "band", "clock")
    assert lines["band"] == [band.line(f, c) for c in band.chains([got])] and alone["band"] == []
    assert lines["clock"] == alone["clock"] and lines["telegrams"] == alone["telegrams"]
