"""The envelope clock on the GPU (tfrec_amd_enable_burst_keying, tfrec_amd_read_burst_keyings, tfrec_gpu -a), bit for bit.

Every record is compared, byte for byte, with clock.keyings run on the context's OWN decimated samples and run table.  Channel-rate
contexts take hand-made samples, so the segment edges, the normalising shift's steps, the split's corner and the tile edges of the
matrix product (H = 32 rows a workgroup) are placed exactly.  Everything is an exact integer; nothing here has a tolerance."""
import functools

import numpy as np
import pytest

import parity
import recorder as R
from recorder import B, CONT, OPEN, TABLE_FIELDS, W, cli_lines, hand_receiver, raises, read_clock, read_envelope, same_chains, same_records, zeros
from recorder_rows import CTX_TYPES, golden_iq, quiet, scene
from tfrec_amd import api, burst, capture, clock, decin

pytestmark = pytest.mark.gpu
SEG = clock.KEY_SEG
H = 32  # keying.h: kKeyTile


def keying_receiver(n, nb, **kw):
    r = hand_receiver(n, nb, (), levels=False, **kw)
    r.enable_burst_keying()
    return r


def read_keying(r, nb, base, overflow=False, decs=None):
    """The oldest undrained submit's records against the restatement -> (records, decimated samples, the run table)."""
    decs, runs, _ = R.submit_view(r, nb, decs, levels=None)
    got = r.read_burst_keyings(allow_overflow=overflow)
    assert len(got) == r.keying_total or r.capture_overflow
    same_records(got, clock.keyings(decs, got[list(TABLE_FIELDS)], base=base), "keying")
    return got, decs, runs


def square(n, period, on, seed=0):
    """n pairs, `on` for the first half of every `period` samples and (0, 0) for the second (shorter than the trigger's hold)."""
    z = np.zeros((n, 2), dtype=np.int16)
    z[(np.arange(n) + seed) % period < period // 2] = on
    return z


# ---- hand-made rows: int16 [2, 2 B, 2], four segments a stream.  A tone on [a, b) gives the run [a, b + W - 1)
@functools.lru_cache(maxsize=None)
def hand_rows(kind):
    rows = np.stack([quiet(2, 21), quiet(2, 22)])
    if kind == "edges":
        # stream 0: [0, 2 SEG), from a boundary to a boundary, keyed every 128 samples: segments 0 and 1; then 8190 samples from
        # 2 SEG + 1, the longest run without a segment.  Stream 1: [SEG + 1, 3 SEG), from a sample behind a boundary across the
        # block's end to a boundary: segment 2; then a run open at the last sample
        for s, a, b, period, on in ((0, 0, 2 * SEG - W + 1, 128, (3000, -1000)), (0, 2 * SEG + 1, 4 * SEG - W, 100, (2000, 2000)),
                                    (1, SEG + 1, 3 * SEG - W + 1, 48, (-5000, 300)), (1, 2 * B - 1500, 2 * B, 64, (0, 4000))):
            rows[s, a:b] = square(b - a, period, on)
            rows[s, b - 1] = on  # (the tone's last sample holds the trigger for W - 1 more)
    else:
        # the shift's steps: mx = 2^14 - 1, 2^14, 2^15 and 65534 (sh = 0, 1, 2, 3), keyed every 128 samples; and segments whose
        # samples are all mx: x = 2^14 - 1 throughout -- both planes at 127, the accumulators' worst case -- and 8191 at sh = 3
        for k, on in enumerate(((16383, 0), (-16384, 0), (16384, -16384), (32767, -32767))):
            rows[0, k * SEG:(k + 1) * SEG] = square(SEG, 128, on)
        rows[1, :2 * SEG] = (8191, -8192)
        rows[1, 2 * SEG:] = (32767, 32767)
    rows.setflags(write=False)
    return rows


@functools.lru_cache(maxsize=None)
def hand_uncut(kind):
    with keying_receiver(2, 2) as r:
        r.submit(np.ascontiguousarray(hand_rows(kind)))
        got = read_keying(r, 2, [0, 0])[0]
        assert r.read_burst_keyings().tobytes() == got.tobytes()  # reading pops nothing
        r.drain()
        raises(api.E_STATE, r.read_burst_keyings)  # nothing undrained
    return got


def test_segment_edges_of_hand_made_runs():
    got = hand_uncut("edges")
    seg = {(int(r["stream"]), int(r["start_sample"])): (int(r["n_samples"]), int(r["n_segments"]), int(r["n_silent"])) for r in got}
    assert seg == {(0, 0): (2 * SEG, 2, 0), (0, 2 * SEG + 1): (8190, 0, 0), (1, SEG + 1): (2 * SEG - 1, 1, 0), (1, 2 * B - 1500): (1500, 0, 0)}
    assert got[-1]["flags"] == OPEN and clock.summary(got[1], clock.KEYING) is None
    qhz, q = clock.summary(got[0], clock.KEYING)  # keyed every 128 samples: 3000 Hz, bin 32
    assert abs(qhz - 4 * 3000) <= 375 and q > 2500


def test_the_shifts_steps_and_segments_that_are_all_mx():
    got = hand_uncut("levels")
    assert [(int(r["n_samples"]), int(r["n_segments"])) for r in got] == [(2 * B, 4)] * 2
    assert abs(clock.summary(got[0], clock.KEYING)[0] - 4 * 3000) <= 375  # (stream 1 is DC alone: nothing in the band)


@pytest.mark.parametrize("kind", ["edges", "levels"])
def test_the_same_rows_in_two_submits_queued_before_the_first_read(kind):
    rows = hand_rows(kind)
    with keying_receiver(2, 1) as r:
        for k in range(2):
            r.submit(np.ascontiguousarray(rows[:, k * B:(k + 1) * B]))
        got = []
        for k in range(2):
            part = decin.clamp(rows[:, k * B:(k + 1) * B])
            got.append(read_keying(r, 1, [k * B] * 2, decs=[part[s].reshape(-1) for s in range(2)])[0])
            r.drain()
    assert (got[1]["flags"] & CONT).any()
    key = lambda c: (int(c["stream"]), int(c["start_sample"]))  # noqa: E731
    same_chains("clock", sorted(clock.chains(got), key=key), sorted(clock.chains([hand_uncut(kind)]), key=key), "1 + 1")


# ---- the work list's tiles: streams that never leave their window hold 4 segments each over 2 blocks; the last stream starts late
@pytest.mark.parametrize("n, late, entries", [(8, 1, H - 1), (8, 0, H), (9, 3 * SEG - 5, H + 1), (33, 3 * SEG - 5, 4 * H + 1), (65, 0, 260)])
def test_work_lists_that_end_beside_a_tiles_edge(n, late, entries):
    x = np.stack([square(2 * B, 2 * (8 + s), (3000 + 37 * s, -(s % 5) * 400), seed=s) for s in range(n)])
    x[n - 1, :late] = quiet(2, 5)[:late]
    with keying_receiver(n, 2) as r:
        r.submit(x)
        got = read_keying(r, 2, [0] * n)[0]
        r.drain()
    assert got["stream"].tolist() == list(range(n)) and int(got["n_segments"].sum()) == entries and not got["n_silent"].any()


# ---- beside the other stages, and the other kinds of context
def test_a_golden_scene_with_the_meter_the_envelope_and_the_clock_beside_it_and_none():
    x = golden_iq()
    with api.Receiver(1, 0x2F, 500, 0, max_blocks=4, all_flushes=True, levels=True) as r:
        r.enable_capture(256, 4 * B)
        rec_mem = r.memory()
        r.submit(x)
        plain_runs = r.read_captures()
        plain = r.drain()
    with api.Receiver(1, 0x2F, 500, 0, max_blocks=4, all_flushes=True, levels=True) as r:
        r.enable_capture(256, 4 * B)
        assert r.memory() == rec_mem  # a recorder without the call holds what it held
        r.enable_burst_keying()
        r.enable_burst_clock()
        r.enable_burst_meter()
        r.enable_burst_envelope()
        r.submit(x)
        got, decs, runs = read_keying(r, 4, [0])
        read_clock(r, 4, [0])
        read_envelope(r, 4, zeros(1), [0])
        bursts = r.read_bursts()
        tab = r.read_captures()
        ev = r.drain()
    assert bursts.tobytes() == burst.bursts(decs, runs, zeros(1)).tobytes() and len(bursts) == len(got) >= 2
    R.assert_tables(tab, plain_runs)
    R.same_events(ev, plain)
    assert len(ev) >= 1


def test_a_submit_runs_replay_gives_the_recordings_records():
    x = golden_iq()
    with api.Receiver(1, 0x2F, 500, 0, max_blocks=3, all_flushes=True) as r:
        r.enable_capture(256, 4 * B)
        r.enable_capture_pre()
        r.enable_burst_keying()
        tabs, recs, pos = [], [], 0
        for p, nb in zip(parity.cut(x, (1, 3)), (1, 3)):
            r.submit(p)
            tabs.append(r.read_captures(pre=True))
            recs.append(read_keying(r, nb, [pos * B])[0])
            pos += nb
            r.drain()
    off = 0
    for t, pool, _ in tabs:
        t["pool_offset"] += off
        off += len(pool)
    runs, pool, pre = (np.concatenate([t[i] for t in tabs]) for i in range(3))
    with api.Receiver(1, 0x2F, 500, 0, max_blocks=2, all_flushes=True, decimated=True) as r:
        r.enable_runs_input(len(runs) + 2, len(pool) + 1)
        r.enable_capture(256, 1)
        r.enable_burst_keying()
        rep = []
        for k in range(2):
            t, p, q = decin.rebase(runs, pool, pre, 2 * k * B, 2 * B)
            assert r.submit_runs(t, p, q, 2) == 2
            rep.append(read_keying(r, 2, [2 * k * B])[0])
            r.drain()
    a, b = clock.chains(recs), clock.chains(rep)
    assert len(a) == len(b) >= 2
    same_chains("clock", b, a, "the replay")


def test_overflow_delivers_the_prefix():
    whole = hand_uncut("edges")
    with keying_receiver(2, 2, cap=(len(whole) - 1, 1)) as r:
        r.submit(np.ascontiguousarray(hand_rows("edges")))
        raises(api.E_OVERFLOW, r.read_burst_keyings)
        got = r.read_burst_keyings(allow_overflow=True)
        assert r.keying_total == len(whole)
        same_records(got, whole[:-1], "the prefix")
        r.drain()


def test_the_refusals_of_the_enable_call_and_what_a_context_holds():
    n, mb = 3, 2
    x = scene()[:n, :api.BLOCK_BYTES]
    with api.Receiver(n, CTX_TYPES, 500, 0, max_blocks=mb) as r:
        plain = r.memory()
        raises(api.E_INVAL, r.enable_burst_keying)  # no recorder
        raises(api.E_INVAL, r.read_burst_keyings)
        assert r.memory() == plain
        r.enable_capture(64, 1024)
        rec = r.memory()
        r.submit(x)
        raises(api.E_INVAL, r.read_burst_keyings)  # the recorder alone
        submitted = r.memory()
        raises(api.E_STATE, r.enable_burst_keying)  # after the first submit
        assert r.memory() == submitted
        runs_plain = r.read_captures()
        ev_plain = r.drain()
    with api.Receiver(n, CTX_TYPES, 500, 0, max_blocks=mb) as r:
        r.enable_capture(64, 1024)
        r.enable_burst_keying()
        m = r.memory()
        # per set the records; the work list, its length, and the twiddle planes
        assert m["device_bytes"] - rec["device_bytes"] == api.FIFO_DEPTH * 64 * 1056 + 16 * mb * n + 4 + (2 << 20)
        assert m["pinned_host_bytes"] == rec["pinned_host_bytes"]
        raises(api.E_INVAL, r.enable_burst_keying)  # a second call: refused, and nothing changes
        assert r.memory() == m
        r.enable_burst_clock()  # independent of the clock
        raises(api.E_STATE, r.read_burst_keyings)  # nothing undrained
        r.submit(x)
        nr = api.C.c_uint32(0)
        buf = np.full(1056, 0x55, dtype=np.uint8)  # the caller's room too small: E_INVAL, nothing written, the count set
        assert r.L.tfrec_amd_read_burst_keyings(r.h, buf.ctypes.data, 0, api.C.byref(nr)) == api.E_INVAL and (buf == 0x55).all()
        assert nr.value == len(r.read_burst_keyings()) == len(r.read_burst_clocks()) == len(runs_plain[0])
        runs = r.read_captures()
        ev = r.drain()
    R.assert_tables(runs, runs_plain)
    R.same_events(ev, ev_plain)


# ---- tfrec_gpu -a
def test_cli_keying_lines_of_an_ook_burst_cut_into_three_batches_beside_the_clock(tmp_path):
    """A u8 recording of 6 blocks, the carrier at full scale on I, on for 512 and off for 512 input samples (a period of 256 decimated
    samples: 1500 Hz) from block 1 into block 5: -b 2 cuts the burst twice."""
    parity.build_cli()
    n = 6 * api.BLOCK_BYTES
    x = (127 + np.arange(n) * 7919 % 3).astype(np.uint8)
    k = np.arange(4 * (B + 700), 4 * (4 * B + 3000))
    x[2 * k[k % 1024 < 512]] = 228
    dec = parity.fresh_oracle(x, 0x2F, 500, keep_dec=True).dec().reshape(-1, 2)
    recs, st = [], None
    for a, b in ((0, 2), (2, 4), (4, 6)):
        runs, _, st = capture.captures(dec[a * B:b * B], 0x2F, 500, st)
        recs.append(clock.keyings([dec[a * B:b * B]], runs, base=[a * B]))
    assert any(c["flags"] & CONT for c in recs[1]) and any(c["flags"] & CONT for c in recs[2])
    f = str(tmp_path / "ook.iq")
    x.tofile(f)
    want = [clock.line(f, c, clock.KEYING) for c in clock.chains(recs)]
    best = max(want, key=lambda ln: int(ln.split()[4])).split()
    assert int(best[4]) >= 5 and abs(float(best[5]) - 1500.0) <= 93.75
    base = ["-T", "2f", "-t", "500", "-b", "2", "-L", f]
    got = cli_lines(["-a", "-C"] + base, "keying", "clock")
    alone = cli_lines(["-C"] + base, "keying", "clock")
    assert got["keying"] == want and alone["keying"] == [] and got["clock"] == alone["clock"] and got["telegrams"] == alone["telegrams"]
