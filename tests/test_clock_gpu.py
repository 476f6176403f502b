"""The burst clock on the GPU (tfrec_amd_enable_burst_clock, tfrec_amd_read_burst_clocks, tfrec_gpu -C), bit for bit.

The records are compared, byte for byte, with the restatement tfrec_amd/clock.py run on the context's OWN decimated samples
(tfrec_amd_read_decimated) and its own run table, so the front end and the recorder ahead of the clock are whatever the context
runs (recorder.read_clock).  Channel-rate contexts (tfrec_amd_create_decimated) take hand-made decimated samples: the layouts the
kernels can get wrong are placed exactly.  Everything is an exact integer; nothing here has a tolerance."""
import functools
import re

import numpy as np
import pytest

import parity
import recorder as R
from recorder import B, CONT, OPEN, W, cli_lines, hand_receiver, raises, read_clock, read_envelope, same_chains, same_records, zeros
from recorder_rows import CTX_TYPES, N, NB, SEG, golden_iq, keyed, mx_rows, quiet, scene, silent_rows
from tfrec_amd import api, burst, capture, clock, decin

pytestmark = pytest.mark.gpu
CLOCK = ("clock",)  # hand_receiver's stages


# ---- hand-made rows on a channel-rate context
@functools.lru_cache(maxsize=None)
def hand_rows():
    """int16 [2, 2 B, 2].  A tone (every sample over the threshold) from a to b gives the run [a, b + W): its last W - 1 samples
    are the trigger's hold.
    Stream 0: a run from 1024 whose tone fills segments 1 and 2 (keyed every 64 samples: 6000 Hz); one from 1024 * 4 + 1 that ends
    on 1024 * 7 (keyed every 10: 38400 Hz, as the rest); in block 1 one from 1024 * 9 that ends a sample short of 1024 * 12; one of
    2046 samples from 1024 * 12 + 1, which holds no segment; one open at the input's last sample.
    Stream 1: from sample 1 every other sample (0, 0) with a large pair between -- a silent segment --; a keyed run from 5000
    across the block boundary into the eight segments of mx_rows (the normalising shift's steps), open at the end."""
    rows = np.stack([quiet(2, 21), quiet(2, 22)])
    k10, k64 = keyed(2, 10, seed=3).reshape(-1, 2), keyed(2, 64, seed=4).reshape(-1, 2)
    for a, b, src in ((SEG, 3 * SEG, k64), (4 * SEG + 1, 7 * SEG - W + 1, k10), (9 * SEG, 12 * SEG - W, k10),
                      (12 * SEG + 1, 12 * SEG + 1 + 2046 - W + 1, k10), (2 * B - 1500, 2 * B, k10)):
        rows[0, a:b] = src[a:b]
    rows[1, :3000] = silent_rows().reshape(-1, 2)[:3000]
    rows[1, 5000:B] = k10[5000:B]
    rows[1, B:] = mx_rows().reshape(-1, 2)
    rows.setflags(write=False)
    return rows


@functools.lru_cache(maxsize=None)
def hand_uncut():
    rows = hand_rows()
    with hand_receiver(2, 2, CLOCK, levels=False) as r:
        r.submit(np.ascontiguousarray(rows))
        got, decs, runs = read_clock(r, 2, [0, 0])
        assert r.read_burst_clocks().tobytes() == got.tobytes()  # reading pops nothing
        r.drain()
        raises(api.E_STATE, r.read_burst_clocks)  # nothing undrained
    assert np.array_equal(np.stack(decs).reshape(2, 2 * B, 2), decin.clamp(rows))
    return got


def test_two_streams_of_two_blocks_of_hand_made_samples():
    got = hand_uncut()
    by_start = {(int(r["stream"]), int(r["start_sample"])): r for r in got}
    assert sorted(by_start) == [(0, SEG), (0, 4 * SEG + 1), (0, 9 * SEG), (0, 12 * SEG + 1), (0, 2 * B - 1500), (1, 1), (1, 5000)]
    seg = lambda s, a: (int(by_start[s, a]["n_samples"]), int(by_start[s, a]["n_segments"]), int(by_start[s, a]["n_silent"]))  # noqa: E731
    # the rows hold what they are meant to hold (the values: the restatement's, on the CPU)
    assert seg(0, SEG) == (2 * SEG + W - 1, 2, 0)  # from a boundary: segments 1 and 2
    assert seg(0, 4 * SEG + 1) == (3 * SEG - 1, 2, 0)  # from a sample behind one, up to one: segments 5 and 6
    assert seg(0, 9 * SEG) == (3 * SEG - 1, 2, 0)  # a sample short of a boundary: segments 9 and 10
    assert seg(0, 12 * SEG + 1) == (2046, 0, 0) and clock.summary(by_start[0, 12 * SEG + 1]) is None
    assert seg(0, 2 * B - 1500) == (1500, 1, 0) and by_start[0, 2 * B - 1500]["flags"] == OPEN  # open at the last sample: segment 15
    assert seg(1, 1) == (2999 + W - 1, 1, 1)  # segment 1 is silent, segment 2 ends in noise
    assert seg(1, 5000) == (2 * B - 5000, 3 + 8, 0) and by_start[1, 5000]["flags"] == OPEN
    hz64, q64 = clock.summary(by_start[0, SEG])
    hz10, q10 = clock.summary(by_start[0, 4 * SEG + 1])
    assert abs(hz10 - 38400) <= 375 and q10 > 2500  # the peak bin is the keying's
    # keyed every 64 samples, the signal has period 64: its spectrum lies on the multiples of 6000 Hz, bin 16 k, and a harmonic may win
    assert (hz64 + 375) % 6000 <= 750 and q64 > 1000


def test_the_same_input_in_two_submits_and_the_merged_chains():
    whole = hand_uncut()
    rows = hand_rows()
    with hand_receiver(2, 1, CLOCK, levels=False) as r:
        for k in range(2):  # both queued before the first read
            r.submit(np.ascontiguousarray(rows[:, k * B:(k + 1) * B]))
        got = []
        for k in range(2):
            part = decin.clamp(rows[:, k * B:(k + 1) * B])  # (a channel-rate context's samples are its input, clamped: hand_uncut)
            got.append(read_clock(r, 1, [k * B] * 2, decs=[part[s].reshape(-1) for s in range(2)])[0])
            r.drain()
    c = got[1][(got[1]["flags"] & CONT) != 0]
    assert c["stream"].tolist() == [1] and c[0]["start_sample"] == B and c[0]["n_segments"] == 8
    o = got[0][(got[0]["flags"] & OPEN) != 0]
    assert o["stream"].tolist() == [1] and (o[0]["n_samples"], o[0]["n_segments"]) == (B - 5000, 3)
    key = lambda r: (int(r["stream"]), int(r["start_sample"]))  # noqa: E731
    merged, uncut = sorted(clock.chains(got), key=key), sorted(clock.chains([whole]), key=key)
    assert len(merged) == len(uncut) == len(whole)
    same_chains("clock", merged, uncut, "1 + 1")


def test_an_auto_stream_of_eight_blocks():
    nb = 8
    rng = np.random.default_rng(31)
    x = np.stack([rng.integers(-400, 401, size=(nb * B, 2)), rng.integers(-330, 331, size=(nb * B, 2))]).astype(np.int16)
    with hand_receiver(2, nb, CLOCK, levels=False, thresh=0) as r:
        r.submit(x)
        got, decs, runs = read_clock(r, nb, [0, 0])
        r.drain()
    r0 = got[got["stream"] == 0]
    assert len(r0) == 1 and r0[0]["n_samples"] >= nb * B - 16 and r0[0]["flags"] == OPEN
    assert r0[0]["n_segments"] >= 8 * nb - 1 and clock.summary(r0[0])[1] < 800  # noise: no clock stands out


@pytest.mark.parametrize("n", [65, 97])
def test_stream_counts_across_a_waves_end(n):
    nb = 4
    rng = np.random.default_rng(41)
    kinds = [rng.integers(-400, 401, size=(nb * B, 2)).astype(np.int16), keyed(nb, 10, seed=5).reshape(-1, 2),
             keyed(nb, 16, seed=6, amp=9000).reshape(-1, 2), quiet(nb, 43)]  # rows 0 .. 2 never leave their window
    kinds[0][0] = (300, 300)  # (... from the first sample on)
    x = np.ascontiguousarray(np.stack(kinds)[np.arange(n) % len(kinds)])
    with hand_receiver(n, nb, CLOCK, levels=False) as r:
        r.submit(x)
        got, decs, runs = read_clock(r, nb, [0] * n)
        r.drain()
    assert got["stream"].tolist() == [s for s in range(n) if s % 4 != 3]  # (row 3 is quiet)
    assert (got["n_samples"] == nb * B).all() and (got["n_segments"] == 8 * nb).all() and (got["flags"] == OPEN).all()
    for s in range(3):  # every copy of a row has the row's record
        assert len({r.tobytes()[4:] for r in got[got["stream"] % 4 == s]}) == 1
    assert abs(clock.summary(got[1])[0] - 38400) <= 375 and abs(clock.summary(got[2])[0] - 24000) <= 375


# ---- the other kinds of context
def scene_receiver(**kw):
    r = R.receiver(**kw)
    r.enable_burst_clock()
    return r


@functools.lru_cache(maxsize=None)
def scene_uncut():
    with scene_receiver() as r:
        r.submit(scene())
        got, decs, runs = read_clock(r, NB, [0] * N)
        ev = r.drain()
    return got, decs, runs, ev


def test_a_reset_mid_chain_drops_the_chain():
    parts = parity.cut(scene(), (2, 2))
    with scene_receiver(max_blocks=2) as r:
        r.submit(parts[0])
        got0, d0, _ = read_clock(r, 2, [0] * N)
        r.drain()
        r.reset_streams([1, 6])
        r.submit(parts[1])
        base = [0 if s in (1, 6) else 2 * B for s in range(N)]  # a reset stream counts from 0 again
        got1, _, _ = read_clock(r, 2, base)
        r.drain()
    assert got0[got0["stream"] == 6][-1]["flags"] & OPEN
    r6 = got1[got1["stream"] == 6]
    assert not (r6["flags"] & CONT).any() and r6[0]["start_sample"] < 16
    r7 = got1[got1["stream"] == 7][0]  # 7 was not reset: its piece continues
    assert r7["flags"] & CONT and r7["start_sample"] == 2 * B
    ch = clock.chains([got0, got1], restarts={1: [1, 6]})
    six = [c for c in ch if c["stream"] == 6]
    assert len(six) == len(got0[got0["stream"] == 6]) + len(r6)  # nothing of stream 6 was merged across the reset
    dropped = six[len(six) - len(r6) - 1]  # the chain the reset cut off: it ends, still OPEN, where the first submit ends
    assert dropped.tobytes() == clock.merge([got0[got0["stream"] == 6][-1]]).tobytes() and dropped["flags"] & OPEN
    assert dropped["start_sample"] + dropped["n_samples"] == 2 * B and dropped["n_segments"] >= 8
    whole, _, _, ev = scene_uncut()
    assert parity.sort_events(ev).tobytes() == parity.sort_events(R.one_submit()[2]).tobytes()  # the events do not notice
    seven = [c for c in ch if c["stream"] == 7 and c["start_sample"] < 2 * B < c["start_sample"] + c["n_samples"]]
    assert len(seven) == 1 and seven[0].tobytes() == [c for c in clock.chains([whole])
                                                      if c["stream"] == 7 and c["start_sample"] == seven[0]["start_sample"]][0].tobytes()


def test_a_golden_scene_with_the_meter_and_the_envelope_beside_it_and_none():
    x = golden_iq()
    with api.Receiver(1, 0x2F, 500, 0, max_blocks=4, all_flushes=True) as r:
        plain_mem = r.memory()
        r.submit(x)
        plain = r.drain()
    with api.Receiver(1, 0x2F, 500, 0, max_blocks=4, all_flushes=True, levels=True) as r:
        r.enable_capture(256, 4 * B)
        rec_mem = r.memory()
        r.submit(x)
        plain_runs = r.read_captures()
        r.drain()
    with api.Receiver(1, 0x2F, 500, 0, max_blocks=4, all_flushes=True, levels=True) as r:
        r.enable_capture(256, 4 * B)
        assert r.memory() == rec_mem  # a recorder without the call holds what it held
        r.enable_burst_clock()
        r.enable_burst_meter()
        r.enable_burst_envelope()
        r.submit(x)
        got, decs, runs = read_clock(r, 4, [0])
        read_envelope(r, 4, zeros(1), [0])  # the envelope's records, exact
        bursts = r.read_bursts()
        tab = r.read_captures()
        ev = r.drain()
    with api.Receiver(1, 0x2F, 500, 0, max_blocks=4, all_flushes=True) as r:
        assert r.memory() == plain_mem  # a context without the call holds what it held
    assert bursts.tobytes() == burst.bursts(decs, runs, zeros(1)).tobytes() and len(bursts) == len(got) >= 2
    R.assert_tables(tab, plain_runs)
    assert parity.sort_events(ev).tobytes() == parity.sort_events(plain).tobytes() and len(ev) >= 1
    sm = [clock.summary(c) for c in got if c["n_segments"] >= 1]
    assert len(sm) >= 2 and all(abs(hz - 17240) <= 150 and q >= 2500 for hz, q in sm)  # TFA_2's bit rate


def test_a_submit_runs_replay_gives_the_recordings_records():
    """The golden TFA_2 scene recorded by a u8 context (1 + 3 blocks) and replayed through sparse submits (2 + 2): a run's samples
    are the recording's and a segment reads nothing else, so the merged records are the recording's."""
    x = golden_iq()
    with api.Receiver(1, 0x2F, 500, 0, max_blocks=3, all_flushes=True) as r:
        r.enable_capture(256, 4 * B)
        r.enable_capture_pre()
        r.enable_burst_clock()
        tabs, recs, pos = [], [], 0
        for p, nb in zip(parity.cut(x, (1, 3)), (1, 3)):
            r.submit(p)
            tabs.append(r.read_captures(pre=True))
            recs.append(read_clock(r, nb, [pos * B])[0])
            pos += nb
            r.drain()
    off = 0
    for t, pool, _ in tabs:
        t["pool_offset"] += off
        off += len(pool)
    runs, pool, pre = (np.concatenate([t[i] for t in tabs]) for i in range(3))
    assert len(runs) >= 2
    with api.Receiver(1, 0x2F, 500, 0, max_blocks=2, all_flushes=True, decimated=True) as r:
        r.enable_runs_input(len(runs) + 2, len(pool) + 1)
        r.enable_capture(256, 1)
        r.enable_burst_clock()
        rep = []
        for k in range(2):
            t, p, q = decin.rebase(runs, pool, pre, 2 * k * B, 2 * B)
            assert r.submit_runs(t, p, q, 2) == 2
            rep.append(read_clock(r, 2, [2 * k * B])[0])
            r.drain()
    a, b = clock.chains(recs), clock.chains(rep)
    assert len(a) == len(b) >= 2 and sum(int(c["n_segments"]) for c in a) >= 3
    same_chains("clock", b, a, "the replay")


def test_overflow_delivers_the_prefix_and_a_pool_of_one_pair_delivers_everything():
    whole = hand_uncut()
    rows = np.ascontiguousarray(hand_rows())
    with hand_receiver(2, 2, CLOCK, levels=False, cap=(len(whole) - 1, 1)) as r:
        r.submit(rows)
        raises(api.E_OVERFLOW, r.read_burst_clocks)
        got = r.read_burst_clocks(allow_overflow=True)
        assert r.clock_total == len(whole)
        same_records(got, whole[:-1], "the prefix")
        r.drain()
    with hand_receiver(2, 2, CLOCK, levels=False, cap=(len(whole), 1)) as r:  # the clock alone, the table just large enough
        r.submit(rows)
        same_records(r.read_burst_clocks(), whole, "a pool of one pair")
        assert len(r.read_captures(allow_overflow=True)[1]) <= 1  # the pool itself held nothing
        r.drain()


def test_the_refusals_of_the_enable_call_and_what_a_context_without_it_holds():
    n, mb = 3, 2
    x = scene()[:n, :api.BLOCK_BYTES]
    with api.Receiver(n, CTX_TYPES, 500, 0, max_blocks=mb) as r:
        plain = r.memory()
        raises(api.E_INVAL, r.enable_burst_clock)  # no recorder
        raises(api.E_INVAL, r.read_burst_clocks)
        assert r.memory() == plain
        r.enable_capture(64, 1024)
        rec = r.memory()
        raises(api.E_INVAL, r.read_burst_clocks)  # the recorder alone: no clock
        r.submit(x)
        raises(api.E_INVAL, r.read_burst_clocks)
        submitted = r.memory()  # (a host submit's staging is counted)
        raises(api.E_STATE, r.enable_burst_clock)  # after the first submit
        assert r.memory() == submitted
        runs_plain = r.read_captures()
        ev_plain = r.drain()
    with api.Receiver(n, CTX_TYPES, 500, 0, max_blocks=mb) as r:
        r.enable_capture(64, 1024)
        assert r.memory() == rec  # a recorder without the clock holds what it held
        r.enable_burst_clock()
        m = r.memory()
        assert m["device_bytes"] - rec["device_bytes"] == api.FIFO_DEPTH * 64 * 1056 and m["pinned_host_bytes"] == rec["pinned_host_bytes"]
        raises(api.E_INVAL, r.enable_burst_clock)  # a second call: refused, and nothing changes
        assert r.memory() == m
        r.enable_burst_meter()  # independent of the meter and the envelope: any order
        r.enable_burst_envelope()
        assert r.memory()["device_bytes"] - m["device_bytes"] == api.FIFO_DEPTH * 64 * (320 + 128)
        raises(api.E_STATE, r.read_burst_clocks)  # nothing undrained
        r.submit(x)
        nr = api.C.c_uint32(0)
        buf = np.full(1056, 0x55, dtype=np.uint8)  # the caller's room too small: E_INVAL, nothing written, the count set
        assert r.L.tfrec_amd_read_burst_clocks(r.h, buf.ctypes.data, 0, api.C.byref(nr)) == api.E_INVAL and (buf == 0x55).all()
        assert r.L.tfrec_amd_read_burst_clocks(r.h, buf.ctypes.data, 1, None) == api.E_INVAL
        recs = r.read_burst_clocks()
        assert nr.value == len(recs) == len(runs_plain[0]) == len(r.read_bursts()) == len(r.read_burst_envelopes()) == 1
        runs = r.read_captures()
        ev = r.drain()
    R.assert_tables(runs, runs_plain)
    assert parity.sort_events(ev).tobytes() == parity.sort_events(ev_plain).tobytes()


def test_a_context_of_4096_blocks_is_refused():
    """A record's spec is summed on the device: 8 segments a block, below 2^15 segments it cannot overflow."""
    with api.Receiver(1, 0x01, 500, 0, max_blocks=4096, decimated=True) as r:
        r.enable_capture(4, 1)
        m = r.memory()
        raises(api.E_INVAL, r.enable_burst_clock)
        assert r.memory() == m


# ---- tfrec_gpu -C
@functools.lru_cache(maxsize=None)
def whb_lines():
    """The golden WHB scene's first 6 blocks -> (its bytes, the lines clock.py expects of tfrec_gpu -C -b 2 on a file named %s)."""
    x = np.ascontiguousarray(golden_iq("whb", 6)[0])
    # the restatement: the oracle's front end (the context's, bit for bit), capture.py and clock.py submit by submit (2 + 2 + 2)
    dec = parity.fresh_oracle(x, 0x2F, 500, keep_dec=True).dec().reshape(-1, 2)
    recs, st = [], None
    for a, b in ((0, 2), (2, 4), (4, 6)):
        part = dec[a * B:b * B]
        runs, _, st = capture.captures(part, 0x2F, 500, st)
        recs.append(clock.clocks([part], runs, base=[a * B]))
    assert any(c["flags"] & CONT for c in recs[1]) and any(c["flags"] & CONT for c in recs[2])  # a burst is cut by the batches, twice
    want = [clock.line("%s", c) for c in clock.chains(recs)]
    assert any(int(ln.split()[4]) >= 20 and abs(int(ln.split()[5]) - 6000) <= 150 for ln in want)  # WHB's 6000 bit/s
    return x, want


BASE = ["-T", "2f", "-t", "500", "-b", "2"]  # -b 2: the burst lies in all three batches
WORDS = ("clock", "burst", "extent", "scan")


def test_cli_clock_lines_of_the_golden_whb_scene_cut_into_batches(tmp_path):
    parity.build_cli()
    x, want = whb_lines()
    f = str(tmp_path / "whb.iq")
    x.tofile(f)
    want = [ln % f for ln in want]
    plain = cli_lines(BASE + ["-L", f], *WORDS)
    got = cli_lines(["-C"] + BASE + ["-L", f], *WORDS)
    assert plain["clock"] == [] and got["telegrams"] == plain["telegrams"] and got["burst"] == got["extent"] == []  # the telegrams do not notice
    assert got["clock"] == want and len(want) >= 1
    f2 = str(tmp_path / "short.iq")  # through a recycled slot beside a second file
    x[:2 * api.BLOCK_BYTES].tofile(f2)
    slot = cli_lines(["-C", "-n", "1"] + BASE + ["-L", f, "-L", f2], *WORDS)
    assert [ln for ln in slot["clock"] if ln.split()[1] == f] == want


def test_cli_clock_beside_the_meter_and_the_envelope_and_the_scans_column(tmp_path):
    parity.build_cli()
    x, want = whb_lines()
    f = str(tmp_path / "whb.iq")
    x.tofile(f)
    want = [ln % f for ln in want]
    # beside -M and -Q: all three kinds of line, each what it is alone
    alone = cli_lines(["-M", "-Q"] + BASE + ["-L", f], *WORDS)
    both = cli_lines(["-M", "-Q", "-C"] + BASE + ["-L", f], *WORDS)
    assert alone["clock"] == [] and both["clock"] == want
    assert all(both[w] == alone[w] for w in ("burst", "extent", "telegrams"))
    assert len(alone["burst"]) == len(alone["extent"]) == len(want)
    # the channel table's column
    scan = cli_lines(["-C", "-s", "100", "-t", "500", "-L", f], *WORDS)
    assert scan["clock"] == [] and len(scan["scan"]) >= 3 and all(re.search(r" burst_clock=(-|\d+)$", ln) for ln in scan["scan"])
    assert any(not ln.endswith("=-") for ln in scan["scan"])
    assert all("burst_clock" not in ln for ln in cli_lines(["-s", "100", "-t", "500", "-L", f], "scan")["scan"])
