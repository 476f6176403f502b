"""The burst track on the GPU (tfrec_amd_enable_burst_track, tfrec_amd_set_burst_track_centre, tfrec_amd_read_burst_tracks,
tfrec_gpu -G), bit for bit.

The records and the bitmap's words are compared, byte for byte, with the restatement tfrec_amd/track.py run on the context's OWN
decimated samples (tfrec_amd_read_decimated), its own run table and the thresholds read back from the same submit, so the front end
and the recorder ahead of the track are whatever the context runs (recorder.read_track).  Channel-rate contexts
(tfrec_amd_create_decimated) take hand-made decimated samples: the layouts the kernels can get wrong are placed exactly.
Everything is an exact integer; nothing here has a tolerance.  Nothing here is measured on real recordings."""
import functools

import numpy as np
import pytest

import parity
import recorder as R
from recorder import (B, CONT, OPEN, W, cli_lines, hand_receiver, raises, read_clock, read_envelope, read_track, same_chains,
                      same_records, zeros)
from recorder_rows import CTX_TYPES, N, NB, TELEGRAMS, bit_string, golden_iq, keyed, pattern, quiet, scene, shifted_tfa_2
from tfrec_amd import api, burst, decin, track

pytestmark = pytest.mark.gpu


# ---- hand-made rows on a channel-rate context
CENTRES = {1: [0, 20000], 5: [0, -35000], 16: [0, 20000]}


@functools.lru_cache(maxsize=None)
def hand_rows():
    """int16 [2, 2 B, 2].  A tone (every sample over the threshold) from a to b gives the run [a, b + W): its last W - 1 samples are
    the trigger's hold.
    Stream 0: a run from the submit's first sample (37 keyed samples: 730 long, so every later run of the pool starts off a word
    boundary); a stretch of constant samples -- every crs is 0, and about centre 0 every sum --; a keyed run from B - 3 across the
    block boundary (cut there, its first piece is 3 samples); one open at the input's last sample.
    Stream 1: a run of 1 over sample; a keyed run from 3001 of 1001 tone samples; a run that ends a sample ahead of block 0's last
    one; one from block 1's first sample."""
    rows = np.stack([quiet(2, 21), quiet(2, 22)])
    k10, k22 = keyed(2, 10, seed=3).reshape(-1, 2), keyed(2, 22, seed=4).reshape(-1, 2)
    for a, b, src in ((0, 37, k10), (B - 3, B + 2000, k22), (2 * B - 1500, 2 * B, k10)):
        rows[0, a:b] = src[a:b]
    rows[0, 2000:2300] = (3000, 0)
    rows[1, 1000] = (-2500, 2600)
    for a, b, src in ((3001, 4002, k22), (B - W - 50, B - W, k10), (B, B + 500, k22)):
        rows[1, a:b] = src[a:b]
    rows.setflags(write=False)
    return rows


@functools.lru_cache(maxsize=None)
def hand_uncut(L):
    rows = hand_rows()
    with hand_receiver(2, 2, {"track": (L,)}) as r:
        r.set_burst_track_centre([0, 1], CENTRES[L])
        r.submit(np.ascontiguousarray(rows))
        got, words, decs, _ = read_track(r, 2, [0, 0], L, CENTRES[L], None)
        again = r.read_burst_tracks()  # reading pops nothing
        assert again[0].tobytes() == got.tobytes() and again[1].tobytes() == words.tobytes()
        r.drain()
        raises(api.E_STATE, r.read_burst_tracks)  # nothing undrained
    assert np.array_equal(np.stack(decs).reshape(2, 2 * B, 2), decin.clamp(rows))
    return got, words


@pytest.mark.parametrize("L", [1, 5, 16])
def test_two_streams_of_two_blocks_of_hand_made_samples(L):
    got, words = hand_uncut(L)
    by_start = {(int(r["stream"]), int(r["start_sample"])): r for r in got}
    assert sorted(by_start) == [(0, 0), (0, 2000), (0, B - 3), (0, 2 * B - 1500), (1, 1000), (1, 3001), (1, B - W - 50), (1, B)]
    # the rows hold what they are meant to hold (the values: the restatement's, on the CPU)
    first = by_start[0, 0]
    assert first["flags"] == 0 and (first["n_samples"], first["last_over"], first["bit_offset"]) == (36 + W, 36, 0)
    assert (got["bit_offset"][1:] % 32 != 0).all()  # every later run shares its first word with the run ahead of it
    still = by_start[0, 2000]
    assert (still["n_samples"], still["last_over"]) == (299 + W, 299)
    assert not track.bits_of(still, words)[:300].any()  # the constant stretch: every sum is exactly 0
    across = by_start[0, B - 3]
    assert across["n_samples"] == 2002 + W and across["n_ones"] > 500
    last0 = by_start[0, 2 * B - 1500]
    assert last0["flags"] == OPEN and (last0["n_samples"], last0["last_over"]) == (1500, 1499)
    one = by_start[1, 1000]
    assert (one["n_samples"], one["last_over"]) == (W, 0)
    end = by_start[1, B - W - 50]
    assert end["start_sample"] + end["n_samples"] == B - 1 and end["flags"] == 0  # block 0's last sample is not captured
    assert by_start[1, B]["flags"] == 0 and by_start[1, B]["start_sample"] == B  # a run from a block's first sample
    assert by_start[1, 3001]["last_over"] == 1000
    if CENTRES[L][1] == 20000:  # keyed every 22 samples between +-46 kHz: the slice at 384000 / 22 bit/s alternates
        symbols = track.slice_bits(track.bits_of(by_start[1, 3001], words)[:1001], 17455)
        assert len(symbols) >= 44 and all(a != b for a, b in zip(symbols, symbols[1:]))


@pytest.mark.parametrize("L", [1, 5, 16])
def test_the_same_rows_in_two_submits_queued_before_the_first_read(L):
    whole, wwords = hand_uncut(L)
    rows = hand_rows()
    with hand_receiver(2, 1, {"track": (L,)}) as r:
        r.set_burst_track_centre([0, 1], CENTRES[L])
        for k in range(2):  # both queued before the first read
            r.submit(np.ascontiguousarray(rows[:, k * B:(k + 1) * B]))
        got, st = [], None
        for k in range(2):
            part = decin.clamp(rows[:, k * B:(k + 1) * B])  # (a channel-rate context's samples are its input, clamped: hand_uncut)
            recs, words, _, st = read_track(r, 1, [k * B] * 2, L, CENTRES[L], st, decs=[part[s].reshape(-1) for s in range(2)])
            if k == 0:
                assert st["prior"].tolist() == [3, 0]  # stream 0's chain begins 3 samples ahead of the cut
            got.append((recs, words))
            r.drain()
    c = got[1][0][(got[1][0]["flags"] & CONT) != 0]
    assert c["stream"].tolist() == [0] and c[0]["start_sample"] == B
    o = got[0][0][(got[0][0]["flags"] & OPEN) != 0]
    assert o["stream"].tolist() == [0] and o[0]["n_samples"] == 3
    key = lambda c: (int(c["stream"]), int(c["start_sample"]))  # noqa: E731
    merged, uncut = sorted(track.chains(got), key=key), sorted(track.chains([(whole, wwords)]), key=key)
    assert len(merged) == len(uncut) == len(whole)
    same_chains("track", merged, uncut, "1 + 1")


@pytest.mark.parametrize("n", [65, 97])
def test_stream_counts_across_a_waves_end(n):
    nb, L = 4, 7
    rng = np.random.default_rng(41)
    kinds = [rng.integers(-400, 401, size=(nb * B, 2)).astype(np.int16), keyed(nb, 10, seed=5).reshape(-1, 2),
             keyed(nb, 16, seed=6, amp=9000).reshape(-1, 2), quiet(nb, 43)]  # rows 0 .. 2 never leave their window
    kinds[0][0] = (300, 300)  # (... from the first sample on)
    x = np.ascontiguousarray(np.stack(kinds)[np.arange(n) % len(kinds)])
    centres = [(0, 20000, -35000)[s % 3] for s in range(n)]
    with hand_receiver(n, nb, {"track": (L,)}) as r:
        r.set_burst_track_centre(range(n), centres)
        r.submit(x)
        got, words, decs, st = read_track(r, nb, [0] * n, L, centres, None)
        r.drain()
    assert got["stream"].tolist() == [s for s in range(n) if s % 4 != 3]  # (row 3 is quiet)
    assert (got["n_samples"] == nb * B).all() and (got["flags"] == OPEN).all() and len(words) == len(got) * nb * B // 32
    assert st["prior"].tolist() == [16 if s % 4 != 3 else 0 for s in range(n)]
    for s in (1, 2):  # copies of a row about the same centre have the row's track
        same = [track.bits_of(g, words).tobytes() for g in got if g["stream"] % 12 == s]
        assert len(same) >= 5 and len(set(same)) == 1
    assert len({track.bits_of(g, words).tobytes() for g in got if g["stream"] % 4 == 1}) == 3  # ... and about another, another


def test_a_centre_changed_between_two_submits():
    """Not a restart: the chain continues, and the second piece -- the carried products included -- is formed about the new centre."""
    rows = hand_rows()
    L = 5
    with hand_receiver(2, 1, {"track": (L,)}) as r:
        raises(api.E_INVAL, r.set_burst_track_centre, [0], [192001])
        raises(api.E_INVAL, r.set_burst_track_centre, [0, 2], [0, 0])  # a stream out of range: nothing is set
        raises(api.E_INVAL, r.set_burst_track_centre, [1, 0], [5000, -192001])
        r.set_burst_track_centre([], [])
        r.submit(np.ascontiguousarray(rows[:, :B]))
        a, wa, d0, st = read_track(r, 1, [0, 0], L, [0, 0], None)  # the refused calls set nothing
        r.drain()
        r.set_burst_track_centre([0, 1], [-60000, 192000])
        r.submit(np.ascontiguousarray(rows[:, B:]))
        b, wb, _, st = read_track(r, 1, [B, B], L, [-60000, 192000], st)
        r.drain()
    assert b[0]["flags"] & CONT and b[0]["stream"] == 0
    ch = [c for c in track.chains([(a, wa), (b, wb)]) if c["stream"] == 0 and c["start_sample"] == B - 3]
    assert len(ch) == 1 and ch[0]["n_samples"] == 2002 + W
    # about -60 kHz both tones of the keyed run (+-46 kHz) lie above the centre: ones throughout the tone
    assert ch[0].bits[3 + L:2000].all()


# ---- the other kinds of context
def scene_receiver(L, **kw):
    r = R.receiver(levels=True, **kw)
    r.enable_burst_track(L)
    return r


def test_a_reset_mid_chain_drops_the_chain():
    L = 9
    parts = parity.cut(scene(), (2, 2))
    cen = [0, 20000, 0, -35000, 0, 0, 20000, 20000]
    with scene_receiver(L, max_blocks=2) as r:
        r.set_burst_track_centre(range(N), cen)
        r.submit(parts[0])
        got0, w0, _, st = read_track(r, 2, [0] * N, L, cen, None)
        r.drain()
        r.reset_streams([1, 6])
        r.submit(parts[1])
        base = [0 if s in (1, 6) else 2 * B for s in range(N)]  # a reset stream counts from 0 again
        got1, w1, _, st = read_track(r, 2, base, L, cen, st)
        ev1 = r.drain()
    assert got0[got0["stream"] == 6][-1]["flags"] & OPEN
    r6 = got1[got1["stream"] == 6]
    assert not (r6["flags"] & CONT).any() and r6[0]["start_sample"] < 16
    r7 = got1[got1["stream"] == 7][0]  # 7 was not reset: its piece continues
    assert r7["flags"] & CONT and r7["start_sample"] == 2 * B
    ch = track.chains([(got0, w0), (got1, w1)], restarts={1: [1, 6]})
    six = [c for c in ch if c["stream"] == 6]
    assert len(six) == len(got0[got0["stream"] == 6]) + len(r6)  # nothing of stream 6 was merged across the reset
    with scene_receiver(L) as r:  # the uncut scene: stream 7's chain across the cut is the uncut run
        r.set_burst_track_centre(range(N), cen)
        r.submit(scene())
        whole, ww, _, _ = read_track(r, NB, [0] * N, L, cen, None)
        r.drain()
    seven = [c for c in ch if c["stream"] == 7 and c["start_sample"] < 2 * B < c["start_sample"] + c["n_samples"]]
    assert len(seven) == 1
    u = [c for c in track.chains([(whole, ww)]) if c["stream"] == 7 and c["start_sample"] == seven[0]["start_sample"]]
    assert len(u) == 1
    same_chains("track", seven, u, "stream 7 across the cut")


def test_the_golden_tfa_2_scene_with_all_four_measurements_and_none():
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
        r.enable_burst_track(11)
        r.enable_burst_clock()
        r.enable_burst_meter()
        r.enable_burst_envelope()
        r.submit(x)
        got, words, decs, _ = read_track(r, 4, [0], 11, [0], None)
        read_clock(r, 4, [0])  # the clock's records, exact
        env = read_envelope(r, 4, zeros(1), [0])[0]  # the envelope's
        bursts = r.read_bursts()
        tab = r.read_captures()
        ev = r.drain()
    with api.Receiver(1, 0x2F, 500, 0, max_blocks=4, all_flushes=True) as r:
        assert r.memory() == plain_mem  # a context without the call holds what it held
    assert bursts.tobytes() == burst.bursts(decs, tab[0], zeros(1)).tobytes() and len(bursts) == len(got) == 2
    assert np.array_equal(env["last_over"], got["last_over"])
    R.assert_tables(tab, plain_runs)
    assert parity.sort_events(ev).tobytes() == parity.sort_events(plain).tobytes() and len(ev) >= 1
    lines = [track.line("f", c, 17240) for c in track.chains([(got, words)])]
    assert [ln.split()[4:6] for ln in lines] == [["1474", "66"], ["1475", "66"]]
    for c, tel in zip(track.chains([(got, words)]), TELEGRAMS["tfa_2"]):
        assert pattern(tel) in bit_string(track.slice_bits(c.bits[:int(c["last_over"]) + 1], 17240))


def test_a_submit_runs_replay_gives_the_recordings_track():
    """The golden TFA_2 scene recorded by a u8 context (1 + 3 blocks) and replayed through sparse submits (2 + 2): a run's samples
    are the recording's and nothing ahead of a chain is used, so the merged records and tracks are the recording's."""
    x = golden_iq()
    L = 11
    with api.Receiver(1, 0x2F, 500, 0, max_blocks=3, all_flushes=True, levels=True) as r:
        r.enable_capture(256, 4 * B)
        r.enable_capture_pre()
        r.enable_burst_track(L)
        tabs, recs, pos, st = [], [], 0, None
        for p, nb in zip(parity.cut(x, (1, 3)), (1, 3)):
            r.submit(p)
            tabs.append(r.read_captures(pre=True))
            g, w, _, st = read_track(r, nb, [pos * B], L, [0], st)
            recs.append((g, w))
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
        r.enable_capture(256, 2 * B)
        r.enable_burst_track(L)
        rep, st = [], None
        for k in range(2):
            t, p, q = decin.rebase(runs, pool, pre, 2 * k * B, 2 * B)
            assert r.submit_runs(t, p, q, 2) == 2
            g, w, _, st = read_track(r, 2, [2 * k * B], L, [0], st, levels=False)
            rep.append((g, w))
            r.drain()
    a, b = track.chains(recs), track.chains(rep)
    assert len(a) == len(b) == 2
    same_chains("track", b, a, "the replay")


def test_overflow_on_max_runs_and_on_max_samples_delivers_the_prefixes():
    L = 5
    whole, wwords = hand_uncut(L)
    rows = np.ascontiguousarray(hand_rows())
    with hand_receiver(2, 2, {"track": (L,)}, cap=(len(whole) - 1, 4 * B)) as r:  # the table a run short
        r.set_burst_track_centre([0, 1], CENTRES[L])
        r.submit(rows)
        raises(api.E_OVERFLOW, r.read_burst_tracks)
        got, words, _, _ = read_track(r, 2, [0, 0], L, CENTRES[L], None, overflow=True)
        assert r.track_total == len(whole) and r.capture_overflow
        same_records(got, whole[:-1], "the prefix")
        assert len(words) == (int(whole[-1]["bit_offset"]) + 31) // 32  # the pairs of the runs the table holds
        r.drain()
    room = int(whole[3]["bit_offset"] + whole[3]["n_samples"])  # the pool holds the first four runs, and not the fifth
    with hand_receiver(2, 2, {"track": (L,)}, cap=(32, room + 10)) as r:
        r.set_burst_track_centre([0, 1], CENTRES[L])
        r.submit(rows)
        raises(api.E_OVERFLOW, r.read_burst_tracks)
        got, words, _, _ = read_track(r, 2, [0, 0], L, CENTRES[L], None, overflow=True)
        same_records(got, whole, "every record")  # ... n_ones of the runs whose bits did not fit included
        assert len(words) == (room + 31) // 32 and len(r.read_captures(allow_overflow=True)[0]) == 4
        r.drain()


def test_the_refusals_and_the_memory_sums():
    n, mb = 3, 2
    x = scene()[:n, :api.BLOCK_BYTES]
    with api.Receiver(n, CTX_TYPES, 500, 0, max_blocks=mb) as r:
        plain = r.memory()
        raises(api.E_INVAL, r.enable_burst_track, 5)  # no recorder
        raises(api.E_INVAL, r.read_burst_tracks)
        raises(api.E_INVAL, r.set_burst_track_centre, [0], [0])  # not enabled
        assert r.memory() == plain
        r.enable_capture(64, 1024)
        rec = r.memory()
        raises(api.E_INVAL, r.read_burst_tracks)  # the recorder alone: no track
        for bad in (0, 17, -1, 2 ** 31):
            raises(api.E_INVAL, r.enable_burst_track, bad)
        assert r.memory() == rec
        r.submit(x)
        raises(api.E_INVAL, r.read_burst_tracks)
        submitted = r.memory()  # (a host submit's staging is counted)
        raises(api.E_STATE, r.enable_burst_track, 5)  # after the first submit
        assert r.memory() == submitted
        runs_plain = r.read_captures()
        ev_plain = r.drain()
    with api.Receiver(n, CTX_TYPES, 500, 0, max_blocks=mb) as r:
        r.enable_capture(64, 1024)
        assert r.memory() == rec  # a recorder without the track holds what it held
        r.enable_burst_track(16)
        m = r.memory()
        assert m["device_bytes"] - rec["device_bytes"] == track.device_bytes(n, 64, 1024)
        assert m["pinned_host_bytes"] - rec["pinned_host_bytes"] == track.pinned_bytes(n)
        raises(api.E_INVAL, r.enable_burst_track, 16)  # a second call: refused, and nothing changes
        assert r.memory() == m
        r.enable_burst_clock()  # independent of the others: any order
        r.enable_burst_meter()
        r.enable_burst_envelope()
        assert r.memory()["device_bytes"] - m["device_bytes"] == api.FIFO_DEPTH * 64 * (1056 + 320 + 128)
        raises(api.E_STATE, r.read_burst_tracks)  # nothing undrained
        r.submit(x)
        nr, nw = api.C.c_uint32(0), api.C.c_uint64(0)
        buf = np.full(40, 0x55, dtype=np.uint8)  # the caller's room too small: E_INVAL, nothing written, the counts set
        wbuf = np.full(4, 0x55555555, dtype=np.uint32)
        f = r.L.tfrec_amd_read_burst_tracks
        assert f(r.h, buf.ctypes.data, 0, api.C.byref(nr), None, 0, api.C.byref(nw)) == api.E_INVAL and (buf == 0x55).all()
        assert nr.value == 1 and nw.value == (int(runs_plain[0][0]["n_samples"]) + 31) // 32
        assert f(r.h, buf.ctypes.data, 1, api.C.byref(nr), wbuf.ctypes.data, 1, api.C.byref(nw)) == api.E_INVAL
        assert (buf == 0x55).all() and (wbuf == 0x55555555).all()
        assert f(r.h, buf.ctypes.data, 1, None, None, 0, api.C.byref(nw)) == api.E_INVAL
        assert f(r.h, buf.ctypes.data, 1, api.C.byref(nr), None, 0, None) == api.E_INVAL
        assert f(r.h, buf.ctypes.data, 1, api.C.byref(nr), None, 5, api.C.byref(nw)) == api.E_INVAL  # no words, yet room for some
        assert f(r.h, buf.ctypes.data, 1, api.C.byref(nr), None, 0, api.C.byref(nw)) == api.E_OK  # the records alone
        recs, words = r.read_burst_tracks()
        assert buf.tobytes() == recs.tobytes() and len(words) == nw.value
        assert len(recs) == len(runs_plain[0]) == len(r.read_bursts()) == len(r.read_burst_clocks()) == 1
        runs = r.read_captures()
        ev = r.drain()
    R.assert_tables(runs, runs_plain)
    assert parity.sort_events(ev).tobytes() == parity.sort_events(ev_plain).tobytes()


# ---- tfrec_gpu -G
BASE = ["-T", "2f", "-t", "500", "-b", "2"]
WORDS = ("bits", "burst", "extent", "clock")


def test_cli_bits_lines_of_the_golden_tfa_2_scene_cut_into_three_batches(tmp_path):
    parity.build_cli()
    x, want = shifted_tfa_2()
    f = str(tmp_path / "tfa2.iq")
    x.tofile(f)
    want = [ln % f for ln in want]
    assert len(want) == 2 and all(ln.split()[5] == "66" for ln in want)
    plain = cli_lines(BASE + ["-L", f], *WORDS)
    got = cli_lines(["-G", "17240"] + BASE + ["-L", f], *WORDS)
    assert plain["bits"] == [] and got["telegrams"] == plain["telegrams"]  # the telegrams do not notice
    assert got["burst"] == got["extent"] == got["clock"] == []
    assert got["bits"] == want
    f2 = str(tmp_path / "short.iq")  # through a recycled slot beside a second file
    x[:2 * api.BLOCK_BYTES].tofile(f2)
    slot = cli_lines(["-G", "17240", "-n", "1"] + BASE + ["-L", f, "-L", f2], *WORDS)
    assert [ln for ln in slot["bits"] if ln.split()[1] == f] == want
    # beside -M, -Q and -C: all four kinds of line, each what it is alone
    alone = cli_lines(["-M", "-Q", "-C"] + BASE + ["-L", f], *WORDS)
    every = cli_lines(["-M", "-Q", "-C", "-G", "17240,0"] + BASE + ["-L", f], *WORDS)
    assert alone["bits"] == [] and every["bits"] == want and len(alone["burst"]) == len(alone["extent"]) == len(alone["clock"]) == 2
    assert all(every[w] == alone[w] for w in ("burst", "extent", "clock", "telegrams"))
