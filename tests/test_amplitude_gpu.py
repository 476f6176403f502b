"""The burst track's amplitude mode on the GPU (tfrec_amd_enable_burst_track_amplitude, tfrec_amd_set_burst_track_level,
tfrec_amd_read_burst_tracks, tfrec_gpu -G -O), bit for bit.

The records and the bitmap's words are compared, byte for byte, with the restatement tfrec_amd/track.py (amplitude_tracks) run on
the context's OWN decimated samples (tfrec_amd_read_decimated), its own run table and the thresholds read back from the same submit.
Channel-rate contexts (tfrec_amd_create_decimated) take hand-made decimated samples: the layouts the kernel can get wrong are
placed exactly.  Everything is an exact integer; nothing here has a tolerance.  Nothing here is measured on real recordings."""
import functools

import numpy as np
import pytest

import amplitude_rows as A
import parity
import recorder as R
from amplitude_rows import B, CONT, LEVELS, OPEN, W
from recorder import cli_lines, hand_receiver, raises, read_amp, same_chains, same_records
from recorder_rows import CTX_TYPES, golden_iq, scene
from tfrec_amd import api, decin, sync, track

pytestmark = pytest.mark.gpu


def amp_receiver(n, nb, L, cap=None, **kw):
    """A channel-rate context with the recorder (a pool for every pair) and the amplitude track."""
    r = hand_receiver(n, nb, (), cap=cap or (32 * n, n * nb * B), **kw)
    r.enable_burst_track_amplitude(L)
    return r


key = lambda c: (int(c["stream"]), int(c["start_sample"]))  # noqa: E731


# ---- hand-made rows on a channel-rate context
@functools.lru_cache(maxsize=None)
def hand_uncut(L):
    rows = A.hand_rows()
    with amp_receiver(2, 2, L) as r:
        r.set_burst_track_level([0, 1], LEVELS)
        r.submit(np.ascontiguousarray(rows))
        got, words, decs, _ = read_amp(r, 2, [0, 0], L, LEVELS, None)
        again = r.read_burst_tracks()  # reading pops nothing
        assert again[0].tobytes() == got.tobytes() and again[1].tobytes() == words.tobytes()
        r.drain()
        raises(api.E_STATE, r.read_burst_tracks)  # nothing undrained
    assert np.array_equal(np.stack(decs).reshape(2, 2 * B, 2), decin.clamp(rows))
    return got, words


@pytest.mark.parametrize("L", [1, 5, 16])
def test_two_streams_of_two_blocks_of_hand_made_samples(L):
    got, words = hand_uncut(L)
    by_start = {key(r): r for r in got}
    assert sorted(by_start) == [(0, 0), (0, 2000), (0, B - 3), (0, 2 * B - 1500), (1, 1000), (1, 3001), (1, B - W - 50), (1, B)]
    # the rows hold what they are meant to hold (the values: the restatement's, on the CPU)
    first = by_start[0, 0]
    assert first["flags"] == 0 and (first["n_samples"], first["last_over"], first["bit_offset"]) == (36 + W, 36, 0)
    assert (got["bit_offset"][1:] % 32 != 0).all()  # every later run shares its first word with the run ahead of it
    still = track.bits_of(by_start[0, 2000], words)
    assert not still[:300].any() and still[300:600].all() and not still[600 + L:].any()  # L * level exactly: 0; L more: 1
    across = by_start[0, B - 3]
    assert across["n_samples"] == across["last_over"] + W and 1980 <= across["last_over"] < 2003  # (the tone's last stretch is off)
    assert 900 <= across["n_ones"] <= 1100  # keyed half on, half off
    last0 = by_start[0, 2 * B - 1500]
    assert last0["flags"] == OPEN and (last0["n_samples"], last0["last_over"]) == (1500, 1499)
    assert by_start[1, 1000]["n_samples"] == W and by_start[1, 1000]["n_ones"] == 0
    full = by_start[1, 3001]
    assert full["last_over"] == 39 and track.bits_of(full, words).tolist() == [int(L - 1 <= k < 40) for k in range(full["n_samples"])]
    end = by_start[1, B - W - 50]
    assert end["start_sample"] + end["n_samples"] == B - 1 and end["flags"] == 0  # block 0's last sample is not captured
    assert by_start[1, B]["flags"] == 0 and by_start[1, B]["n_ones"] == 0  # a run from a block's first sample
    if L == 5:  # keyed every 22 samples: the pulses and the gaps between them
        w = track.pulses(track.bits_of(across, words)[:2003])
        assert len(w) == 91 and all(abs(x - 22) <= 1 for x in w[1:-1])


@pytest.mark.parametrize("L", [1, 5, 16])
def test_the_same_rows_in_two_submits_queued_before_the_first_read(L):
    whole, wwords = hand_uncut(L)
    rows = A.hand_rows()
    with amp_receiver(2, 1, L) as r:
        r.set_burst_track_level([0, 1], LEVELS)
        for k in range(2):  # both queued before the first read
            r.submit(np.ascontiguousarray(rows[:, k * B:(k + 1) * B]))
        got, st = [], None
        for k in range(2):
            part = decin.clamp(rows[:, k * B:(k + 1) * B])  # (a channel-rate context's samples are its input, clamped: hand_uncut)
            recs, words, _, st = read_amp(r, 1, [k * B] * 2, L, LEVELS, st, decs=[part[s].reshape(-1) for s in range(2)])
            if k == 0:
                assert st["prior"].tolist() == [3, 0]  # stream 0's chain begins 3 samples ahead of the cut
            got.append((recs, words))
            r.drain()
    c = got[1][0][(got[1][0]["flags"] & CONT) != 0]
    assert c["stream"].tolist() == [0] and c[0]["start_sample"] == B
    o = got[0][0][(got[0][0]["flags"] & OPEN) != 0]
    assert o["stream"].tolist() == [0] and o[0]["n_samples"] == 3
    merged, uncut = sorted(track.chains(got), key=key), sorted(track.chains([(whole, wwords)]), key=key)
    assert len(merged) == len(uncut) == len(whole)
    same_chains("track", merged, uncut, "1 + 1")


def test_a_level_changed_between_two_submits_and_a_reset_mid_chain():
    """Not a restart: the chain continues, and the second piece is formed with the new level.  A reset drops the chain: the piece
    behind it does not continue, and nothing ahead of it is used."""
    rows = A.hand_rows()
    L = 5
    with amp_receiver(2, 1, L) as r:
        raises(api.E_INVAL, r.set_burst_track_level, [0], [65536])
        raises(api.E_INVAL, r.set_burst_track_level, [0, 2], [0, 0])  # a stream out of range: nothing is set
        raises(api.E_INVAL, r.set_burst_track_level, [1, 0], [5000, -1])
        r.set_burst_track_level([], [])
        r.submit(np.ascontiguousarray(rows[:, :B]))
        a, wa, _, st = read_amp(r, 1, [0, 0], L, [0, 0], None)  # the refused calls set nothing: level 0
        r.drain()
        r.set_burst_track_level([0, 1], [4000, 0])
        r.submit(np.ascontiguousarray(rows[:, B:]))
        b, wb, _, st = read_amp(r, 1, [B, B], L, [4000, 0], st)
        r.drain()
    assert b[0]["flags"] & CONT and b[0]["stream"] == 0
    ch = [c for c in track.chains([(a, wa), (b, wb)]) if key(c) == (0, B - 3)]
    assert len(ch) == 1 and ch[0]["n_samples"] == ch[0]["last_over"] + W > 2600
    assert ch[0].bits[:3].tolist() == [1, 1, 1] and not ch[0].bits[3:].any()  # level 0 reads the floor too; 4000 nothing
    with amp_receiver(2, 1, L) as r:
        r.set_burst_track_level([0, 1], LEVELS)
        r.submit(np.ascontiguousarray(rows[:, :B]))
        a, wa, _, st = read_amp(r, 1, [0, 0], L, LEVELS, None)
        r.drain()
        r.reset_streams([0])
        r.submit(np.ascontiguousarray(rows[:, B:]))
        b, wb, _, st = read_amp(r, 1, [0, B], L, LEVELS, st)  # a reset stream counts from 0 again
        r.drain()
    assert st is not None and a[a["stream"] == 0][-1]["flags"] & OPEN
    b0 = b[b["stream"] == 0][0]
    assert not b0["flags"] & CONT and b0["start_sample"] == 0
    assert len(track.chains([(a, wa), (b, wb)], restarts={1: [0]})) == len(a) + len(b)  # nothing was merged across the reset
    # nothing ahead of it counts: three on-samples of 3000 are needed above 5 * 1500, where the chain it was had them behind it
    assert track.bits_of(b0, wb)[:3].tolist() == [0, 0, 1] and hand_uncut(L)[0][2]["start_sample"] == B - 3
    assert track.bits_of(hand_uncut(L)[0][2], hand_uncut(L)[1])[3:6].tolist() == [1, 1, 1]


@pytest.mark.parametrize("n", [65, 97])
def test_stream_counts_across_a_waves_end(n):
    nb, L = 4, 7
    kinds = [A.floor(nb * B, 41, amp=400), A.keyed([10] * (nb * B // 10 + 1), True, 5, on=3000)[:nb * B],
             A.keyed([16] * (nb * B // 16), True, 6, on=9000), A.floor(nb * B, 43)]  # rows 0 .. 2 never leave their window
    kinds[0][0] = (300, 300)  # (... from the first sample on)
    x = np.ascontiguousarray(np.stack(kinds)[np.arange(n) % len(kinds)])
    lv = [(300, 1500, 4500)[s % 3] for s in range(n)]
    with amp_receiver(n, nb, L) as r:
        r.set_burst_track_level(range(n), lv)
        r.submit(x)
        got, words, decs, st = read_amp(r, nb, [0] * n, L, lv, None)
        r.drain()
    assert got["stream"].tolist() == [s for s in range(n) if s % 4 != 3]  # (row 3 is quiet)
    assert (got["n_samples"] == nb * B).all() and (got["flags"] == OPEN).all() and len(words) == len(got) * nb * B // 32
    assert st["prior"].tolist() == [16 if s % 4 != 3 else 0 for s in range(n)]
    for s in (1, 2):  # copies of a row at the same level have the row's track
        same = [track.bits_of(g, words).tobytes() for g in got if g["stream"] % 12 == s]
        assert len(same) >= 5 and len(set(same)) == 1
    assert len({track.bits_of(g, words).tobytes() for g in got if g["stream"] % 4 == 1}) == 3  # ... and at another, another


def test_overflow_on_max_runs_and_on_max_samples_delivers_the_prefixes():
    L = 5
    whole, wwords = hand_uncut(L)
    rows = np.ascontiguousarray(A.hand_rows())
    with amp_receiver(2, 2, L, cap=(len(whole) - 1, 4 * B)) as r:  # the table a run short
        r.set_burst_track_level([0, 1], LEVELS)
        r.submit(rows)
        raises(api.E_OVERFLOW, r.read_burst_tracks)
        got, words, _, _ = read_amp(r, 2, [0, 0], L, LEVELS, None, overflow=True)
        assert r.track_total == len(whole) and r.capture_overflow
        same_records(got, whole[:-1], "the prefix")
        assert len(words) == (int(whole[-1]["bit_offset"]) + 31) // 32  # the pairs of the runs the table holds
        r.drain()
    room = int(whole[3]["bit_offset"] + whole[3]["n_samples"])  # the pool holds the first four runs, and not the fifth
    with amp_receiver(2, 2, L, cap=(32, room + 10)) as r:
        r.set_burst_track_level([0, 1], LEVELS)
        r.submit(rows)
        raises(api.E_OVERFLOW, r.read_burst_tracks)
        got, words, _, _ = read_amp(r, 2, [0, 0], L, LEVELS, None, overflow=True)
        same_records(got, whole, "every record")  # ... n_ones of the runs whose bits did not fit included
        assert len(words) == (room + 31) // 32 and len(r.read_captures(allow_overflow=True)[0]) == 4
        r.drain()


# ---- the sync on top
@pytest.mark.parametrize("sizes", [(2,), (1, 1)])
def test_the_sync_finds_the_nrz_frames_word_in_the_amplitude_track(sizes):
    z = A.nrz_row()
    st = sync.Settings(A.RATE, A.WORD, 16, 0)
    tsubs, ssubs, tst, sst, pos = [], [], None, None, 0
    with amp_receiver(1, max(sizes), A.L_NRZ) as r:
        r.enable_burst_sync(A.RATE, A.WORD, 16, 0)
        r.set_burst_track_level([0], [A.ON // 2])
        for nb in sizes:
            r.submit(np.ascontiguousarray(z[None, pos * B:(pos + nb) * B]))
            trecs, twords, _, tst = read_amp(r, nb, [pos * B], A.L_NRZ, [A.ON // 2], tst)
            srecs, swords, sst = R.read_sync(r, st, sst, trecs, twords)
            tsubs.append((trecs, twords))
            ssubs.append((srecs, swords))
            pos += nb
            r.drain()
    t, s = track.chains(tsubs), sync.chains(ssubs)
    assert len(t) == len(s) == 1 and len(sync.plateaus(s[0].bits)) == 1
    fr = sync.frames(t[0], s[0], st, 4)
    assert len(fr) == 1 and fr[0][1:3] == (0, "+") and track.hex_of(fr[0][3]) == A.PAYLOAD
    assert A.FRAME in track.line("f", t[0], A.RATE)


# ---- the other kinds of context
def test_a_submit_runs_replay_gives_the_recordings_track():
    """The golden TFA_2 scene recorded by a u8 context (1 + 3 blocks) and replayed through sparse submits (2 + 2): a run's samples
    are the recording's and nothing ahead of a chain is used, so the merged records and tracks are the recording's."""
    x = golden_iq()
    L, lv = 11, [2000]
    with api.Receiver(1, 0x2F, 500, 0, max_blocks=3, all_flushes=True, levels=True) as r:
        r.enable_capture(256, 4 * B)
        r.enable_capture_pre()
        r.enable_burst_track_amplitude(L)
        r.set_burst_track_level([0], lv)
        tabs, recs, pos, st = [], [], 0, None
        for p, nb in zip(parity.cut(x, (1, 3)), (1, 3)):
            r.submit(p)
            tabs.append(r.read_captures(pre=True))
            g, w, _, st = read_amp(r, nb, [pos * B], L, lv, st)
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
        r.enable_burst_track_amplitude(L)
        r.set_burst_track_level([0], lv)
        rep, st = [], None
        for k in range(2):
            t, p, q = decin.rebase(runs, pool, pre, 2 * k * B, 2 * B)
            assert r.submit_runs(t, p, q, 2) == 2
            g, w, _, st = read_amp(r, 2, [2 * k * B], L, lv, st, levels=False)
            rep.append((g, w))
            r.drain()
    a, b = track.chains(recs), track.chains(rep)
    assert len(a) == len(b) == 2 and all(0 < int(c["n_ones"]) < int(c["n_samples"]) for c in a)
    same_chains("track", b, a, "the replay")


def test_the_refusals_the_memory_sums_and_a_context_without_the_call():
    n, mb = 3, 2
    x = scene()[:n, :api.BLOCK_BYTES]
    with api.Receiver(n, CTX_TYPES, 500, 0, max_blocks=mb) as r:
        plain = r.memory()
        raises(api.E_INVAL, r.enable_burst_track_amplitude, 5)  # no recorder
        raises(api.E_INVAL, r.set_burst_track_level, [0], [0])  # not enabled
        assert r.memory() == plain
        r.enable_capture(64, 1024)
        rec = r.memory()
        raises(api.E_INVAL, r.set_burst_track_level, [0], [0])  # the recorder alone: no track
        for bad in (0, 17, -1, 2 ** 31):
            raises(api.E_INVAL, r.enable_burst_track_amplitude, bad)
        assert r.memory() == rec
        r.submit(x)
        submitted = r.memory()  # (a host submit's staging is counted)
        raises(api.E_STATE, r.enable_burst_track_amplitude, 5)  # after the first submit
        assert r.memory() == submitted
        runs_plain = r.read_captures()
        ev_plain = r.drain()
    with api.Receiver(n, CTX_TYPES, 500, 0, max_blocks=mb) as r:  # the frequency mode: no levels, no second mode
        r.enable_capture(64, 1024)
        assert r.memory() == rec  # a recorder without the call holds what it held
        r.enable_burst_track(16)
        freq = r.memory()
        raises(api.E_INVAL, r.enable_burst_track_amplitude, 16)
        raises(api.E_INVAL, r.set_burst_track_level, [0], [100])
        assert "enabled already" in str(pytest.raises(api.TfrecAmdError, r.enable_burst_track_amplitude, 16).value)
        assert r.memory() == freq
        r.set_burst_track_centre([0], [1000])  # ... and what it had works as it did
    with api.Receiver(n, CTX_TYPES, 500, 0, max_blocks=mb) as r:
        r.enable_capture(64, 1024)
        r.enable_burst_track_amplitude(16)
        m = r.memory()
        assert m == freq  # the memory sums are equal in both modes
        assert m["device_bytes"] - rec["device_bytes"] == track.device_bytes(n, 64, 1024)
        assert m["pinned_host_bytes"] - rec["pinned_host_bytes"] == track.pinned_bytes(n)
        raises(api.E_INVAL, r.enable_burst_track_amplitude, 16)  # a second call, of either mode: refused, and nothing changes
        raises(api.E_INVAL, r.enable_burst_track, 16)
        assert "enabled already" in str(pytest.raises(api.TfrecAmdError, r.enable_burst_track, 16).value)
        raises(api.E_INVAL, r.set_burst_track_centre, [0], [0])  # an amplitude context has no centres
        raises(api.E_INVAL, r.set_burst_track_level, [0], [65536])
        raises(api.E_INVAL, r.set_burst_track_level, [0], [-1])
        raises(api.E_INVAL, r.set_burst_track_level, [n], [5])
        raises(api.E_INVAL, r.set_burst_track_level, [0], [2 ** 31])
        assert r.L.tfrec_amd_set_burst_track_level(r.h, None, None, 1) == api.E_INVAL
        assert r.L.tfrec_amd_set_burst_track_level(r.h, None, None, -1) == api.E_INVAL
        assert r.memory() == m
        r.enable_burst_sync(4800, 0x2DD4, 16, 0)  # the sync accepts either mode
        r.enable_burst_meter()  # independent of the others: any order
        raises(api.E_STATE, r.read_burst_tracks)  # nothing undrained
        r.submit(x)
        got, words, _, _ = read_amp(r, 1, [0] * n, 16, [0] * n, None, levels=False)  # the refused calls set nothing: level 0
        assert len(got) == len(runs_plain[0]) == len(r.read_bursts()) == len(r.read_burst_syncs()[0]) == 1
        runs = r.read_captures()
        ev = r.drain()
    R.assert_tables(runs, runs_plain)  # the table and the events do not notice
    assert parity.sort_events(ev).tobytes() == parity.sort_events(ev_plain).tobytes()


# ---- a short fixed-seed random set
@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_generated_rows_and_cuts(seed):
    rows, lv, L, sizes = A.generated(seed)
    n, nb = rows.shape[0], rows.shape[1] // B
    whole = None
    for cut in ((nb,), sizes):
        subs, st, pos = [], None, 0
        with amp_receiver(n, max(cut), L) as r:
            r.set_burst_track_level(range(n), lv)
            for m in cut:
                r.submit(np.ascontiguousarray(rows[:, pos * B:(pos + m) * B]))
                recs, words, _, st = read_amp(r, m, [pos * B] * n, L, lv, st)
                subs.append((recs, words))
                pos += m
                r.drain()
        ch = sorted(track.chains(subs), key=key)
        assert len(ch) >= n
        if whole is None:
            whole = ch
        else:
            same_chains("track", ch, whole, "cut %s" % (cut,))


# ---- tfrec_gpu -G -O
def test_cli_bits_pulses_and_frame_lines_of_an_ook_burst_across_a_batch_boundary(tmp_path):
    parity.build_cli()
    x, level, want = A.cli_scene()
    f = str(tmp_path / "ook.iq")
    x.tofile(f)
    want = [ln % f for ln in want]
    assert [ln.split()[0] for ln in want] == ["bits", "pulses", "frame"] and A.FRAME in want[0] and want[2].endswith(" 32 " + A.PAYLOAD)
    base = ["-T", "2f", "-t", "500", "-b", "2"]
    every = ("bits", "pulses", "frame")
    got = cli_lines(["-G", str(A.RATE), "-O", str(level), "-Y", "2dd4,0,4"] + base + ["-L", f], every)
    assert got[every] == want
    alone = cli_lines(["-O", str(level), "-G", str(A.RATE)] + base + ["-L", f], every)  # without -Y: the bits and the pulses
    assert alone[every] == want[:2] and alone["telegrams"] == got["telegrams"]
    fsk = cli_lines(["-G", str(A.RATE)] + base + ["-L", f], every)  # without -O: -G's frequency track, no pulses line
    assert [ln.split()[0] for ln in fsk[every]] == ["bits"]
