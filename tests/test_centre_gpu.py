"""The burst track's auto-centre mode on the GPU (tfrec_amd_enable_burst_track_auto, tfrec_amd_read_burst_track_centres, tfrec_gpu
-G rate,auto), bit for bit.

The centre records, the track records and the bitmap's words are compared, byte for byte, with the restatement tfrec_amd/track.py
(head_centres and tracks about every entry's index: auto_tracks) run on the context's OWN decimated samples
(tfrec_amd_read_decimated), its own run table and the thresholds read back from the same submit.  Channel-rate contexts
(tfrec_amd_create_decimated) take hand-made decimated samples: what the kernels can get wrong is placed exactly, and what each run
must give is reasoned in tests/centre_rows.py.  Everything is an exact integer; nothing here has a tolerance.  Nothing here is
measured on real recordings.  Left untested: the enable call's out-of-memory path."""
import functools

import numpy as np
import pytest

import centre_rows as C
import parity
import recorder as R
from centre_rows import B, CONT, FALLBACK, OPEN
from recorder import cli_lines, hand_receiver, raises, read_auto, same_chains, same_records, zeros
from recorder_rows import CTX_TYPES, RATE, TELEGRAMS, golden_iq, scene
from tfrec_amd import api, burst, decin, sync, track

pytestmark = pytest.mark.gpu

key = lambda c: (int(c["stream"]), int(c["start_sample"]))  # noqa: E731
figures = lambda c: (int(c["n_counted"]), int(c["source"]), int(c["centre_hz"]), int(c["deviation_hz"]))  # noqa: E731


def auto_receiver(n, nb, L, K, cap=None, **kw):
    """A channel-rate context with the recorder (a pool for every pair) and the auto-centre track."""
    r = hand_receiver(n, nb, (), cap=cap or (32 * n, n * nb * B), **kw)
    r.enable_burst_track_auto(L, K)
    return r


# ---- hand-made rows on a channel-rate context
@functools.lru_cache(maxsize=None)
def hand_uncut(L, K):
    rows = C.hand_rows()
    with auto_receiver(2, 2, L, K) as r:
        r.set_burst_track_centre([0, 1], FALLBACK)
        r.submit(np.ascontiguousarray(rows))
        cen, got, words, decs, _ = read_auto(r, 2, [0, 0], L, K, FALLBACK, None)
        again = r.read_burst_track_centres()  # reading pops nothing
        assert again.tobytes() == cen.tobytes()
        r.drain()
        raises(api.E_STATE, r.read_burst_track_centres)  # nothing undrained
    assert np.array_equal(np.stack(decs).reshape(2, 2 * B, 2), decin.clamp(rows))
    return cen, got, words


@pytest.mark.parametrize("K", [64, 1024, 4096])
@pytest.mark.parametrize("L", [1, 5, 16])
def test_two_streams_of_two_blocks_of_hand_made_fsk(L, K):
    cen, got, words = hand_uncut(L, K)
    assert [key(c) for c in cen] == sorted(C.HAND_1024)
    assert (cen["flags"] == got["flags"]).all() and cen[4]["flags"] == OPEN
    if K == 64:  # 63 products at the most: never measured
        assert (cen["source"] == C.F).all() and cen["n_counted"].tolist() == [63] * 5 + [63, 63, 63, 63, 63, 63, 0]
        assert cen["centre_hz"].tolist() == [FALLBACK[0]] * 5 + [FALLBACK[1]] * 7
    if K == 1024:  # what centre_rows reasons for every run
        assert {key(c): figures(c) for c in cen} == C.HAND_1024
    if K == 4096:  # the whole burst, where it is shorter than that: the same centres
        assert [figures(c)[1:] for c in cen] == [C.HAND_1024[key(c)][1:] for c in cen]
        assert cen["n_counted"].tolist() == [299, 1499, 1499, 1202, 1499, 63, 64, 160, 160, 994, 1999, 0]
    if K >= 1024 and L == 5:  # about its own centre every FSK burst reads its alternating first symbols, 40 samples each
        for c, g in zip(cen, got):
            if int(c["deviation_hz"]) == 30000:
                t = track.bits_of(g, words)
                assert [int(t[20 + 40 * k]) for k in range(6)] == [0, 1, 0, 1, 0, 1], key(c)


@pytest.mark.parametrize("L,K", [(1, 1024), (5, 1024), (16, 1024), (5, 64), (5, 4096)])
def test_the_same_rows_in_two_submits_queued_before_the_first_read(L, K):
    wcen, whole, wwords = hand_uncut(L, K)
    rows = C.hand_rows()
    with auto_receiver(2, 1, L, K) as r:
        r.set_burst_track_centre([0, 1], FALLBACK)
        for k in range(2):  # both queued before the first read
            r.submit(np.ascontiguousarray(rows[:, k * B:(k + 1) * B]))
        subs, st = [], None
        for k in range(2):
            part = decin.clamp(rows[:, k * B:(k + 1) * B])
            cen, recs, words, _, st = read_auto(r, 1, [k * B] * 2, L, K, FALLBACK, st, decs=[part[s].reshape(-1) for s in range(2)])
            subs.append((cen, recs, words))
            r.drain()
    first, second = subs[0][0], subs[1][0]
    o = {int(c["stream"]): c for c in first if c["flags"] & OPEN}
    c = {int(c["stream"]): c for c in second if c["flags"] & CONT}
    assert o[0]["n_samples"] == 3 and figures(o[0]) == (2, C.F, FALLBACK[0], 0)  # 3 samples: the fallback ...
    assert figures(c[0]) == (0, C.I, FALLBACK[0], 0) and c[0]["index"] == o[0]["index"]  # ... which its continuation inherits
    assert o[1]["n_samples"] == 500 and figures(c[1]) == (0, C.I, int(o[1]["centre_hz"]), 0)
    if K >= 1024:  # centred on the 500 samples the first piece has
        assert figures(o[1]) == (499, C.M, 48000, 30000)
    mcen, mtrk = (sorted(x, key=key) for x in C.chains(subs))
    ucen, utrk = (sorted(x, key=key) for x in C.chains([(wcen, whole, wwords)]))
    assert [key(x) for x in mcen] == [key(x) for x in ucen] and len(mcen) == len(wcen)
    for a, b, ta, tb in zip(mcen, ucen, mtrk, utrk):
        if key(a) in ((0, B - 3), (1, B - 500)):  # the chains that begin within K samples of the cut
            assert (a["flags"], a["n_samples"]) == (b["flags"], b["n_samples"])
            if key(a) == (1, B - 500) and K >= 1024:  # the same centre from fewer samples: the same track
                assert a["index"] == b["index"]
                same_chains("track", [ta], [tb], "the 500-sample first piece")
        else:  # every other first piece holds its head: the merged result is the uncut one
            assert a.tobytes() == b.tobytes(), key(a)
            same_chains("track", [ta], [tb], "1 + 1")


@pytest.mark.parametrize("n", [65, 97])
def test_stream_counts_across_a_waves_end(n):
    nb, L, K = 4, 7, 1024
    kinds = [C.floor(nb * B, 41), C.floor(nb * B, 42), C.floor(nb * B, 43), C.floor(nb * B, 44)]
    kinds[0][100:2100] = C.fsk(2000, 60000, seed=1)
    kinds[0][3 * B - 400:3 * B + 900] = C.fsk(1300, -30000, seed=2)  # a head across a block boundary
    kinds[1][:] = C.fsk(nb * B, -72000, seed=3)  # never leaves its window
    kinds[2][2 * B + 5:2 * B + 70] = C.tone([24000] * 65)
    kinds[3][500:629] = C.tone(np.concatenate([[0], np.repeat(np.arange(-16, 16) * 6000, 4)]))  # 4 products in each of 32 bins: none occupied
    x = np.ascontiguousarray(np.stack(kinds)[np.arange(n) % 4])
    fb = [(0, 6000, -150000)[s % 3] for s in range(n)]
    with auto_receiver(n, nb, L, K) as r:
        r.set_burst_track_centre(range(n), fb)
        r.submit(x)
        cen, got, words, decs, st = read_auto(r, nb, [0] * n, L, K, fb, None)
        r.drain()
    assert len(cen) == sum((2, 1, 1, 1)[s % 4] for s in range(n))
    for c in cen:
        want = {0: [(1023, C.M, 60000, 30000), (1023, C.M, -30000, 30000)], 1: [(1023, C.M, -72000, 30000)], 2: [(64, C.M, 24000, 0)],
                3: [(128, C.F, fb[int(c["stream"])], 0)]}
        assert figures(c) in want[int(c["stream"]) % 4]
    assert st[1]["index"].tolist() == [track.index_of(-72000) if s % 4 == 1 else -1 for s in range(n)]


def test_a_fallback_changed_between_two_submits_and_a_reset_mid_chain():
    """A new fallback is in force from the next submit on, for the entries that fall back there; an inherited centre is not
    touched.  A reset drops the chain: the piece behind it does not continue and is measured as a first piece."""
    rows = C.hand_rows()
    L, K = 5, 1024
    with auto_receiver(2, 1, L, K) as r:
        raises(api.E_INVAL, r.set_burst_track_centre, [0], [192001])
        raises(api.E_INVAL, r.set_burst_track_centre, [0, 2], [0, 0])  # a stream out of range: nothing is set
        r.submit(np.ascontiguousarray(rows[:, :B]))
        a = read_auto(r, 1, [0, 0], L, K, [0, 0], None)  # the refused calls set nothing: fallback 0
        r.drain()
        r.set_burst_track_centre([0, 1], [-30000, 90000])
        r.submit(np.ascontiguousarray(rows[:, B:]))
        b = read_auto(r, 1, [B, B], L, K, [-30000, 90000], a[4])
        r.drain()
    assert [figures(c) for c in a[0] if c["flags"] & OPEN] == [(2, C.F, 0, 0), (499, C.M, 48000, 30000)]
    assert [figures(c) for c in b[0] if c["flags"] & CONT] == [(0, C.I, 0, 0), (0, C.I, 48000, 0)]  # the old fallback, inherited
    assert figures(b[0][-1]) == (0, C.F, 90000, 0)  # the one over sample: the new one
    with auto_receiver(2, 1, L, K) as r:
        r.set_burst_track_centre([0, 1], FALLBACK)
        r.submit(np.ascontiguousarray(rows[:, :B]))
        a = read_auto(r, 1, [0, 0], L, K, FALLBACK, None)
        r.drain()
        r.reset_streams([1])
        r.submit(np.ascontiguousarray(rows[:, B:]))
        st = (a[4][0], track.fresh_centre_state(2))
        st[1]["index"][0], st[1]["centre_hz"][0] = a[4][1]["index"][0], a[4][1]["centre_hz"][0]  # stream 0 goes on
        b = read_auto(r, 1, [B, 0], L, K, FALLBACK, st)  # a reset stream counts from 0 again
        r.drain()
    b1 = b[0][b[0]["stream"] == 1][0]
    assert not b1["flags"] & CONT and b1["start_sample"] == 0 and figures(b1) == (1023, C.M, 48000, 30000)  # the burst's other 1500
    assert figures(b[0][0]) == (0, C.I, FALLBACK[0], 0)


def test_overflow_on_max_runs_loses_the_inheritance_and_on_max_samples_nothing():
    L, K = 5, 1024
    wcen, whole, wwords = hand_uncut(L, K)
    rows = np.ascontiguousarray(C.hand_rows())
    with auto_receiver(2, 1, L, K, cap=(9, 2 * B)) as r:  # block 0 has 4 + 6 runs: stream 1's OPEN run has no record
        r.set_burst_track_centre([0, 1], FALLBACK)
        r.submit(np.ascontiguousarray(rows[:, :B]))
        raises(api.E_OVERFLOW, r.read_burst_track_centres)
        a = read_auto(r, 1, [0, 0], L, K, FALLBACK, None, overflow=True)
        assert r.centre_total == 10 and len(a[0]) == 9 and r.capture_overflow
        r.drain()
        r.submit(np.ascontiguousarray(rows[:, B:]))
        st = a[4]
        assert st[1]["index"].tolist() == [track.index_of(FALLBACK[0]), -1] and st[0]["prior"].tolist() == [3, 0]
        st[0]["prior"][1] = 16  # (the header's prior is the OPEN piece's, record or not: the restatement saw the table's prefix)
        b = read_auto(r, 1, [B, B], L, K, FALLBACK, st)
        r.drain()
    assert [figures(c) for c in b[0] if c["flags"] & CONT] == [(0, C.I, FALLBACK[0], 0), (0, C.F, FALLBACK[1], 0)]
    room = int(whole[3]["bit_offset"] + whole[3]["n_samples"])  # the pool holds the first four runs, and not the fifth
    with auto_receiver(2, 2, L, K, cap=(32, room + 10)) as r:
        r.set_burst_track_centre([0, 1], FALLBACK)
        r.submit(rows)
        raises(api.E_OVERFLOW, r.read_burst_tracks)
        assert len(r.read_burst_track_centres()) == len(wcen)  # tfrec_amd_read_bursts' rules: the pool does not matter to the records
        cen, got, words, _, _ = read_auto(r, 2, [0, 0], L, K, FALLBACK, None, overflow=True)
        same_records(cen, wcen, "every centre")  # the head is read from the rows, not the pool
        same_records(got, whole, "every record")
        assert len(words) == (room + 31) // 32
        r.drain()


@pytest.mark.parametrize("sizes", [(2,), (1, 1)])
def test_the_sync_on_top(sizes):
    rows = C.hand_rows()
    L, K = 16, 1024
    st = sync.Settings(9600, 0x5555, 16, 1, True)
    tst, sst, pos, ssubs = None, None, 0, []
    with auto_receiver(2, max(sizes), L, K) as r:
        r.enable_burst_sync(9600, 0x5555, 16, 1, True)
        for nb in sizes:
            r.submit(np.ascontiguousarray(rows[:, pos * B:(pos + nb) * B]))
            _, trecs, twords, _, tst = read_auto(r, nb, [pos * B] * 2, L, K, [0, 0], tst)
            srecs, swords, sst = R.read_sync(r, st, sst, trecs, twords)
            ssubs.append((srecs, swords))
            pos += nb
            r.drain()
    hits = {key(c): int(c["n_hits"]) for c in sync.chains(ssubs)}
    assert all(hits[k] > 0 for k in ((0, 2000), (0, 5000), (1, B - 500)))  # the alternating symbols at the bursts' heads


# ---- the other kinds of context
def test_the_golden_tfa_2_scene_with_every_burst_call_on():
    x = golden_iq()
    with api.Receiver(1, 0x2F, 500, 0, max_blocks=4, all_flushes=True) as r:
        r.submit(x)
        plain = r.drain()
    with api.Receiver(1, 0x2F, 500, 0, max_blocks=4, all_flushes=True, levels=True) as r:
        r.enable_capture(256, 4 * B)
        r.submit(x)
        plain_runs = r.read_captures()
        r.drain()
    with api.Receiver(1, 0x2F, 500, 0, max_blocks=4, all_flushes=True, levels=True) as r:
        r.enable_capture(256, 4 * B)
        r.enable_burst_track_auto(11, 1024)
        r.enable_burst_sync(17240, 0x2DD4, 16, 0)
        r.enable_burst_clock()
        r.enable_burst_meter()
        r.enable_burst_envelope()
        r.submit(x)
        cen, got, words, decs, _ = read_auto(r, 4, [0], 11, 1024, [0], None)
        R.read_sync(r, sync.Settings(17240, 0x2DD4, 16, 0), None, got, words)
        R.read_clock(r, 4, [0])
        env = R.read_envelope(r, 4, zeros(1), [0])[0]
        bursts = r.read_bursts()
        tab = r.read_captures()
        ev = r.drain()
    assert bursts.tobytes() == burst.bursts(decs, tab[0], zeros(1)).tobytes() and np.array_equal(env["last_over"], got["last_over"])
    R.assert_tables(tab, plain_runs)
    assert parity.sort_events(ev).tobytes() == parity.sort_events(plain).tobytes() and len(ev) >= 1
    assert [figures(c) for c in cen] == [(1023, C.M) + f for f in C.FIGURES["tfa_2", 0]]
    for c, tel in zip(track.chains([(got, words)]), TELEGRAMS["tfa_2"]):
        assert C.reads(c, RATE["tfa_2"], tel)


def test_a_submit_runs_replay_gives_the_recordings_centres_and_track():
    """The golden TFA_2 scene recorded by a u8 context (1 + 3 blocks) and replayed through sparse submits (2 + 2): both bursts lie
    inside blocks, so every first piece holds its head and the merged records and tracks are the recording's."""
    x = golden_iq()
    L, K = 11, 1024
    with api.Receiver(1, 0x2F, 500, 0, max_blocks=3, all_flushes=True, levels=True) as r:
        r.enable_capture(256, 4 * B)
        r.enable_capture_pre()
        r.enable_burst_track_auto(L, K)
        tabs, recs, pos, st = [], [], 0, None
        for p, nb in zip(parity.cut(x, (1, 3)), (1, 3)):
            r.submit(p)
            tabs.append(r.read_captures(pre=True))
            c, g, w, _, st = read_auto(r, nb, [pos * B], L, K, [0], st)
            recs.append((c, g, w))
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
        r.enable_burst_track_auto(L, K)
        rep, st = [], None
        for k in range(2):
            t, p, q = decin.rebase(runs, pool, pre, 2 * k * B, 2 * B)
            assert r.submit_runs(t, p, q, 2) == 2
            c, g, w, _, st = read_auto(r, 2, [2 * k * B], L, K, [0], st, levels=False)
            rep.append((c, g, w))
            r.drain()
    (ac, at), (bc, bt) = C.chains(recs), C.chains(rep)
    assert len(ac) == len(bc) == 2 and [figures(c)[2:] for c in ac] == list(C.FIGURES["tfa_2", 0])
    assert [c.tobytes() for c in ac] == [c.tobytes() for c in bc]
    same_chains("track", bt, at, "the replay")


def test_the_refusals_the_memory_sums_and_contexts_without_the_call():
    n, mb = 3, 2
    x = scene()[:n, :api.BLOCK_BYTES]
    with api.Receiver(n, CTX_TYPES, 500, 0, max_blocks=mb) as r:
        plain = r.memory()
        raises(api.E_INVAL, r.enable_burst_track_auto, 5, 1024)  # no recorder
        raises(api.E_INVAL, r.read_burst_track_centres)  # not enabled
        assert r.memory() == plain
        r.enable_capture(64, 1024)
        rec = r.memory()
        for bad in ((0, 1024), (17, 1024), (5, 63), (5, 4097), (5, 0), (5, -1), (2 ** 31, 1024), (5, 2 ** 31)):
            raises(api.E_INVAL, r.enable_burst_track_auto, *bad)
        assert r.memory() == rec
        r.submit(x)
        submitted = r.memory()
        raises(api.E_STATE, r.enable_burst_track_auto, 5, 1024)  # after the first submit
        assert r.memory() == submitted
        runs_plain = r.read_captures()
        ev_plain = r.drain()
    mems = {}
    for mode in ("enable_burst_track", "enable_burst_track_amplitude"):  # the two old modes: what they had, and no third on top
        with api.Receiver(n, CTX_TYPES, 500, 0, max_blocks=mb) as r:
            r.enable_capture(64, 1024)
            assert r.memory() == rec  # a recorder without the call holds what it held
            getattr(r, mode)(16)
            mems[mode] = r.memory()
            assert mems[mode]["device_bytes"] - rec["device_bytes"] == track.device_bytes(n, 64, 1024)
            raises(api.E_INVAL, r.enable_burst_track_auto, 16, 1024)
            assert "enabled already" in str(pytest.raises(api.TfrecAmdError, r.enable_burst_track_auto, 16, 1024).value)
            raises(api.E_INVAL, r.read_burst_track_centres)  # no centre records in another mode
            assert r.memory() == mems[mode]
            (r.set_burst_track_centre if mode == "enable_burst_track" else r.set_burst_track_level)([0], [1000])
            r.submit(x)
            if mode == "enable_burst_track":  # ... and its track is the one it was: the set centre's index
                got = R.read_track(r, 1, [0] * n, 16, [1000, 0, 0], None, levels=False)[0]
                assert len(got) == len(runs_plain[0])
            R.assert_tables(r.read_captures(), runs_plain)
            assert parity.sort_events(r.drain()).tobytes() == parity.sort_events(ev_plain).tobytes()
    with api.Receiver(n, CTX_TYPES, 500, 0, max_blocks=mb) as r:
        r.enable_capture(64, 1024)
        r.enable_burst_track_auto(16, 4096)
        m = r.memory()
        assert m["device_bytes"] - rec["device_bytes"] == track.auto_device_bytes(n, 64, 1024)
        assert m["device_bytes"] - mems["enable_burst_track"]["device_bytes"] == api.FIFO_DEPTH * 64 * 48 + 8 * n
        assert m["pinned_host_bytes"] - rec["pinned_host_bytes"] == track.pinned_bytes(n)
        for again in (r.enable_burst_track_auto, r.enable_burst_track, r.enable_burst_track_amplitude):  # a second call, of any mode
            raises(api.E_INVAL, again, *((16, 1024) if again == r.enable_burst_track_auto else (16,)))
        raises(api.E_INVAL, r.set_burst_track_level, [0], [100])  # an auto-centre context has no levels
        raises(api.E_INVAL, r.set_burst_track_centre, [0], [-192001])
        raises(api.E_INVAL, r.set_burst_track_centre, [n], [5])
        assert r.L.tfrec_amd_read_burst_track_centres(r.h, None, 0, None) == api.E_INVAL
        assert r.memory() == m
        r.enable_burst_sync(4800, 0x2DD4, 16, 0)  # the sync accepts the mode
        r.enable_burst_meter()
        raises(api.E_STATE, r.read_burst_track_centres)  # nothing undrained
        r.submit(x)
        cen, got, words, _, _ = read_auto(r, 1, [0] * n, 16, 4096, [0] * n, None, levels=False)
        assert len(cen) == len(runs_plain[0]) == len(r.read_bursts()) == len(r.read_burst_syncs()[0]) == 1
        runs = r.read_captures()
        ev = r.drain()
    R.assert_tables(runs, runs_plain)  # the table and the events do not notice
    assert parity.sort_events(ev).tobytes() == parity.sort_events(ev_plain).tobytes()


# ---- tfrec_gpu -G rate,auto
def test_cli_centre_bits_and_frame_lines_of_the_mixed_tfa_2_scene_across_batch_boundaries(tmp_path):
    parity.build_cli()
    x, want = C.cli_scene()
    f = str(tmp_path / "mixed.iq")
    x.tofile(f)
    want = [ln % f for ln in want]
    assert [ln.split()[0] for ln in want] == ["centre", "bits", "frame"] * 2
    assert [ln.split()[-1] for ln in want[2::3]] == ["96070960", "98812225"]  # both telegrams' first bytes, +40 kHz and -40 kHz
    assert want[0].split()[4:] == ["880", "39000", "33000", "m"]  # the first burst begins 881 samples ahead of the first batch's end
    base = ["-T", "2f", "-t", "500", "-b", "2"]
    every = ("centre", "bits", "frame")
    got = cli_lines(["-G", "17240,auto", "-Y", "2dd4,0,4"] + base + ["-L", f], every)
    assert got[every] == want
    alone = cli_lines(["-G", "17240,auto"] + base + ["-L", f], every)  # without -Y: the centres and the bits
    assert alone[every] == [ln for ln in want if not ln.startswith("frame ")] and alone["telegrams"] == got["telegrams"]
    for centre in (-40000, 0, 40000):  # no single centre reads both
        fixed = cli_lines(["-G", "17240,%d" % centre, "-Y", "2dd4,0,4"] + base + ["-L", f], every)
        assert not any(ln.startswith("centre ") for ln in fixed[every])
        assert len([ln for ln in fixed[every] if ln.startswith("frame ") and ln.split()[-1] in ("96070960", "98812225")]) <= 1
