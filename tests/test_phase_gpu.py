"""The burst track's phase mode on the GPU (tfrec_amd_enable_burst_track_phase, tfrec_gpu -G rate,psk), bit for bit.

The carrier records, the track records and the bitmap's words are compared, byte for byte, with the restatement tfrec_amd/track.py
(head_carriers and phase_tracks) run on the context's OWN decimated samples (tfrec_amd_read_decimated), its own run table and the
thresholds read back from the same submit.  Channel-rate contexts (tfrec_amd_create_decimated) take hand-made decimated samples:
what the kernels can get wrong is placed exactly, and what each run is there for is said in tests/phase_rows.py.  Everything is an
exact integer; nothing here has a tolerance.  Nothing here is measured on real recordings.  Left untested: the enable call's
out-of-memory path."""
import functools

import numpy as np
import pytest

import parity
import phase_rows as P
import recorder as R
from phase_rows import B, CONT, FALLBACK, OPEN
from recorder import cli_lines, hand_receiver, raises, read_phase, same_chains, same_records, zeros
from recorder_rows import CTX_TYPES, golden_iq, quiet, scene
from tfrec_amd import api, burst, decin, sync, track

pytestmark = pytest.mark.gpu

key = lambda c: (int(c["stream"]), int(c["start_sample"]))  # noqa: E731
src = lambda c: (int(c["n_counted"]), int(c["source"]), int(c["centre_hz"]))  # noqa: E731


def phase_receiver(n, nb, L, m, K, cap=None, **kw):
    """A channel-rate context with the recorder (a pool for every pair) and the phase track."""
    r = hand_receiver(n, nb, (), cap=cap or (32 * n, n * nb * B), **kw)
    r.enable_burst_track_phase(L, K, m)
    return r


# ---- hand-made rows on a channel-rate context
@functools.lru_cache(maxsize=None)
def hand_uncut(L, m, K):
    rows = P.hand_rows()
    with phase_receiver(2, 2, L, m, K) as r:
        r.set_burst_track_centre([0, 1], FALLBACK)
        r.submit(np.ascontiguousarray(rows))
        cen, got, words, decs, _ = read_phase(r, 2, [0, 0], L, m, K, FALLBACK, None)
        again = r.read_burst_track_centres()  # reading pops nothing
        assert again.tobytes() == cen.tobytes()
        r.drain()
        raises(api.E_STATE, r.read_burst_track_centres)  # nothing undrained
    assert np.array_equal(np.stack(decs).reshape(2, 2 * B, 2), decin.clamp(rows))
    return cen, got, words


@pytest.mark.parametrize("L,m,K", P.SETS)
def test_two_streams_of_two_blocks_of_hand_made_frames(L, m, K):
    cen, got, words = hand_uncut(L, m, K)
    assert [key(c) for c in cen] == P.HAND_RUNS
    assert (cen["flags"] == got["flags"]).all() and cen[3]["flags"] == OPEN and cen[8]["flags"] == OPEN and cen[8]["n_samples"] == 2
    by = {key(c): c for c in cen}
    if K == 64:  # 63 products at the most: never measured
        assert (cen["source"] == P.F).all() and (cen["n_counted"] <= 63).all()
        assert cen["centre_hz"].tolist() == [FALLBACK[0]] * 4 + [FALLBACK[1]] * 5
    else:
        for s, at, hz, sym in P.FRAMES:  # every frame's carrier is found to the table's step
            assert by[s, at]["source"] == P.M and abs(int(by[s, at]["centre_hz"]) - hz) <= 94, (s, at)
        assert src(by[1, 1000]) == (200, P.F, FALLBACK[1])  # the (0, 0) head
        assert src(by[1, B + 3000]) == (0, P.F, FALLBACK[1]) and src(by[1, 2 * B - 2]) == (0, P.F, FALLBACK[1])
    if (L, m) == (5, P.SPB) and K >= 1024:  # at a symbol's lag the track is the symbol
        for s, at, hz, sym in P.FRAMES:
            g = got[[key(c) for c in cen].index((s, at))]
            t = track.bits_of(g, words)
            assert [int(t[P.SPB * i + L + 1]) for i in range(1, len(sym))] == sym[1:], (s, at)
    s, a, e = P.ZERO_SUMS  # the (0, 0) pairs: every sum there is exactly 0
    t = track.bits_of(got[[key(c) for c in cen].index((1, 2500))], words)
    assert not t[a - 2500 + m + L:e - 2500].any()
    if m > 2:  # the run of 2 samples is shorter than m: no product
        assert got[8]["n_ones"] == 0


@pytest.mark.parametrize("L,m,K", P.SETS)
def test_the_same_rows_in_two_submits_queued_before_the_first_read(L, m, K):
    wcen, whole, wwords = hand_uncut(L, m, K)
    rows = P.hand_rows()
    with phase_receiver(2, 1, L, m, K) as r:
        r.set_burst_track_centre([0, 1], FALLBACK)
        for k in range(2):  # both queued before the first read
            r.submit(np.ascontiguousarray(rows[:, k * B:(k + 1) * B]))
        subs, st = [], None
        for k in range(2):
            part = decin.clamp(rows[:, k * B:(k + 1) * B])
            cen, recs, words, _, st = read_phase(r, 1, [k * B] * 2, L, m, K, FALLBACK, st, decs=[part[s].reshape(-1) for s in range(2)])
            subs.append((cen, recs, words))
            r.drain()
    first, second = subs[0][0], subs[1][0]
    o = {int(c["stream"]): c for c in first if c["flags"] & OPEN}
    c = {int(c["stream"]): c for c in second if c["flags"] & CONT}
    assert o[0]["n_samples"] == 3 and src(o[0]) == (2, P.F, FALLBACK[0])  # 3 samples: the fallback ...
    assert src(c[0]) == (0, P.I, FALLBACK[0]) and c[0]["index"] == o[0]["index"]  # ... which its continuation inherits
    assert o[1]["n_samples"] == 500 and src(c[1]) == (0, P.I, int(o[1]["centre_hz"])) and c[1]["index"] == o[1]["index"]
    if m > 3:  # the 3-sample piece has no product, and the continuation's first m - 3 are 0
        g = subs[0][1][[key(x) for x in first].index((0, B - 3))]
        assert g["n_ones"] == 0
        if L == 1:
            assert not track.bits_of(subs[1][1][0], subs[1][2])[:m - 3].any()
    mcen, mtrk = (sorted(x, key=key) for x in P.chains(subs))
    ucen, utrk = (sorted(x, key=key) for x in P.chains([(wcen, whole, wwords)]))
    assert [key(x) for x in mcen] == [key(x) for x in ucen] and len(mcen) == len(wcen)
    for a, b, ta, tb in zip(mcen, ucen, mtrk, utrk):
        if key(a) in ((0, B - 3), (1, B - 500)):  # the chains that begin within K samples of the cut
            assert (a["flags"], a["n_samples"]) == (b["flags"], b["n_samples"])
        else:  # every other first piece holds its head: the merged result is the uncut one
            assert a.tobytes() == b.tobytes(), key(a)
            same_chains("track", [ta], [tb], "1 + 1")


@pytest.mark.parametrize("n", [65, 97])
def test_stream_counts_across_a_waves_end(n):
    nb, L, m, K = 4, 7, 12, 1024
    kinds = [quiet(nb, 41 + k) for k in range(4)]
    kinds[0][100:2100] = P.psk(P.symbols(200, 1), 60000)
    kinds[0][3 * B - 400:3 * B + 900] = P.psk(P.symbols(130, 2), -30000)  # a head across a block boundary
    kinds[1][:] = P.psk(P.symbols(nb * B // P.SPB + 1, 3), -72000)[:nb * B]  # never leaves its window
    kinds[2][2 * B + 5:2 * B + 70] = (3000, 0)  # 64 products
    kinds[3][500:629] = P.quarter_turns(129)  # 128 products that sum to (0, 0)
    x = np.ascontiguousarray(np.stack(kinds)[np.arange(n) % 4])
    fb = [(0, 6000, -150000)[s % 3] for s in range(n)]
    with phase_receiver(n, nb, L, m, K) as r:
        r.set_burst_track_centre(range(n), fb)
        r.submit(x)
        cen, got, words, decs, st = read_phase(r, nb, [0] * n, L, m, K, fb, None)
        r.drain()
    assert len(cen) == sum((2, 1, 1, 1)[s % 4] for s in range(n))
    for c in cen:
        s = int(c["stream"])
        want = {0: [(1023, P.M, 60000), (1023, P.M, -30000)], 1: [(1023, P.M, -72000)], 2: [(64, P.M, 0)], 3: [(128, P.F, fb[s])]}[s % 4]
        assert any(src(c)[:2] == w[:2] and abs(src(c)[2] - w[2]) <= 94 for w in want), (s, src(c))
    assert [int(i) >= 0 for i in st[1]["index"]] == [s % 4 == 1 for s in range(n)]
    assert st[0]["prior"].tolist() == [80 if s % 4 == 1 else 0 for s in range(n)]


def test_a_fallback_changed_between_two_submits_and_a_reset_mid_chain():
    """A new fallback is in force from the next submit on, for the entries that fall back there; an inherited carrier is not
    touched.  A reset drops the chain: the piece behind it does not continue and is measured as a first piece."""
    rows = P.hand_rows()
    L, m, K = 5, 10, 1024
    with phase_receiver(2, 1, L, m, K) as r:
        raises(api.E_INVAL, r.set_burst_track_centre, [0], [192001])
        raises(api.E_INVAL, r.set_burst_track_centre, [0, 2], [0, 0])  # a stream out of range: nothing is set
        r.submit(np.ascontiguousarray(rows[:, :B]))
        a = read_phase(r, 1, [0, 0], L, m, K, [0, 0], None)  # the refused calls set nothing: fallback 0
        r.drain()
        r.set_burst_track_centre([0, 1], [-30000, 90000])
        r.submit(np.ascontiguousarray(rows[:, B:]))
        b = read_phase(r, 1, [B, B], L, m, K, [-30000, 90000], a[4])
        r.drain()
    assert [src(c)[:2] for c in a[0] if c["flags"] & OPEN] == [(2, P.F), (499, P.M)] and a[0][2]["centre_hz"] == 0
    assert [src(c)[:2] for c in b[0] if c["flags"] & CONT] == [(0, P.I), (0, P.I)] and b[0][0]["centre_hz"] == 0  # the old fallback, inherited
    assert src(b[0][-1]) == (0, P.F, 90000) and src(b[0][-2]) == (0, P.F, 90000)  # the single over samples: the new one
    with phase_receiver(2, 1, L, m, K) as r:
        r.set_burst_track_centre([0, 1], FALLBACK)
        r.submit(np.ascontiguousarray(rows[:, :B]))
        a = read_phase(r, 1, [0, 0], L, m, K, FALLBACK, None)
        r.drain()
        r.reset_streams([1])
        r.submit(np.ascontiguousarray(rows[:, B:]))
        pst, cst = a[4][0], track.fresh_centre_state(2)
        cst["index"][0], cst["centre_hz"][0] = a[4][1]["index"][0], a[4][1]["centre_hz"][0]  # stream 0 goes on
        b = read_phase(r, 1, [B, 0], L, m, K, FALLBACK, (pst, cst))  # a reset stream counts from 0 again
        r.drain()
    b1 = b[0][b[0]["stream"] == 1][0]
    assert not b1["flags"] & CONT and b1["start_sample"] == 0 and src(b1)[:2] == (1023, P.M)  # the frame's other 1500 samples
    assert src(b[0][0]) == (0, P.I, FALLBACK[0])


def test_overflow_on_max_runs_loses_the_inheritance_and_on_max_samples_nothing():
    L, m, K = 5, 10, 1024
    wcen, whole, wwords = hand_uncut(L, m, K)
    rows = np.ascontiguousarray(P.hand_rows())
    with phase_receiver(2, 1, L, m, K, cap=(5, 2 * B)) as r:  # block 0 has 3 + 3 runs: stream 1's OPEN run has no record
        r.set_burst_track_centre([0, 1], FALLBACK)
        r.submit(np.ascontiguousarray(rows[:, :B]))
        raises(api.E_OVERFLOW, r.read_burst_track_centres)
        a = read_phase(r, 1, [0, 0], L, m, K, FALLBACK, None, overflow=True)
        assert r.centre_total == 6 and len(a[0]) == 5 and r.capture_overflow
        r.drain()
        r.submit(np.ascontiguousarray(rows[:, B:]))
        pst, cst = a[4]
        assert cst["index"].tolist() == [track.index_of(FALLBACK[0]), -1] and pst["prior"].tolist() == [3, 0]
        pst["prior"][1] = 80  # (the header's prior is the OPEN piece's, record or not: the restatement saw the table's prefix)
        b = read_phase(r, 1, [B, B], L, m, K, FALLBACK, (pst, cst))
        r.drain()
    assert [src(c) for c in b[0] if c["flags"] & CONT] == [(0, P.I, FALLBACK[0]), (0, P.F, FALLBACK[1])]
    room = int(whole[3]["bit_offset"] + whole[3]["n_samples"])  # the pool holds the first four runs, and not the fifth
    with phase_receiver(2, 2, L, m, K, cap=(32, room + 10)) as r:
        r.set_burst_track_centre([0, 1], FALLBACK)
        r.submit(rows)
        raises(api.E_OVERFLOW, r.read_burst_tracks)
        assert len(r.read_burst_track_centres()) == len(wcen)  # tfrec_amd_read_bursts' rules: the pool does not matter to the records
        cen, got, words, _, _ = read_phase(r, 2, [0, 0], L, m, K, FALLBACK, None, overflow=True)
        same_records(cen, wcen, "every carrier")  # the head is read from the rows, not the pool
        same_records(got, whole, "every record")
        assert len(words) == (room + 31) // 32
        r.drain()


@pytest.mark.parametrize("sizes", [(2,), (1, 1)])
def test_the_sync_on_top(sizes):
    rows = P.hand_rows()
    L, m, K = 5, 10, 1024
    st = sync.Settings(P.RATE, P.WORD, 16, 0)
    tst, sst, pos, ssubs = None, None, 0, []
    with phase_receiver(2, max(sizes), L, m, K) as r:
        r.enable_burst_sync(P.RATE, P.WORD, 16, 0)
        for nb in sizes:
            r.submit(np.ascontiguousarray(rows[:, pos * B:(pos + nb) * B]))
            _, trecs, twords, _, tst = read_phase(r, nb, [pos * B] * 2, L, m, K, [0, 0], tst)
            srecs, swords, sst = R.read_sync(r, st, sst, trecs, twords)
            ssubs.append((srecs, swords))
            pos += nb
            r.drain()
    hits = {key(c): int(c["n_hits"]) for c in sync.chains(ssubs)}
    assert all(hits[k] > 0 for k in ((0, 2000), (1, 2500), (1, B - 500)))  # the frames that hold the word and whose head is whole
    assert hits[0, 0] == 0 and hits[1, 1000] == 0


# ---- the other kinds of context
def test_the_golden_tfa_1_scene_with_every_burst_call_on():
    x = golden_iq("tfa_1")
    rate, m, L, runs, _, n_bits = P.GOLDEN["tfa_1"]
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
        r.enable_burst_track_phase(L, 1024, m)
        r.enable_burst_sync(rate, P.WORD, 16, 0)
        r.enable_burst_clock()
        r.enable_burst_meter()
        r.enable_burst_envelope()
        r.submit(x)
        cen, got, words, decs, _ = read_phase(r, 4, [0], L, m, 1024, [0], None)
        st = sync.Settings(rate, P.WORD, 16, 0)
        srecs, swords, _ = R.read_sync(r, st, None, got, words)
        R.read_clock(r, 4, [0])
        env = R.read_envelope(r, 4, zeros(1), [0])[0]
        bursts = r.read_bursts()
        tab = r.read_captures()
        ev = r.drain()
    assert bursts.tobytes() == burst.bursts(decs, tab[0], zeros(1)).tobytes() and np.array_equal(env["last_over"], got["last_over"])
    R.assert_tables(tab, plain_runs)
    assert parity.sort_events(ev).tobytes() == parity.sort_events(plain).tobytes() and len(ev) >= 1
    assert [P.figures(c) for c in cen] == [(a, n, p, i) for a, n, _, p, i in runs] and (cen["source"] == P.M).all()
    trk = track.chains([(got, words)])
    for t, s, tel, pay in zip(trk, sync.chains([(srecs, swords)]), P.TFA_1_TELEGRAMS, P.TFA_1_PAYLOADS):
        bits = P.sliced(t, rate)
        assert len(bits) == n_bits and bits[P.FROM_BIT:P.FROM_BIT + 88] == P.lsb_first(tel)
        fr = sync.frames(t, s, st, 4)
        assert len(fr) == 1 and track.hex_of(fr[0][3]) == pay


def test_a_submit_runs_replay_gives_the_recordings_carriers_and_track():
    """The golden TFA_1 scene recorded by a u8 context (1 + 3 blocks) and replayed through sparse submits (2 + 2): both bursts lie
    inside blocks, so every first piece holds its head and the merged records and tracks are the recording's."""
    x = golden_iq("tfa_1")
    L, m, K = 5, 10, 1024
    with api.Receiver(1, 0x2F, 500, 0, max_blocks=3, all_flushes=True, levels=True) as r:
        r.enable_capture(256, 4 * B)
        r.enable_capture_pre()
        r.enable_burst_track_phase(L, K, m)
        tabs, recs, pos, st = [], [], 0, None
        for p, nb in zip(parity.cut(x, (1, 3)), (1, 3)):
            r.submit(p)
            tabs.append(r.read_captures(pre=True))
            c, g, w, _, st = read_phase(r, nb, [pos * B], L, m, K, [0], st)
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
        r.enable_burst_track_phase(L, K, m)
        rep, st = [], None
        for k in range(2):
            t, p, q = decin.rebase(runs, pool, pre, 2 * k * B, 2 * B)
            assert r.submit_runs(t, p, q, 2) == 2
            c, g, w, _, st = read_phase(r, 2, [2 * k * B], L, m, K, [0], st, levels=False)
            rep.append((c, g, w))
            r.drain()
    (ac, at), (bc, bt) = P.chains(recs), P.chains(rep)
    assert len(ac) == len(bc) == 2 and [int(c["index"]) for c in ac] == [r[4] for r in P.GOLDEN["tfa_1"][3]]
    assert [c.tobytes() for c in ac] == [c.tobytes() for c in bc]
    same_chains("track", bt, at, "the replay")


def test_the_refusals_the_memory_sums_and_contexts_without_the_call():
    n, mb = 3, 2
    x = scene()[:n, :api.BLOCK_BYTES]
    with api.Receiver(n, CTX_TYPES, 500, 0, max_blocks=mb) as r:
        plain = r.memory()
        raises(api.E_INVAL, r.enable_burst_track_phase, 5, 1024, 10)  # no recorder
        raises(api.E_INVAL, r.read_burst_track_centres)  # not enabled
        assert r.memory() == plain
        r.enable_capture(64, 1024)
        rec = r.memory()
        for bad in ((0, 1024, 10), (17, 1024, 10), (5, 63, 10), (5, 4097, 10), (5, 0, 10), (5, -1, 10), (5, 1024, 0), (5, 1024, 65),
                    (5, 1024, -1), (2 ** 31, 1024, 10), (5, 2 ** 31, 10), (5, 1024, 2 ** 31)):
            raises(api.E_INVAL, r.enable_burst_track_phase, *bad)
        assert r.memory() == rec
        r.submit(x)
        submitted = r.memory()
        raises(api.E_STATE, r.enable_burst_track_phase, 5, 1024, 10)  # after the first submit
        assert r.memory() == submitted
        runs_plain = r.read_captures()
        ev_plain = r.drain()
    mems = {}
    for mode, args in (("enable_burst_track", (16,)), ("enable_burst_track_amplitude", (16,)), ("enable_burst_track_auto", (16, 1024))):
        with api.Receiver(n, CTX_TYPES, 500, 0, max_blocks=mb) as r:  # the three old modes: what they had, and no fourth on top
            r.enable_capture(64, 1024)
            assert r.memory() == rec  # a recorder without the call holds what it held
            getattr(r, mode)(*args)
            mems[mode] = r.memory()
            want = track.auto_device_bytes if mode == "enable_burst_track_auto" else track.device_bytes
            assert mems[mode]["device_bytes"] - rec["device_bytes"] == want(n, 64, 1024)
            raises(api.E_INVAL, r.enable_burst_track_phase, 16, 1024, 10)
            assert "enabled already" in str(pytest.raises(api.TfrecAmdError, r.enable_burst_track_phase, 16, 1024, 10).value)
            assert r.memory() == mems[mode]
            r.submit(x)
            if mode == "enable_burst_track":  # ... and its track is the one it was
                got = R.read_track(r, 1, [0] * n, 16, [0, 0, 0], None, levels=False)[0]
                assert len(got) == len(runs_plain[0])
            R.assert_tables(r.read_captures(), runs_plain)
            assert parity.sort_events(r.drain()).tobytes() == parity.sort_events(ev_plain).tobytes()
    with api.Receiver(n, CTX_TYPES, 500, 0, max_blocks=mb) as r:
        r.enable_capture(64, 1024)
        r.enable_burst_track_phase(16, 4096, 64)
        mem = r.memory()
        assert mem["device_bytes"] - rec["device_bytes"] == track.phase_device_bytes(n, 64, 1024)
        assert mem["device_bytes"] - mems["enable_burst_track_auto"]["device_bytes"] == 4 * 64 * n
        assert mem["pinned_host_bytes"] - rec["pinned_host_bytes"] == track.pinned_bytes(n)
        for again, args in ((r.enable_burst_track_phase, (16, 1024, 10)), (r.enable_burst_track_auto, (16, 1024)), (r.enable_burst_track, (16,)),
                            (r.enable_burst_track_amplitude, (16,))):  # a second call, of any mode
            raises(api.E_INVAL, again, *args)
        raises(api.E_INVAL, r.set_burst_track_level, [0], [100])  # a phase context has no levels
        raises(api.E_INVAL, r.set_burst_track_centre, [0], [-192001])
        raises(api.E_INVAL, r.set_burst_track_centre, [n], [5])
        assert r.memory() == mem
        r.enable_burst_sync(4800, 0x2DD4, 16, 0)  # the sync accepts the mode
        r.enable_burst_meter()
        raises(api.E_STATE, r.read_burst_track_centres)  # nothing undrained
        r.submit(x)
        cen, got, words, _, _ = read_phase(r, 1, [0] * n, 16, 64, 4096, [0] * n, None, levels=False)
        assert len(cen) == len(runs_plain[0]) == len(r.read_bursts()) == len(r.read_burst_syncs()[0]) == 1
        runs = r.read_captures()
        ev = r.drain()
    R.assert_tables(runs, runs_plain)  # the table and the events do not notice
    assert parity.sort_events(ev).tobytes() == parity.sort_events(ev_plain).tobytes()


# ---- tfrec_gpu -G rate,psk
def test_cli_centre_bits_and_frame_lines_of_the_tfa_1_scene_across_a_batch_boundary(tmp_path):
    parity.build_cli()
    x, want = P.cli_scene()
    f = str(tmp_path / "tfa_1.iq")
    x.tofile(f)
    want = [ln % f for ln in want]
    assert [ln.split()[0] for ln in want] == ["centre", "bits", "frame"] * 2
    assert [ln.split()[-1] for ln in want[2::3]] == list(P.TFA_1_PAYLOADS)  # the four bytes behind b42b of both telegrams
    assert want[0].split()[2:5] == ["15504", "4056", "839"] and want[0].split()[-1] == "m"  # 880 samples ahead of the first batch's end, 840 of them over
    base = ["-T", "2f", "-t", "500", "-b", "2"]
    every = ("centre", "bits", "frame")
    got = cli_lines(["-G", "38400,psk", "-Y", "b42b,0,4"] + base + ["-L", f], every)
    assert got[every] == want
    alone = cli_lines(["-G", "38400,psk,10"] + base + ["-L", f], every)  # without -Y, the lag given: the centres and the bits
    assert alone[every] == [ln for ln in want if not ln.startswith("frame ")] and alone["telegrams"] == got["telegrams"]
    fixed = cli_lines(["-G", "38400", "-Y", "b42b,0,4"] + base + ["-L", f], every)  # the frequency track finds no frame in it
    assert not any(ln.startswith(("centre ", "frame ")) for ln in fixed[every])
