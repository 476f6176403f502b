"""The line code on the GPU (tfrec_amd_enable_burst_code, tfrec_amd_read_burst_codes, tfrec_gpu -G -U), bit for bit.

The coded records and the coded bitmap's words are compared, byte for byte, with the restatement tfrec_amd/linecode.py run on the
context's OWN track records and words (tfrec_amd_read_burst_tracks) of the same submit -- so everything ahead of the code is
whatever the context runs --, and the sync's records and words with tfrec_amd/sync.py FED THE CODED TRACK the context returned.
Channel-rate contexts take hand-made rows: tests/phase_rows.py's phase-keyed frames on the phase track and their FSK sibling
(tests/linecode_rows.py) on the frequency track; what each run is there for is said there.  Everything is an exact integer;
nothing here has a tolerance.  Nothing here is measured on real recordings.  Left untested: the enable call's out-of-memory path."""
import functools

import numpy as np
import pytest

import linecode_rows as LR
import parity
import phase_rows as P
import recorder as R
from linecode_rows import B, CONT, OPEN
from recorder import cli_lines, hand_receiver, raises, same_chains, same_records, same_words
from recorder_rows import CTX_TYPES, frame_symbols, fsk, golden_iq, quiet, scene
from tfrec_amd import api, decin, linecode, sync, track

pytestmark = pytest.mark.gpu

ST = sync.Settings(17240, LR.WORD, 16, 3, True)  # the sync on top in the hand-made cases: loose enough to match in noise-like bits
ROWS = {"psk": (P.hand_rows, ("phase", 1024, 10), 5, P.FALLBACK), "fsk": (LR.fsk_rows, None, 11, [0, 0])}  # rows, mode, L, centres
key = lambda c: (int(c["stream"]), int(c["start_sample"]))  # noqa: E731


def read_code(r, cs, state, st=None, sstate=None, overflow=False):
    """The oldest undrained submit's coded records and words against the restatement on the track records and words the context
    returned for it, and with `st` the sync's against sync.syncs on those coded ones -> ((track records, words), (coded records,
    words), the code's state behind the submit, (sync records, words) or None, the sync's state)."""
    r.read_captures(allow_overflow=True)
    trecs, twords = r.read_burst_tracks(allow_overflow=overflow)
    got, words = r.read_burst_codes(allow_overflow=overflow)
    assert got.dtype == track.TRACK_DTYPE and r.code_total == r.track_total, "code: dtype %s, totals %d and %d" % (got.dtype, r.code_total, r.track_total)
    want, wwords, state = linecode.codes(trecs, twords, cs, state, r.n_streams, max_samples=r._capture[1])
    same_records(got, want, "code")
    same_words(words, wwords, "code")
    ssub = None
    if st is not None:
        srecs, swords, sstate = R.read_sync(r, st, sstate, got, words, overflow=overflow)
        ssub = (srecs, swords)
    return (trecs, twords), (got, words), state, ssub, sstate


def run_cut(rows, mode, L, centres, cs, sizes, st=ST, cap=None, resets=None, sync_first=False):
    """The rows in submits of `sizes` blocks, all queued before the first read (unless a reset comes between them); every
    submit's code and sync checked -> [(track records, words)], [(coded records, words)], [(sync records, words)]."""
    n = len(rows)
    parts, pos = [], 0
    for nb in sizes:
        parts.append(np.ascontiguousarray(rows[:, pos * B:(pos + nb) * B]))
        pos += nb
    tsubs, csubs, ssubs = [], [], []
    with hand_receiver(n, max(sizes), (), cap=cap or (32 * n, n * max(sizes) * B)) as r:
        R.enable_mode(r, mode, L)
        if st is not None and sync_first:  # the order of the two enables does not matter: the pointer is chosen per submit
            r.enable_burst_sync(st.rate, st.pattern, st.P, st.E, st.both)
        r.enable_burst_code(cs.rate, cs.taps, cs.invert)
        if st is not None and not sync_first:
            r.enable_burst_sync(st.rate, st.pattern, st.P, st.E, st.both)
        if mode is None or mode[0] != "amplitude":
            r.set_burst_track_centre(range(n), centres)
        if not resets:
            for x in parts:
                r.submit(x)
        cstate = sstate = None
        for i, x in enumerate(parts):
            if resets:
                if i in resets:
                    r.reset_streams(resets[i])
                r.submit(x)
            t, c, cstate, s, sstate = read_code(r, cs, cstate, st, sstate, overflow=cap is not None)
            if i == 0:
                again = r.read_burst_codes(allow_overflow=cap is not None)  # reading pops nothing
                assert again[0].tobytes() == c[0].tobytes() and again[1].tobytes() == c[1].tobytes()
            tsubs.append(t)
            csubs.append(c)
            ssubs.append(s)
            r.drain()
        raises(api.E_STATE, r.read_burst_codes)  # nothing undrained
    return tsubs, csubs, ssubs


@functools.lru_cache(maxsize=None)
def hand_uncut(kind, name):
    rows, mode, L, centres = ROWS[kind]
    return run_cut(rows(), mode, L, centres, LR.settings(name), (2,), sync_first=name == "nrzs")


def merged(subs):
    return sorted(linecode.chains(subs), key=key)


def alone(rec, words, cs):
    """A record's coded track as a chain's first piece would have it: nothing ahead of it."""
    one = rec.copy().reshape(1)
    one["flags"] &= ~np.uint32(CONT)
    r, w, _ = linecode.codes(one, words, cs)
    return track.bits_of(r[0], w)


# ---- hand-made rows on a channel-rate context
@pytest.mark.parametrize("name", list(LR.SETS))
@pytest.mark.parametrize("kind", list(ROWS))
def test_two_streams_of_two_blocks(kind, name):
    cs = LR.settings(name)
    tsubs, csubs, ssubs = hand_uncut(kind, name)
    (trecs, twords), (got, words) = tsubs[0], csubs[0]
    assert got[0]["stream"] == 0 and got[0]["start_sample"] == 0  # a run at submit index 0
    assert (got["bit_offset"][1:] % 32 != 0).any()  # runs that share a bitmap word
    assert any(r["start_sample"] < B < r["start_sample"] + r["n_samples"] for r in got)  # a run across the block boundary
    last = got[(got["stream"] == 1) & (got["start_sample"] == 2 * B - 2)]  # a run shorter than the smallest delta, open at the last sample
    assert len(last) == 1 and last[0]["flags"] == OPEN and last[0]["n_samples"] == 2 < cs.delta[0]
    assert np.array_equal(track.bits_of(last[0], words), track.bits_of(last[0], twords) ^ (1 if cs.invert else 0))
    assert (got[got["stream"] == 0][-1]["flags"] & OPEN) and got[got["stream"] == 0][-1]["start_sample"] + got[got["stream"] == 0][-1]["n_samples"] == 2 * B
    assert np.array_equal(got["last_over"], trecs["last_over"]) and not np.array_equal(words, twords)
    assert [int(r["n_ones"]) for r in got] == [int(track.bits_of(r, words).sum()) for r in got] and got["n_ones"].sum() > 500
    if name == "span2047":
        assert cs.span == 2047
    if name == "nrzs":  # the complement of nrzi's, bit for bit within the runs
        other = hand_uncut(kind, "nrzi")[1][0]
        for a, b in zip(got, other[0]):
            assert np.array_equal(track.bits_of(a, words), 1 - track.bits_of(b, other[1]))


@pytest.mark.parametrize("name", list(LR.SETS))
@pytest.mark.parametrize("kind", list(ROWS))
def test_the_same_rows_in_two_submits_queued_before_the_first_read(kind, name):
    cs = LR.settings(name)
    rows, mode, L, centres = ROWS[kind]
    whole = hand_uncut(kind, name)
    tsubs, csubs, ssubs = run_cut(rows(), mode, L, centres, cs, (1, 1))
    o = {int(r["stream"]): r for r in csubs[0][0] if r["flags"] & OPEN}
    c = {int(r["stream"]): r for r in csubs[1][0] if r["flags"] & CONT}
    assert (o[0]["n_samples"], o[1]["n_samples"]) == (3, 500) and sorted(c) == [0, 1]  # runs of 3 and 500 samples at a submit's end, continued
    # the piece behind the 500 samples needs the carried bits: alone it reads differently (the 3 samples' bits may all be 0)
    assert not np.array_equal(track.bits_of(c[1], csubs[1][1]), alone(c[1], tsubs[1][1], cs))
    if kind == "fsk":  # the frequency track does not depend on the cut: the merged chains are the uncut run's, the sync's on top too
        same_chains("track", merged(csubs), merged(whole[1]), "1 + 1")
        skey = lambda x: sorted(sync.chains(x), key=key)  # noqa: E731
        same_chains("sync", skey(ssubs), skey(whole[2]), "1 + 1")
    else:  # the phase track's chains that begin within K samples of the cut are read about what their first piece has
        got, want = merged(csubs), merged(whole[1])
        assert [key(x) for x in got] == [key(x) for x in want]
        for a, b in zip(got, want):
            if key(a) not in ((0, B - 3), (1, B - 500)):
                same_chains("track", [a], [b], "1 + 1")


def test_a_chain_of_three_pieces():
    """1000 (1500) samples, a whole block and the rest: the second cut's history comes from a piece that itself began with carried
    bits."""
    cs = LR.settings("g3ruh")
    tsubs, csubs, ssubs = run_cut(LR.long_rows(), None, 11, [0, 0], cs, (1, 1, 1))
    assert [int(r["n_samples"]) for recs, _ in csubs for r in recs if r["stream"] == 0] == [1000, B, 3000 + R.W - 1]
    for k in (1, 2):
        for rec in csubs[k][0]:
            assert rec["flags"] & CONT and not np.array_equal(track.bits_of(rec, csubs[k][1])[:cs.span], alone(rec, tsubs[k][1], cs)[:cs.span])
    whole = run_cut(LR.long_rows(), None, 11, [0, 0], cs, (3,))
    assert len(merged(csubs)) == 2
    same_chains("track", merged(csubs), merged(whole[1]), "1 + 1 + 1")
    same_chains("sync", sorted(sync.chains(ssubs), key=key), sorted(sync.chains(whole[2]), key=key), "1 + 1 + 1")


def test_a_reset_mid_chain_drops_the_history():
    cs = LR.settings("g3ruh")
    tsubs, csubs, _ = run_cut(LR.long_rows(), None, 11, [0, 0], cs, (1, 1, 1), resets={1: [1]})
    r1 = csubs[1][0]
    zero, one = r1[r1["stream"] == 0][0], r1[r1["stream"] == 1][0]
    assert zero["flags"] & CONT and not one["flags"] & CONT and one["start_sample"] < 16  # a reset stream counts from 0 again
    assert np.array_equal(track.bits_of(one, csubs[1][1]), alone(one, tsubs[1][1], cs))
    assert not np.array_equal(track.bits_of(zero, csubs[1][1]), alone(zero, tsubs[1][1], cs))


@pytest.mark.parametrize("n", [65, 97])
def test_stream_counts_across_a_waves_end(n):
    nb = 4
    cs = linecode.Settings(17240, 0x10801, True)  # three windows, and the complement
    rng = np.random.default_rng(43)
    symbols = sum((frame_symbols(LR.WORD, 16, 100 + k, pre=4, pay=9, invert=k % 3 == 1) for k in range(70)), [])
    kinds = [rng.integers(-400, 401, size=(nb * B, 2)).astype(np.int16), fsk(symbols, 17240)[:nb * B], fsk(symbols[5:], 17240, amp=3000)[:nb * B],
             quiet(nb, 44)]  # rows 0 .. 2 never leave their window
    kinds[0][0] = (300, 300)  # (... from the first sample on)
    x = np.ascontiguousarray(np.stack(kinds)[np.arange(n) % len(kinds)])
    if n == 65:  # the same rows again in a second submit: every run CONTINUES
        x = np.concatenate([x, x], axis=1)
    tsubs, csubs, ssubs = run_cut(x, None, 11, [0] * n, cs, (nb, nb) if n == 65 else (nb,))
    got, words = csubs[-1]
    assert got["stream"].tolist() == [s for s in range(n) if s % 4 != 3] and (got["n_samples"] == nb * B).all()
    for s in (1, 2):  # copies of a row have the row's coded track
        same = [track.bits_of(g, words).tobytes() for g in got if g["stream"] % 4 == s]
        assert len(same) >= 16 and len(set(same)) == 1
    if n == 65:
        assert (got["flags"] == CONT | OPEN).all() and (csubs[0][0]["flags"] == OPEN).all()
        first, fw = csubs[0]  # the same rows, but the second submit's first span bits have their history (and its first 16 track bits)
        assert any(not np.array_equal(track.bits_of(a, words)[:cs.span], track.bits_of(b, fw)[:cs.span]) for a, b in zip(got, first))
        assert all(np.array_equal(track.bits_of(a, words)[cs.span + 16:], track.bits_of(b, fw)[cs.span + 16:]) for a, b in zip(got, first))


def test_overflow_on_max_runs_and_on_max_samples_delivers_the_prefixes():
    cs = LR.settings("g3ruh")
    rows, mode, L, centres = ROWS["fsk"]
    rows = rows()
    whole = hand_uncut("fsk", "g3ruh")[1][0][0]
    tsubs, csubs, _ = run_cut(rows, mode, L, centres, cs, (2,), cap=(len(whole) - 1, 4 * B))  # the table a run short
    same_records(csubs[0][0], whole[:-1], "the prefix")
    assert len(csubs[0][1]) == (int(whole[-1]["bit_offset"]) + 31) // 32
    with hand_receiver(2, 2, (), cap=(len(whole) - 1, 4 * B)) as r:
        r.enable_burst_track(L)
        r.enable_burst_code(cs.rate, cs.taps)
        r.submit(np.ascontiguousarray(rows))
        raises(api.E_OVERFLOW, r.read_burst_codes)
        r.drain()
    full = run_cut(rows, mode, L, centres, cs, (1, 1))
    # (1, 1) submits with a table one run short of the first submit: its last run, stream 1's OPEN piece, has no record and leaves no
    # history -- the piece that continues it reads as a chain's first; stream 0's continues as ever
    n0 = len(full[1][0][0])
    tsubs, csubs, _ = run_cut(rows, mode, L, centres, cs, (1, 1), cap=(n0 - 1, 4 * B))
    same_records(csubs[0][0], full[1][0][0][:-1], "the runs that have a record")
    b, wb = csubs[1]
    c, fc = b[(b["flags"] & CONT) != 0], full[1][1][0][(full[1][1][0]["flags"] & CONT) != 0]
    assert c["stream"].tolist() == [0, 1] and np.array_equal(track.bits_of(c[0], wb), track.bits_of(fc[0], full[1][1][1]))
    assert np.array_equal(track.bits_of(c[1], wb), alone(c[1], tsubs[1][1], cs))
    assert not np.array_equal(track.bits_of(fc[1], full[1][1][1]), alone(c[1], tsubs[1][1], cs))
    # ... and with a pool one pair short of the first submit: the same run does not fit, has no bits and leaves no history
    room = int(full[1][0][0]["n_samples"].sum()) - 1
    tsubs, csubs, _ = run_cut(rows, mode, L, centres, cs, (1, 1), cap=(32, room))
    a, wa = csubs[0]
    same_records(a[:-1], full[1][0][0][:-1], "the runs that fit")
    assert a[-1]["stream"] == 1 and a[-1]["flags"] & OPEN and a[-1]["n_ones"] == 0 and a[-1]["last_over"] == full[1][0][0][-1]["last_over"]
    assert full[1][0][0][-1]["n_ones"] > 0 and len(wa) == (int(a[-1]["bit_offset"]) + 31) // 32
    b, wb = csubs[1]  # (the second submit is smaller: everything fits)
    c = b[(b["flags"] & CONT) != 0]
    assert c["stream"].tolist() == [0, 1] and c[0].tobytes() == fc[0].tobytes()
    assert np.array_equal(track.bits_of(c[1], wb), alone(c[1], tsubs[1][1], cs))


def test_a_piece_that_continues_behind_a_run_that_did_not_fit_reads_no_stale_history():
    """Three submits of a block with a pool one pair short of the second: stream 1's whole-block piece does not fit and leaves
    H = 0, while the words the stream carried still hold the first piece's bits -- the third piece reads none of them."""
    cs = LR.settings("g3ruh")
    tsubs, csubs, _ = run_cut(LR.long_rows(), None, 11, [0, 0], cs, (1, 1, 1), cap=(32, 2 * B - 1))
    mid = csubs[1][0]
    assert mid["stream"].tolist() == [0, 1] and mid[0]["n_ones"] > 0 and mid[1]["n_ones"] == 0 and (mid["n_samples"] == B).all()
    assert csubs[0][0][1]["n_samples"] == 1500 and csubs[0][0][1]["n_ones"] > 0  # (what the stream carried into the second submit)
    last, wl = csubs[2]
    assert (last["flags"] & CONT).all()
    assert np.array_equal(track.bits_of(last[1], wl), alone(last[1], tsubs[2][1], cs))
    assert not np.array_equal(track.bits_of(last[0], wl), alone(last[0], tsubs[2][1], cs))


def test_a_context_with_the_sync_but_without_the_code_is_what_it_was():
    """The track and the sync of a context without the call, against their restatements and against the track of one with it."""
    rows, mode, L, centres = ROWS["fsk"]
    rows = rows()
    with hand_receiver(2, 2, {"track": (L,), "sync": (ST.rate, ST.pattern, ST.P, ST.E, ST.both)}) as r:
        mem = r.memory()
        r.submit(np.ascontiguousarray(rows))
        part = decin.clamp(rows)
        trecs, twords, _, _ = R.read_track(r, 2, [0, 0], L, [0, 0], None, decs=[part[s].reshape(-1) for s in range(2)])
        srecs, swords, _ = R.read_sync(r, ST, None, trecs, twords)  # fed the raw track
        raises(api.E_INVAL, r.read_burst_codes)
        r.drain()
    with hand_receiver(2, 2, {"track": (L,), "sync": (ST.rate, ST.pattern, ST.P, ST.E, ST.both)}) as r:
        cs = LR.settings("g3ruh")
        r.enable_burst_code(cs.rate, cs.taps)
        m2 = r.memory()
        assert m2["device_bytes"] - mem["device_bytes"] == linecode.device_bytes(2, 64, 4 * B) and m2["pinned_host_bytes"] == mem["pinned_host_bytes"]
    t2, c2, s2 = hand_uncut("fsk", "g3ruh")
    assert t2[0][0].tobytes() == trecs.tobytes() and t2[0][1].tobytes() == twords.tobytes()
    assert s2[0][0].tobytes() != srecs.tobytes()  # with the code on the sync reads the coded track


# ---- the other kinds of context
def test_the_golden_whb_scene_with_the_phase_track_the_code_and_the_sync():
    x = golden_iq("whb", 6)
    cs, st = linecode.g3ruh(6000), sync.Settings(6000, LR.WORD, 16, 0)
    with api.Receiver(1, 0x2F, 500, 0, max_blocks=6, all_flushes=True) as r:
        plain_mem = r.memory()
        r.submit(x)
        plain = r.drain()
    with api.Receiver(1, 0x2F, 500, 0, max_blocks=6, all_flushes=True, levels=True) as r:
        r.enable_capture(256, 6 * B)
        r.enable_burst_track_phase(16, 1024, 64)
        trk_mem = r.memory()
        r.submit(x)
        plain_runs = r.read_captures()
        plain_track = r.read_burst_tracks()
        plain_cen = r.read_burst_track_centres()
        r.drain()
    with api.Receiver(1, 0x2F, 500, 0, max_blocks=6, all_flushes=True, levels=True) as r:
        r.enable_capture(256, 6 * B)
        r.enable_burst_track_phase(16, 1024, 64)
        assert r.memory() == trk_mem  # a track without the call holds what it held
        r.enable_burst_code(cs.rate, cs.taps, cs.invert)
        m = r.memory()
        assert m["device_bytes"] - trk_mem["device_bytes"] == linecode.device_bytes(1, 256, 6 * B)
        assert m["pinned_host_bytes"] - trk_mem["pinned_host_bytes"] == linecode.pinned_bytes(1)
        r.enable_burst_sync(st.rate, st.pattern, st.P, st.E)
        r.submit(x)
        (trecs, twords), (got, words), _, (srecs, swords), _ = read_code(r, cs, None, st)
        cen = r.read_burst_track_centres()
        tab = r.read_captures()
        ev = r.drain()
    with api.Receiver(1, 0x2F, 500, 0, max_blocks=6, all_flushes=True) as r:
        assert r.memory() == plain_mem  # a context without the call holds what it held
    assert trecs.tobytes() == plain_track[0].tobytes() and twords.tobytes() == plain_track[1].tobytes() and cen.tobytes() == plain_cen.tobytes()
    R.assert_tables(tab, plain_runs)
    assert parity.sort_events(ev).tobytes() == parity.sort_events(plain).tobytes() and len(ev) >= 1
    assert len(got) == 1 and int(got[0]["n_ones"]) == LR.WHB_N_ONES and int(got[0]["last_over"]) == 27650
    cch, sch = linecode.chains([(got, words)]), sync.chains([(srecs, swords)])
    assert [sync.plateaus(s.bits) for s in sch] == [[LR.WHB_PLATEAU]]
    lines = [sync.line("f", s, f) for t, s in zip(cch, sch) for f in sync.frames(t, s, st, 26, lsb=True)]
    assert lines == ["frame f 10004 24316 0 + 208 " + LR.WHB_FRAME]  # the one frame and its 26 bytes
    assert len(track.slice_bits(cch[0].bits[:27651], 6000)) == LR.WHB_SLICED


def test_a_submit_runs_replay_gives_the_recordings_code():
    """The golden WHB scene recorded by a u8 context (1 + 5 blocks) and replayed through sparse submits (3 + 3)."""
    x = golden_iq("whb", 6)
    cs, st = linecode.g3ruh(6000), sync.Settings(6000, LR.WORD, 16, 0)

    def on(r):
        r.enable_burst_track_phase(16, 1024, 64)
        r.enable_burst_code(cs.rate, cs.taps)
        r.enable_burst_sync(st.rate, st.pattern, st.P, st.E)

    with api.Receiver(1, 0x2F, 500, 0, max_blocks=5, all_flushes=True, levels=True) as r:
        r.enable_capture(256, 6 * B)
        r.enable_capture_pre()
        on(r)
        tabs, recs, srec, cst, sst = [], [], [], None, None
        for p in parity.cut(x, (1, 5)):
            r.submit(p)
            tabs.append(r.read_captures(pre=True))
            _, c, cst, s, sst = read_code(r, cs, cst, st, sst)
            recs.append(c)
            srec.append(s)
            r.drain()
    off = 0
    for t, pool, _ in tabs:
        t["pool_offset"] += off
        off += len(pool)
    runs, pool, pre = (np.concatenate([t[i] for t in tabs]) for i in range(3))
    assert len(runs) == 1  # the scene's one burst
    with api.Receiver(1, 0x2F, 500, 0, max_blocks=3, all_flushes=True, decimated=True) as r:
        r.enable_runs_input(len(runs) + 2, len(pool) + 1)
        r.enable_capture(256, 3 * B)
        on(r)
        rep, srep, cst, sst = [], [], None, None
        for k in range(2):
            t, p, q = decin.rebase(runs, pool, pre, 3 * k * B, 3 * B)
            assert r.submit_runs(t, p, q, 3) == 3
            _, c, cst, s, sst = read_code(r, cs, cst, st, sst)
            rep.append(c)
            srep.append(s)
            r.drain()
    a, b = linecode.chains(recs), linecode.chains(rep)
    assert len(a) == len(b) == 1 and any(rec["flags"] & CONT for cr, _ in rep for rec in cr)  # the replay cuts the burst
    same_chains("track", b, a, "the replay")
    same_chains("sync", sync.chains(srep), sync.chains(srec), "the replay")
    assert sync.plateaus(sync.chains(srep)[0].bits) == [LR.WHB_PLATEAU]


def test_the_refusals():
    x = scene()[:3, :api.BLOCK_BYTES]
    with api.Receiver(3, CTX_TYPES, 500, 0, max_blocks=2) as r:
        raises(api.E_INVAL, r.enable_burst_code, 6000, 1)  # no recorder, no track
        raises(api.E_INVAL, r.read_burst_codes)
        r.enable_capture(64, 1024)
        raises(api.E_INVAL, r.enable_burst_code, 6000, 1)  # the recorder alone: no track
        r.enable_burst_track(11)
        m = r.memory()
        for bad in ((999, 1), (96001, 1), (6000, 0), (6001, 1 << 31), (2250, 1 << 11), (2 ** 31, 1), (6000, 1 << 32), (6000, -1)):
            raises(api.E_INVAL, r.enable_burst_code, *bad)
        assert r.L.tfrec_amd_enable_burst_code(r.h, 6000, 1, 2) == api.E_INVAL  # an unknown flag
        assert r.memory() == m  # nothing was allocated
        raises(api.E_INVAL, r.read_burst_codes)  # not enabled
        r.enable_burst_code(6002, (1 << 31) | 1, True)  # span 2047
        m2 = r.memory()
        assert m2["device_bytes"] - m["device_bytes"] == linecode.device_bytes(3, 64, 1024) and m2["pinned_host_bytes"] == m["pinned_host_bytes"]
        raises(api.E_INVAL, r.enable_burst_code, 6000, 1)  # a second call: refused, and nothing changes
        assert r.memory() == m2
        raises(api.E_STATE, r.read_burst_codes)  # nothing undrained
        r.enable_burst_sync(17240, 0x2DD4, 16)  # behind the code
        r.submit(x)
        nr, nw = api.C.c_uint32(0), api.C.c_uint64(0)
        buf = np.full(40, 0x55, dtype=np.uint8)  # the caller's room too small: E_INVAL, nothing written, the counts set
        f = r.L.tfrec_amd_read_burst_codes
        assert f(r.h, buf.ctypes.data, 0, api.C.byref(nr), None, 0, api.C.byref(nw)) == api.E_INVAL and (buf == 0x55).all()
        trecs, twords = r.read_burst_tracks()
        assert nr.value == len(trecs) == len(r.read_captures()[0]) == 1 and nw.value == len(twords)
        assert f(r.h, buf.ctypes.data, 1, api.C.byref(nr), None, 5, api.C.byref(nw)) == api.E_INVAL  # no words, yet room for some
        assert f(r.h, buf.ctypes.data, 1, api.C.byref(nr), None, 0, api.C.byref(nw)) == api.E_OK  # the records alone
        _, (got, words), _, _, _ = read_code(r, linecode.Settings(6002, (1 << 31) | 1, True), None, sync.Settings(17240, 0x2DD4, 16))
        assert buf.tobytes() == got.tobytes()
        r.drain()
    with api.Receiver(3, CTX_TYPES, 500, 0, max_blocks=2) as r:
        r.enable_capture(64, 1024)
        r.enable_burst_track(11)
        r.submit(x)
        raises(api.E_STATE, r.enable_burst_code, 6000, 1)  # after the first submit
        r.drain()


# ---- tfrec_gpu -G -U -Y
def test_cli_lines_of_the_golden_whb_scene_with_the_sync_word_across_a_batch_boundary(tmp_path):
    parity.build_cli()
    x, want = LR.cli_scene()
    f = str(tmp_path / "whb.iq")
    x.tofile(f)
    want = [ln % f for ln in want]
    kinds = ("centre", "bits", "code", "frame")  # every kind of line, in the order they were printed
    base = ["-T", "2f", "-t", "500", "-b", "2", "-L", f]
    got = cli_lines(["-G", "6000,psk", "-U", "g3ruh", "-Y", "b42b,0,26,0,1"] + base, kinds, "frame")
    assert got[kinds] == want and [ln.split()[0] for ln in want] == ["centre", "bits", "code", "frame"]
    assert got["frame"][0].split()[3:] == [str(19004 + 14312), "0", "+", "208", LR.WHB_FRAME]
    # without -Y the code line alone; without -U every other line is what it was, and the raw track has no such frame
    plain = cli_lines(["-G", "6000,psk", "-U", "g3ruh"] + base, kinds)
    assert plain[kinds] == want[:3] and plain["telegrams"] == got["telegrams"]
    raw = cli_lines(["-G", "6000,psk", "-Y", "b42b,0,26,0,1"] + base, kinds)
    assert raw[kinds] == want[:2] and raw["telegrams"] == got["telegrams"]
