"""The frame check on the GPU (tfrec_amd_enable_burst_crc, tfrec_amd_read_burst_crcs, tfrec_gpu -G -Y -V), bit for bit.

The check records and the check bitmap's words are compared, byte for byte, with the restatement tfrec_amd/crc.py run on the
context's OWN input records and words of the same submit -- tfrec_amd_read_burst_codes' where the line code is on, else
tfrec_amd_read_burst_tracks' --, so everything ahead of the check is whatever the context runs.  Channel-rate contexts take
hand-made rows: tests/phase_rows.py's phase-keyed frames, tests/linecode_rows.py's FSK ones and tests/crc_rows.py's, in which frames
that carry their CRC are planted; what each run is there for is said there.  Everything is an exact integer; nothing here has a
tolerance.  Nothing here is measured on real recordings.  Left untested: the enable call's out-of-memory path."""
import functools

import numpy as np
import pytest

import crc_rows as CR
import linecode_rows as LR
import parity
import phase_rows as P
import recorder as R
import recorder_rows as RR
from linecode_rows import B, CONT, OPEN
from recorder import cli_lines, hand_receiver, raises, same_records, same_words
from recorder_rows import CTX_TYPES, fsk, golden_iq, quiet, scene
from tfrec_amd import api, crc, decin, linecode, sync, track

pytestmark = pytest.mark.gpu

SST = sync.Settings(17240, LR.WORD, 16, 3, True)  # the sync beside the check in the hand-made cases
# rows, the track's mode, L, the centres
ROWS = {"psk": (P.hand_rows, ("phase", 1024, 10), 5, P.FALLBACK), "fsk": (LR.fsk_rows, None, 11, [0, 0]), "long": (LR.long_rows, None, 11, [0, 0])}
key = lambda c: (int(c["stream"]), int(c["start_sample"]))  # noqa: E731
FIELDS = [f for f in crc.CRC_DTYPE.names if f != "bit_offset"]


def read_crc(r, vs, state, code=None, overflow=False):
    """The oldest undrained submit's check records and words against the restatement on the input records and words the context
    returned for it -> ((input records, words), (check records, words), the check's state behind the submit)."""
    r.read_captures(allow_overflow=True)
    trecs, twords = (r.read_burst_codes if code else r.read_burst_tracks)(allow_overflow=overflow)
    got, words = r.read_burst_crcs(allow_overflow=overflow)
    assert got.dtype == crc.CRC_DTYPE and r.crc_total == (r.code_total if code else r.track_total), "crc: dtype %s, total %d" % (got.dtype, r.crc_total)
    want, wwords, state = crc.crcs(trecs, twords, vs, state, r.n_streams, max_samples=r._capture[1])
    same_records(got, want, "crc")
    same_words(words, wwords, "crc")
    return (trecs, twords), (got, words), state


def run_cut(rows, mode, L, centres, vs, sizes, code=None, sst=None, cap=None, resets=None, crc_first=False):
    """The rows in submits of `sizes` blocks, all queued before the first read (unless a reset comes between them); every
    submit's check compared -> [(input records, words)], [(check records, words)]."""
    n = len(rows)
    parts, pos = [], 0
    for nb in sizes:
        parts.append(np.ascontiguousarray(rows[:, pos * B:(pos + nb) * B]))
        pos += nb
    tsubs, vsubs = [], []
    with hand_receiver(n, max(sizes), (), cap=cap or (32 * n, n * max(sizes) * B)) as r:
        R.enable_mode(r, mode, L)
        on = lambda: r.enable_burst_crc(vs.rate, vs.N, vs.W, vs.poly, vs.init, vs.xorout, vs.S, vs.lsb, vs.invert)  # noqa: E731
        if crc_first:  # the order of the enables does not matter: the input is chosen per submit
            on()
        if code is not None:
            r.enable_burst_code(code.rate, code.taps, code.invert)
        if sst is not None:
            r.enable_burst_sync(sst.rate, sst.pattern, sst.P, sst.E, sst.both)
        if not crc_first:
            on()
        if mode is None or mode[0] != "amplitude":
            r.set_burst_track_centre(range(n), centres)
        if not resets:
            for x in parts:
                r.submit(x)
        state = sstate = None
        for i, x in enumerate(parts):
            if resets:
                if i in resets:
                    r.reset_streams(resets[i])
                r.submit(x)
            t, v, state = read_crc(r, vs, state, code, overflow=cap is not None)
            if sst is not None:  # the sync beside it is what it is without the check
                _, _, sstate = R.read_sync(r, sst, sstate, t[0], t[1], overflow=cap is not None)
            if i == 0:
                again = r.read_burst_crcs(allow_overflow=cap is not None)  # reading pops nothing
                assert again[0].tobytes() == v[0].tobytes() and again[1].tobytes() == v[1].tobytes()
            tsubs.append(t)
            vsubs.append(v)
            r.drain()
        raises(api.E_STATE, r.read_burst_crcs)  # nothing undrained
    return tsubs, vsubs


@functools.lru_cache(maxsize=None)
def uncut(kind, name, coded=False):
    rows, mode, L, centres = ROWS[kind]
    rows = rows()
    return run_cut(rows, mode, L, centres, CR.settings(name), (rows.shape[1] // B,), code=linecode.nrzi(38400) if coded else None,
                   sst=SST if name in ("crc8", "ccitt") else None, crc_first=name == "ccitt")


def merged(subs):
    return sorted(crc.chains(subs), key=key)


def same_chains(got, want, label):
    assert [key(x) for x in got] == [key(x) for x in want], label
    for a, b in zip(got, want):
        assert [int(a[f]) for f in FIELDS] == [int(b[f]) for f in FIELDS] and np.array_equal(a.bits, b.bits), (label, key(a))


def alone(rec, words, vs):
    """A record's check track as a chain's first piece would have it: nothing ahead of it."""
    one = rec.copy().reshape(1)
    one["flags"] &= ~np.uint32(CONT)
    r, w, _ = crc.crcs(one, words, vs)
    return crc.bits_of(r[0], w)


# ---- hand-made rows on a channel-rate context
@pytest.mark.parametrize("name", list(CR.SETS))
@pytest.mark.parametrize("kind", ["psk", "fsk", "long"])
def test_hand_made_rows_uncut(kind, name):
    vs = CR.settings(name)
    tsubs, vsubs = uncut(kind, name, coded=(kind, name) == ("psk", "crc8"))  # once with the line code ahead of it
    (trecs, twords), (got, words) = tsubs[0], vsubs[0]
    assert [int(r["n_ok"]) for r in got] == [int(crc.bits_of(r, words).sum()) for r in got]
    assert all(int(r["n_ok"]) == 0 and int(r["first_at"]) == crc.NONE for r in got if r["n_samples"] <= vs.D)  # a run shorter than D
    if kind != "long":
        assert got[0]["stream"] == 0 and got[0]["start_sample"] == 0  # a run at submit index 0
        assert (got["bit_offset"][1:] % 32 != 0).any()  # runs that share a bitmap word
        assert any(r["start_sample"] < B < r["start_sample"] + r["n_samples"] for r in got)  # a run across the block boundary
        last = got[(got["stream"] == 1) & (got["start_sample"] == 2 * B - 2)]  # a run of 2 samples, open at the last sample
        assert len(last) == 1 and last[0]["flags"] == OPEN and last[0]["n_samples"] == 2 and last[0]["n_ok"] == 0
    if name == "reach":
        assert vs.D == 16381 and got["n_ok"].sum() == 0  # no run here is that long


@pytest.mark.parametrize("name", list(CR.SETS))
@pytest.mark.parametrize("kind", ["psk", "fsk", "long"])
def test_the_same_rows_in_one_block_submits_queued_before_the_first_read(kind, name):
    vs = CR.settings(name)
    rows, mode, L, centres = ROWS[kind]
    rows = rows()
    whole = uncut(kind, name, coded=(kind, name) == ("psk", "crc8"))
    tsubs, vsubs = run_cut(rows, mode, L, centres, vs, (1,) * (rows.shape[1] // B), code=linecode.nrzi(38400) if (kind, name) == ("psk", "crc8") else None)
    if kind != "long":
        o = {int(r["stream"]): r for r in vsubs[0][0] if r["flags"] & OPEN}
        c = {int(r["stream"]): r for r in vsubs[1][0] if r["flags"] & CONT}
        assert (o[0]["n_samples"], o[1]["n_samples"]) == (3, 500) and sorted(c) == [0, 1]  # runs of 3 and 500 samples at a submit's end, continued
    else:
        assert [int(r["n_samples"]) for recs, _ in vsubs for r in recs if r["stream"] == 0] == [1000, B, 3000 + R.W - 1]  # three pieces
    if kind != "psk":  # the frequency track does not depend on the cut: the merged chains are the uncut run's
        same_chains(merged(vsubs), merged(whole[1]), "one block a submit")


def test_planted_frames_check_across_the_cuts():
    """Stream 0's frame ends in the third piece of its chain, 11776 samples behind its first bit in the first piece: the history
    reaches over a whole block.  Stream 1's lies across the block boundary.  Stream 2's has the largest reach there is, 16381 samples:
    a window then begins within the first words of LDS, the bit index still above 0."""
    rows, planted = CR.planted_rows()
    for s, (name, frame) in planted.items():
        vs = CR.settings(name)
        whole = run_cut(rows, None, 11, [0, 0, 0], vs, (3,))
        tsubs, vsubs = run_cut(rows, None, 11, [0, 0, 0], vs, (1, 1, 1))
        same_chains(merged(vsubs), merged(whole[1]), name)
        v = [c for c in merged(vsubs) if c["stream"] == s][0]
        t = [c for c in sorted(track.chains(tsubs), key=key) if c["stream"] == s][0]
        ok = np.flatnonzero(v.bits)
        assert int(v["n_ok"]) == len(ok) >= 1 and int(v["first_at"]) == ok[0]
        read = {int(k): CR.frame_at(vs, t.bits, int(k)) for k in ok}  # the frames, read where the check says they end
        assert all(vs.check(f) for f in read.values())  # (an 8-bit CRC may hold by chance elsewhere in the burst)
        mine = [k for k in read if read[k] == frame]  # the planted frame: one stretch, a symbol wide at most
        assert 1 <= len(mine) <= 384000 // vs.rate + 1 and mine == list(range(mine[0], mine[-1] + 1)), (name, mine)
        if name == "whb":
            pieces = [r for recs, _ in vsubs for r in recs if r["stream"] == 0]
            assert [int(p["n_samples"]) for p in pieces][:2] == [1000, B] and [int(p["n_ok"]) for p in pieces][:2] == [0, 0]
            assert int(pieces[2]["n_ok"]) == len(ok) == len(mine) and vs.D > B  # the verdict comes in the submit that holds the last bit
            assert not alone(pieces[2], tsubs[2][1], vs).any()  # ... and needs what the stream carried


def test_a_reset_mid_chain_drops_the_history():
    """Two constant tones from B - 1000 to 2 B + 3000.  With init 0 and xorout 0 a constant stretch is an all-zero frame, which
    checks at every defined sample: a piece that continues checks from its first sample, one behind a reset from sample D."""
    rows = np.stack([quiet(3, 61), quiet(3, 62)])
    n = B + 4000
    rows[:, B - 1000:B - 1000 + n] = fsk([1] * (n * 17240 // 384000 + 2), 17240)[:n]
    trecs, twords = RR.submits(decin.clamp(rows)[0].reshape(-1), (3,), 11, thresh=R.T)[0]  # the restatement's track of the tone: all 0, or all 1
    ones = track.bits_of(trecs[0], twords)[100:-800].all()
    assert ones or not track.bits_of(trecs[0], twords)[100:-800].any()
    vs = crc.Settings(17240, 4, 8, 0x31, invert=bool(ones))
    tsubs, vsubs = run_cut(rows, None, 11, [0, 0], vs, (1, 1, 1), resets={1: [1]})
    r1 = vsubs[1][0]
    zero, one = r1[r1["stream"] == 0][0], r1[r1["stream"] == 1][0]
    assert zero["flags"] & CONT and not one["flags"] & CONT and one["start_sample"] < 16  # a reset stream counts from 0 again
    assert zero["n_samples"] == B and crc.bits_of(zero, vsubs[1][1]).all() and zero["first_at"] == 0  # its history: 1000 samples, above D
    assert not alone(zero, tsubs[1][1], vs)[:vs.D].any() and vs.D == 713
    got = crc.bits_of(one, vsubs[1][1])
    assert np.array_equal(got, alone(one, tsubs[1][1], vs)) and not got[:vs.D].any() and got[vs.D + 100:].all() and int(one["first_at"]) >= vs.D


@pytest.mark.parametrize("n", [65, 97])
def test_stream_counts_across_a_waves_end(n):
    nb = 4
    vs = CR.settings("crc8")
    rng = np.random.default_rng(43)
    symbols = sum((CR.planted_symbols(vs, 100 + k, pre=30, post=9)[0] for k in range(70)), [])
    kinds = [rng.integers(-400, 401, size=(nb * B, 2)).astype(np.int16), fsk(symbols, 17240)[:nb * B], fsk(symbols[5:], 17240, amp=3000)[:nb * B],
             quiet(nb, 44)]  # rows 0 .. 2 never leave their window
    kinds[0][0] = (300, 300)  # (... from the first sample on)
    x = np.ascontiguousarray(np.stack(kinds)[np.arange(n) % len(kinds)])
    if n == 65:  # the same rows again in a second submit: every run CONTINUES
        x = np.concatenate([x, x], axis=1)
    tsubs, vsubs = run_cut(x, None, 11, [0] * n, vs, (nb, nb) if n == 65 else (nb,))
    got, words = vsubs[-1]
    assert got["stream"].tolist() == [s for s in range(n) if s % 4 != 3] and (got["n_samples"] == nb * B).all()
    for s in (1, 2):  # copies of a row have the row's check track, with the planted frames in it
        same = [crc.bits_of(g, words).tobytes() for g in got if g["stream"] % 4 == s]
        assert len(same) >= 16 and len(set(same)) == 1
        assert min(int(g["n_ok"]) for g in got if g["stream"] % 4 == s) >= 1
    if n == 65:
        assert (got["flags"] == CONT | OPEN).all() and (vsubs[0][0]["flags"] == OPEN).all()
        first, fw = vsubs[0]  # the same rows: the first submit's first D samples are undefined, the second's have their history
        assert all(not crc.bits_of(b, fw)[:vs.D].any() for b in first)
        assert any(crc.bits_of(a, words)[:vs.D].any() for a in got)
        assert all(np.array_equal(crc.bits_of(a, words)[vs.D + 16:], crc.bits_of(b, fw)[vs.D + 16:]) for a, b in zip(got, first))


def test_overflow_on_max_runs_and_on_max_samples_delivers_the_prefixes_and_loses_the_history():
    vs = crc.Settings(17240, 4, 8, 0x31)
    rows, mode, L, centres = ROWS["fsk"]
    rows = rows()
    whole = run_cut(rows, mode, L, centres, vs, (2,))[1][0][0]
    tsubs, vsubs = run_cut(rows, mode, L, centres, vs, (2,), cap=(len(whole) - 1, 4 * B))  # the table a run short
    same_records(vsubs[0][0], whole[:-1], "the prefix")
    assert len(vsubs[0][1]) == (int(whole[-1]["bit_offset"]) + 31) // 32
    with hand_receiver(2, 2, (), cap=(len(whole) - 1, 4 * B)) as r:
        r.enable_burst_track(L)
        r.enable_burst_crc(*vs.args()[:2], vs.W, vs.poly)
        r.submit(np.ascontiguousarray(rows))
        raises(api.E_OVERFLOW, r.read_burst_crcs)
        r.drain()
    full = run_cut(rows, mode, L, centres, vs, (1, 1))
    # (1, 1) submits with a table one run short of the first submit: its last run, stream 1's OPEN piece, has no record and leaves no
    # history -- the piece that continues it reads as a chain's first; stream 0's continues as ever
    n0 = len(full[1][0][0])
    tsubs, vsubs = run_cut(rows, mode, L, centres, vs, (1, 1), cap=(n0 - 1, 4 * B))
    same_records(vsubs[0][0], full[1][0][0][:-1], "the runs that have a record")
    b, wb = vsubs[1]
    c, fc = b[(b["flags"] & CONT) != 0], full[1][1][0][(full[1][1][0]["flags"] & CONT) != 0]
    assert c["stream"].tolist() == [0, 1] and np.array_equal(crc.bits_of(c[0], wb), crc.bits_of(fc[0], full[1][1][1]))
    assert np.array_equal(crc.bits_of(c[1], wb), alone(c[1], tsubs[1][1], vs)) and not crc.bits_of(c[1], wb)[:vs.D].any()
    assert crc.bits_of(fc[1], full[1][1][1])[:vs.D].any()  # (with its history the same piece has defined samples there, and some check)
    # ... and with a pool one pair short of the first submit: the same run does not fit, has no bits and leaves no history
    room = int(full[1][0][0]["n_samples"].sum()) - 1
    tsubs, vsubs = run_cut(rows, mode, L, centres, vs, (1, 1), cap=(32, room))
    a, wa = vsubs[0]
    same_records(a[:-1], full[1][0][0][:-1], "the runs that fit")
    assert a[-1]["stream"] == 1 and a[-1]["flags"] & OPEN and a[-1]["n_ok"] == 0 and a[-1]["first_at"] == crc.NONE
    assert len(wa) == (int(a[-1]["bit_offset"]) + 31) // 32
    b, wb = vsubs[1]  # (the second submit is smaller: everything fits)
    c = b[(b["flags"] & CONT) != 0]
    assert c["stream"].tolist() == [0, 1] and c[0].tobytes() == fc[0].tobytes()
    assert np.array_equal(crc.bits_of(c[1], wb), alone(c[1], tsubs[1][1], vs))


# ---- the other kinds of context
def test_the_golden_whb_scene_with_the_phase_track_the_code_the_sync_and_the_check():
    x = golden_iq("whb", 6)
    cs, st, vs = linecode.g3ruh(6000), sync.Settings(6000, LR.WORD, 16, 0), CR.golden_settings("whb", 23)
    with api.Receiver(1, 0x2F, 500, 0, max_blocks=6, all_flushes=True) as r:
        plain_mem = r.memory()
        r.submit(x)
        plain = r.drain()
    with api.Receiver(1, 0x2F, 500, 0, max_blocks=6, all_flushes=True, levels=True) as r:
        r.enable_capture(256, 6 * B)
        r.enable_burst_track_phase(16, 1024, 64)
        r.enable_burst_code(cs.rate, cs.taps, cs.invert)
        r.enable_burst_sync(st.rate, st.pattern, st.P, st.E)
        base_mem = r.memory()
        r.submit(x)
        base = (r.read_captures(), r.read_burst_tracks(), r.read_burst_track_centres(), r.read_burst_codes(), r.read_burst_syncs())
        raises(api.E_INVAL, r.read_burst_crcs)  # not enabled
        r.drain()
    with api.Receiver(1, 0x2F, 500, 0, max_blocks=6, all_flushes=True, levels=True) as r:
        r.enable_capture(256, 6 * B)
        r.enable_burst_track_phase(16, 1024, 64)
        r.enable_burst_code(cs.rate, cs.taps, cs.invert)
        r.enable_burst_sync(st.rate, st.pattern, st.P, st.E)
        assert r.memory() == base_mem  # a context without the call holds what it held
        r.enable_burst_crc(vs.rate, vs.N, vs.W, vs.poly, vs.init, vs.xorout, vs.S, vs.lsb, vs.invert)
        m = r.memory()
        assert m["device_bytes"] - base_mem["device_bytes"] == crc.device_bytes(1, 256, 6 * B, 23)
        assert m["pinned_host_bytes"] - base_mem["pinned_host_bytes"] == crc.pinned_bytes(1)
        r.submit(x)
        (crecs, cwords), (got, words), _ = read_crc(r, vs, None, code=cs)
        now = (r.read_captures(), r.read_burst_tracks(), r.read_burst_track_centres(), (crecs, cwords), r.read_burst_syncs())
        ev = r.drain()
    with api.Receiver(1, 0x2F, 500, 0, max_blocks=6, all_flushes=True) as r:
        assert r.memory() == plain_mem
    R.assert_tables(now[0], base[0])
    assert now[2].tobytes() == base[2].tobytes()  # the centre records
    for a, b in zip((now[1], now[3], now[4]), (base[1], base[3], base[4])):  # the track, the code, the sync: records and words
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    assert parity.sort_events(ev).tobytes() == parity.sort_events(plain).tobytes() and len(ev) >= 1
    assert len(got) == 1 and (int(got[0]["n_ok"]), int(got[0]["first_at"])) == (CR.WHB_N_OK, CR.WHB_FIRST_AT)
    cch, sch, vch = linecode.chains([(crecs, cwords)]), sync.chains([now[4]]), crc.chains([(got, words)])
    fr = sync.frames(cch[0], sch[0], st, 23, lsb=True)
    assert [sync.line("f", sch[0], f) for f in fr] == ["frame f 10004 24316 0 + 184 " + CR.GOLDEN_FRAMES["whb"][0]]
    assert crc.verdicts(fr, vch[0], vs) == ["ok"]  # the one frame
    assert crc.line("f", vch[0], vs) == "crc f 10004 28344 64 24285"


def test_a_submit_runs_replay_gives_the_recordings_check():
    """The golden WHB scene recorded by a u8 context (1 + 5 blocks) and replayed through sparse submits (3 + 3), without a sync."""
    x = golden_iq("whb", 6)
    cs, vs = linecode.g3ruh(6000), CR.golden_settings("whb", 23)

    def on(r):
        r.enable_burst_track_phase(16, 1024, 64)
        r.enable_burst_crc(vs.rate, vs.N, vs.W, vs.poly, vs.init, vs.xorout, vs.S, vs.lsb, vs.invert)  # ahead of the code: the input is chosen per submit
        r.enable_burst_code(cs.rate, cs.taps)

    with api.Receiver(1, 0x2F, 500, 0, max_blocks=5, all_flushes=True, levels=True) as r:
        r.enable_capture(256, 6 * B)
        r.enable_capture_pre()
        on(r)
        tabs, recs, state = [], [], None
        for p in parity.cut(x, (1, 5)):
            r.submit(p)
            tabs.append(r.read_captures(pre=True))
            _, v, state = read_crc(r, vs, state, code=cs)
            recs.append(v)
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
        rep, state = [], None
        for k in range(2):
            t, p, q = decin.rebase(runs, pool, pre, 3 * k * B, 3 * B)
            assert r.submit_runs(t, p, q, 3) == 3
            _, v, state = read_crc(r, vs, state, code=cs)
            rep.append(v)
            r.drain()
    a, b = crc.chains(recs), crc.chains(rep)
    assert len(a) == len(b) == 1 and any(rec["flags"] & CONT for cr, _ in rep for rec in cr)  # the replay cuts the burst
    same_chains(b, a, "the replay")
    assert (int(b[0]["n_ok"]), int(b[0]["first_at"])) == (CR.WHB_N_OK, CR.WHB_FIRST_AT)


def test_the_refusals():
    x = scene()[:3, :api.BLOCK_BYTES]
    good = (17240, 5, 8, 0x31)
    with api.Receiver(3, CTX_TYPES, 500, 0, max_blocks=2) as r:
        raises(api.E_INVAL, r.enable_burst_crc, *good)  # no recorder, no track
        raises(api.E_INVAL, r.read_burst_crcs)
        r.enable_capture(64, 1024)
        raises(api.E_INVAL, r.enable_burst_crc, *good)  # the recorder alone: no track
        r.enable_burst_track(11)
        m = r.memory()
        for bad in ((999, 5, 8, 0x31), (96001, 5, 8, 0x31), (6000, 0, 8, 0x31), (48002, 257, 8, 0x31), (6000, 5, 12, 0x31), (6000, 5, 0, 0x31),
                    (6000, 5, 8, 0), (6000, 5, 8, 0x131), (6000, 5, 8, 0x31, 0x100), (6000, 5, 8, 0x31, 0, 0x100), (6000, 5, 8, 0x31, 0, 0, -1),
                    (6000, 5, 8, 0x31, 0, 0, 4), (6000, 5, 32, 0x04C11DB7, 0, 0, 1), (6000, 32, 8, 0x07), (2 ** 31, 5, 8, 0x31), (6000, 5, 8, 1 << 32),
                    (6000, 5, 8, -1), (6000, 5, 2 ** 31, 0x31)):
            raises(api.E_INVAL, r.enable_burst_crc, *bad)
        assert r.L.tfrec_amd_enable_burst_crc(r.h, 17240, 5, 0, 8, 0x31, 0, 0, 4) == api.E_INVAL  # an unknown flag
        assert r.memory() == m  # nothing was allocated
        raises(api.E_INVAL, r.read_burst_crcs)  # not enabled
        r.enable_burst_crc(6001, 32, 8, 0x07, lsb=True, invert=True)  # D = 16381; no sync, no code
        m2 = r.memory()
        assert m2["device_bytes"] - m["device_bytes"] == crc.device_bytes(3, 64, 1024, 32) and m2["pinned_host_bytes"] == m["pinned_host_bytes"]
        raises(api.E_INVAL, r.enable_burst_crc, *good)  # a second call: refused, and nothing changes
        assert r.memory() == m2
        raises(api.E_STATE, r.read_burst_crcs)  # nothing undrained
        r.submit(x)
        nr, nw = api.C.c_uint32(0), api.C.c_uint64(0)
        buf = np.full(40, 0x55, dtype=np.uint8)  # the caller's room too small: E_INVAL, nothing written, the counts set
        f = r.L.tfrec_amd_read_burst_crcs
        assert f(r.h, buf.ctypes.data, 0, api.C.byref(nr), None, 0, api.C.byref(nw)) == api.E_INVAL and (buf == 0x55).all()
        trecs, twords = r.read_burst_tracks()
        assert nr.value == len(trecs) == len(r.read_captures()[0]) == 1 and nw.value == len(twords)
        assert f(r.h, buf.ctypes.data, 1, api.C.byref(nr), None, 5, api.C.byref(nw)) == api.E_INVAL  # no words, yet room for some
        assert f(r.h, buf.ctypes.data, 1, api.C.byref(nr), None, 0, api.C.byref(nw)) == api.E_OK  # the records alone
        _, (got, words), _ = read_crc(r, crc.Settings(6001, 32, 8, 0x07, lsb=True, invert=True), None)
        assert buf.tobytes() == got.tobytes()
        r.drain()
    with api.Receiver(3, CTX_TYPES, 500, 0, max_blocks=2) as r:
        r.enable_capture(64, 1024)
        r.enable_burst_track(11)
        r.submit(x)
        raises(api.E_STATE, r.enable_burst_crc, *good)  # after the first submit
        r.drain()


# ---- tfrec_gpu -G -U -Y -V
def test_cli_lines_of_the_golden_whb_scene_with_the_frame_across_batch_boundaries(tmp_path):
    parity.build_cli()
    x, want = CR.cli_scene()
    f = str(tmp_path / "whb.iq")
    x.tofile(f)
    want = [ln % f for ln in want]
    kinds = ("centre", "bits", "code", "frame", "crc")  # every kind of line, in the order they were printed
    base = ["-T", "2f", "-t", "500", "-b", "1", "-L", f]
    got = cli_lines(CR.CLI_ARGS + base, kinds, "frame")
    assert got[kinds] == want and [ln.split()[0] for ln in want] == ["centre", "bits", "code", "frame", "crc"]
    assert got["frame"][0].split()[3:] == [str(19004 + 14312), "0", "+", "184", CR.GOLDEN_FRAMES["whb"][0], "ok"]
    assert got[kinds][-1].split()[2:] == ["19004", "28344", "64", str(19004 + LR.WHB_PLATEAU[0])]
    # without -V every line is what it was
    plain = cli_lines(CR.CLI_ARGS[:-2] + base, kinds)
    assert plain[kinds] == want[:3] + [want[3][:-3]] and plain["telegrams"] == got["telegrams"]
    # a wrong init: the same frame, bad, and nothing in the burst checks
    wrong = cli_lines(CR.CLI_ARGS[:-1] + ["32,04c11db7,f59c5a1f,0,1"] + base, kinds)
    assert wrong[kinds] == want[:3] + [want[3][:-2] + "bad", "crc %s 19004 28344 0 -" % f]
