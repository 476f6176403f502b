"""The burst sync on the GPU (tfrec_amd_enable_burst_sync, tfrec_amd_read_burst_syncs, tfrec_gpu -G -Y), bit for bit.

The records and the match bitmap's words are compared, byte for byte, with the restatement tfrec_amd/sync.py run on the context's
OWN track (tfrec_amd_read_burst_tracks) and run table, and that track with tfrec_amd/track.py on the context's own decimated
samples (tests/recorder.py: read_sync on read_track), so everything ahead of the sync is whatever the context runs.  Channel-rate
contexts take hand-made FSK rows with the sync word planted where the kernels can go wrong; every such case asserts that the
expected match track has a one in the place it is about.  Everything is an exact integer; nothing here has a tolerance.

One class of the list in DESIGN.md 6u cannot be placed on a device: a chain's middle piece both CONTINUES and is OPEN, so it is a
whole submit, at least 8192 samples -- never 500.  The three-piece chain here is 1000 samples, a whole block, and the rest; pieces
of 1000 and 500 samples, which need the carried words combined, are tests/test_sync_cpu.py's, on the restatement.  Nothing here is
measured on real recordings."""
import functools

import numpy as np
import pytest

import parity
import recorder as R
from recorder import (B, CONT, OPEN, W, cli_lines, hand_receiver, raises, read_clock, read_envelope, read_sync, read_track,
                      same_chains, same_records, zeros)
from recorder_rows import CTX_TYPES, PAYLOADS, PLATEAUS, WORD, frame_symbols, fsk, golden_iq, quiet, scene, shifted_tfa_2
from tfrec_amd import api, burst, decin, sync, track

pytestmark = pytest.mark.gpu

WORD64 = 0x5A0FF0A5C3963C69
# (rate, word, P, E, BOTH): P = 8, 16, 24 (span 2047) and 64; E = 0 and P / 2 - 1; BOTH with stream 1's frames inverted
CASES = {"p16": (17240, WORD, 16, 0, False), "p16_e7": (17240, WORD, 16, 7, False), "p8": (17240, 0xD4, 8, 0, False),
         "p64": (12000, WORD64, 64, 3, False), "p24_span2047": (4315, 0xAA2DD4, 24, 1, False), "both": (17240, WORD, 16, 1, True)}


def receiver(n, nb, st, cap=None, **kw):
    stages = {"track": (track.smooth_of(st.rate),), "sync": (st.rate, st.pattern, st.P, st.E, st.both)}
    return hand_receiver(n, nb, stages, cap=cap, **kw)


def run_cut(rows, st, sizes, cap=None, resets=None):
    """The rows in submits of `sizes` blocks, all queued before the first read; every submit's track and sync checked ->
    [(track records, track words)], [(sync records, sync words)].  resets: {submit index: streams reset ahead of it} (then the
    submits are not queued: a reset comes between them)."""
    n, L = len(rows), track.smooth_of(st.rate)
    parts, pos = [], 0
    for nb in sizes:
        parts.append((pos, nb, np.ascontiguousarray(rows[:, pos * B:(pos + nb) * B])))
        pos += nb
    tsubs, ssubs = [], []
    with receiver(n, max(sizes), st, cap=cap) as r:
        if not resets:
            for _, _, x in parts:
                r.submit(x)
        tstate = sstate = None
        origin = [0] * n
        for i, (pos, nb, x) in enumerate(parts):
            if resets:
                if i in resets:
                    r.reset_streams(resets[i])
                    for s in resets[i]:
                        origin[s] = pos * B
                r.submit(x)
            part = decin.clamp(x)
            trecs, twords, _, tstate = read_track(r, nb, [pos * B - o for o in origin], L, [0] * n, tstate,
                                                  decs=[part[s].reshape(-1) for s in range(n)], overflow=cap is not None)
            srecs, swords, sstate = read_sync(r, st, sstate, trecs, twords, overflow=cap is not None)
            if i == 0:
                again = r.read_burst_syncs(allow_overflow=cap is not None)  # reading pops nothing
                assert again[0].tobytes() == srecs.tobytes() and again[1].tobytes() == swords.tobytes()
            tsubs.append((trecs, twords))
            ssubs.append((srecs, swords))
            r.drain()
        raises(api.E_STATE, r.read_burst_syncs)  # nothing undrained
    return tsubs, ssubs


# ---- hand-made FSK rows on a channel-rate context
def plant(rows, s, at, symbols, rate):
    x = fsk(symbols, rate)
    at = int(at)
    n = min(len(x), rows.shape[1] - at)
    rows[s, at:at + n] = x[:n]
    return at + n


@functools.lru_cache(maxsize=None)
def hand_rows(case):
    """int16 [2, 2 B, 2] for a case's rate and word.
    Stream 0: a run from the submit's first sample (37 tone samples: 730 long, so every later run of the pool starts off a word
    boundary); a frame whose sync word lies across sample B; a run open at the input's last sample, 100 samples: shorter than
    every span.
    Stream 1 (its frames inverted under BOTH): frames where there is room for them, and one whose word's last symbol centre is
    sample B, so that the plateau lies across it."""
    rate, word, P, _, both = CASES[case]
    sps = 384000.0 / rate
    L = track.smooth_of(rate)
    rows = np.stack([quiet(2, 31), quiet(2, 32)])
    rows[0, :37] = fsk([1, 0], rate)[:37]
    plant(rows, 0, B - (16 + P / 2) * sps, frame_symbols(word, P, 1), rate)
    rows[0, 2 * B - 100:] = fsk([1, 0] * 50, rate)[:100]
    length = int((48 + P) * sps) + 1
    at = B - int(round((16 + P - 0.5) * sps)) - L // 2
    end = plant(rows, 1, at, frame_symbols(word, P, 2, invert=both), rate)
    for k, pos in enumerate((300, 300 + length + W + 200)):
        if pos + length + W + 50 < at:
            plant(rows, 1, pos, frame_symbols(word, P, 3 + k, invert=both), rate)
    if end + W + 50 + length < 2 * B:
        plant(rows, 1, end + W + 50, frame_symbols(word, P, 5, invert=both), rate)
    rows.setflags(write=False)
    return rows


def settings(case):
    return sync.Settings(*CASES[case])


@functools.lru_cache(maxsize=None)
def hand_uncut(case):
    return run_cut(hand_rows(case), settings(case), (2,))


def merged(tsubs, ssubs):
    key = lambda c: (int(c["stream"]), int(c["start_sample"]))  # noqa: E731
    return sorted(track.chains(tsubs), key=key), sorted(sync.chains(ssubs), key=key)


def at_sample(chain, sample):
    """The chain's match bit at an absolute sample."""
    k = sample - int(chain["start_sample"])
    return int(chain.bits[k]) if 0 <= k < len(chain.bits) else 0


@pytest.mark.parametrize("case", list(CASES))
def test_two_streams_of_two_blocks_with_the_word_planted(case):
    st = settings(case)
    tsubs, ssubs = hand_uncut(case)
    got, words = ssubs[0]
    tch, sch = merged(tsubs, ssubs)
    assert (got["bit_offset"][1:] % 32 != 0).any() and got[0]["n_samples"] == 36 + W and got["reserved"].max() == 0
    # stream 0: the word across the block boundary: a match whose samples begin ahead of sample B and end behind it
    a = [c for c in sch if c["stream"] == 0 and c["start_sample"] < B < c["start_sample"] + c["n_samples"]]
    assert len(a) == 1
    hits = np.flatnonzero(a[0].bits) + int(a[0]["start_sample"])
    assert any(k - st.span < B <= k for k in hits), "no match across the block boundary"
    assert int(a[0]["best"]) <= st.E
    # the run shorter than the span: nothing is defined
    last = got[(got["stream"] == 0) & (got["start_sample"] == 2 * B - 100)]
    assert len(last) == 1 and last[0]["flags"] == OPEN and (last[0]["best"], last[0]["best_at"], last[0]["n_hits"]) == (sync.NONE, 0, 0)
    assert st.span > 100
    # stream 1: the plateau across sample B
    b = [c for c in sch if c["stream"] == 1 and c["start_sample"] < B < c["start_sample"] + c["n_samples"]]
    assert len(b) == 1 and at_sample(b[0], B - 1) and at_sample(b[0], B), "no plateau across sample B"
    if case in ("p16", "both", "p8"):  # a plateau that lies across a word boundary of the bitmap, in a run that starts off one
        across = [(r, p) for r in got if r["bit_offset"] % 32 for p in sync.plateaus(sync.bits_of(r, words))
                  if (int(r["bit_offset"]) + p[0]) // 32 != (int(r["bit_offset"]) + p[1]) // 32]
        assert across
    if case == "both":  # the inverted frames are found in the other polarity, the plain one of stream 0 in this
        f1 = [f for t, s in zip(tch, sch) if s["stream"] == 1 for f in sync.frames(t, s, st, 4)]
        f0 = [f for t, s in zip(tch, sch) if s["stream"] == 0 for f in sync.frames(t, s, st, 4)]
        assert len(f1) >= 3 and {f[2] for f in f1} == {"-"} and {f[2] for f in f0} == {"+"}
    if case == "p24_span2047":
        assert st.span == 2047
    if case == "p16_e7":
        assert st.E == st.P // 2 - 1 and got["n_hits"].sum() > 10 * hand_uncut("p16")[1][0][0]["n_hits"].sum()


@pytest.mark.parametrize("case", list(CASES))
def test_the_same_rows_in_two_submits_queued_before_the_first_read(case):
    st = settings(case)
    whole = merged(*hand_uncut(case))
    tsubs, ssubs = run_cut(hand_rows(case), st, (1, 1))
    c = ssubs[1][0][(ssubs[1][0]["flags"] & CONT) != 0]
    assert c["stream"].tolist() == [0, 1]
    # the continuing pieces hold matches that need the carried bits: ones among their first span samples
    for rec in c:
        assert sync.bits_of(rec, ssubs[1][1])[:st.span].any(), "no match across the submit boundary"
    assert sync.bits_of(c[1], ssubs[1][1])[0] == 1  # ... stream 1's at its very first sample: the plateau lies across the cut
    o = ssubs[0][0][(ssubs[0][0]["flags"] & OPEN) != 0]
    assert o["stream"].tolist() == [0, 1] and sync.bits_of(o[1], ssubs[0][1])[-1] == 1
    got = merged(tsubs, ssubs)
    assert len(got[1]) == len(whole[1])
    same_chains("sync", got[1], whole[1], "1 + 1")


@functools.lru_cache(maxsize=None)
def long_rows():
    """int16 [2, 3 B, 2]: transmissions from B - 1000 (stream 0) and B - 1500 (stream 1) to 2 B + 3000, alternating symbols with
    the word every 800 samples; one ends 100 samples behind sample B and one 100 behind 2 B, so both lie across a block's end."""
    rows = np.stack([quiet(3, 33), quiet(3, 34)])
    for s, at in ((0, B - 1000), (1, B - 1500)):
        symbols = [i & 1 for i in range((2 * B + 3000 - at) * 17240 // 384000 + 2)]
        for end in range(B + 100 - 800, 2 * B + 3000, 800):  # (B + 100 and 2 B + 100 = B + 100 + 8192 are not both on one grid of 800)
            for e in (end, end + 8192 % 800 if end > 2 * B - 800 else end):
                i = (e - at) * 17240 // 384000
                if 16 <= i < len(symbols):
                    symbols[i - 15:i + 1] = [(WORD >> (15 - k)) & 1 for k in range(16)]
        x = fsk(symbols, 17240)
        rows[s, at:2 * B + 3000] = x[:2 * B + 3000 - at]
    rows.setflags(write=False)
    return rows


def test_a_chain_of_three_pieces():
    """1000 samples, a whole block and the rest (see the module's text): the second cut's history comes from a piece that itself
    began with carried bits."""
    st = settings("p16")
    tsubs, ssubs = run_cut(long_rows(), st, (1, 1, 1))
    assert [int(r["n_samples"]) for recs, _ in ssubs for r in recs if r["stream"] == 0] == [1000, B, 3000 + W - 1]
    for k in (1, 2):
        for rec in ssubs[k][0]:
            assert rec["flags"] & CONT and sync.bits_of(rec, ssubs[k][1])[:st.span].any()
    whole = merged(*run_cut(long_rows(), st, (3,)))
    got = merged(tsubs, ssubs)
    assert len(got[1]) == len(whole[1]) == 2
    same_chains("sync", got[1], whole[1], "1 + 1 + 1")
    assert all(int(a["n_hits"]) > 100 for a in got[1])


def test_a_reset_mid_chain_drops_the_history():
    st = settings("p16")
    tsubs, ssubs = run_cut(long_rows(), st, (1, 1, 1), resets={1: [1]})
    r1 = ssubs[1][0]
    zero, one = r1[r1["stream"] == 0][0], r1[r1["stream"] == 1][0]
    assert zero["flags"] & CONT and not one["flags"] & CONT and one["start_sample"] < 16  # a reset stream counts from 0 again
    assert sync.bits_of(zero, ssubs[1][1])[:st.span].any() and not sync.bits_of(one, ssubs[1][1])[:st.span].any()
    assert one["best_at"] >= st.span


@pytest.mark.parametrize("n", [65, 97])
def test_stream_counts_across_a_waves_end(n):
    nb = 4
    st = sync.Settings(17240, WORD, 16, 2, True)
    rng = np.random.default_rng(43)
    symbols = sum((frame_symbols(WORD, 16, 100 + k, pre=4, pay=9, invert=k % 3 == 1) for k in range(70)), [])
    kinds = [rng.integers(-400, 401, size=(nb * B, 2)).astype(np.int16), fsk(symbols, 17240)[:nb * B], fsk(symbols[5:], 17240, amp=3000)[:nb * B],
             quiet(nb, 44)]  # rows 0 .. 2 never leave their window
    kinds[0][0] = (300, 300)  # (... from the first sample on)
    x = np.ascontiguousarray(np.stack(kinds)[np.arange(n) % len(kinds)])
    if n == 65:  # the same rows again in a second submit: every run CONTINUES
        x = np.concatenate([x, x], axis=1)
    tsubs, ssubs = run_cut(x, st, (nb, nb) if n == 65 else (nb,))
    got, words = ssubs[-1]
    assert got["stream"].tolist() == [s for s in range(n) if s % 4 != 3] and (got["n_samples"] == nb * B).all()
    for s in (1, 2):  # copies of a row have the row's match track
        same = [sync.bits_of(g, words).tobytes() for g in got if g["stream"] % 4 == s]
        assert len(same) >= 16 and len(set(same)) == 1
        assert got[got["stream"] % 4 == s]["n_hits"].min() > 500 and (got[got["stream"] % 4 == s]["best"] == 0).all()
    if n == 65:
        assert (got["flags"] == CONT | OPEN).all() and (ssubs[0][0]["flags"] == OPEN).all()
        first = ssubs[0][0]  # the same rows, but every sample of the second submit has its history: none is undefined
        assert (got["n_hits"] >= first["n_hits"]).all() and (got["n_hits"] > first["n_hits"]).any()


def test_overflow_on_max_runs_and_on_max_samples_delivers_the_prefixes():
    st = settings("p16")
    rows = hand_rows("p16")
    whole = hand_uncut("p16")[1][0][0]
    tsubs, ssubs = run_cut(rows, st, (2,), cap=(len(whole) - 1, 4 * B))  # the table a run short
    same_records(ssubs[0][0], whole[:-1], "the prefix")
    assert len(ssubs[0][1]) == (int(whole[-1]["bit_offset"]) + 31) // 32
    with receiver(2, 2, st, cap=(len(whole) - 1, 4 * B)) as r:
        r.submit(np.ascontiguousarray(rows))
        raises(api.E_OVERFLOW, r.read_burst_syncs)
        r.drain()
    # (1, 1) submits with a pool one pair short of the first submit: its last run, stream 1's OPEN piece, does not fit, has no bits
    # and leaves no history -- the piece that continues it starts undefined, where with room for everything it has its matches;
    # stream 0's, which fitted, continues as ever
    full = run_cut(rows, st, (1, 1))[1]
    room = int(full[0][0]["n_samples"].sum()) - 1
    tsubs, ssubs = run_cut(rows, st, (1, 1), cap=(32, room))
    a, wa = ssubs[0]
    same_records(a[:-1], full[0][0][:-1], "the runs that fit")
    assert a[-1]["stream"] == 1 and a[-1]["flags"] & OPEN and (a[-1]["best"], a[-1]["best_at"], a[-1]["n_hits"]) == (sync.NONE, 0, 0)
    assert full[0][0][-1]["n_hits"] > 0 and len(wa) == (int(a[-1]["bit_offset"]) + 31) // 32
    b, wb = ssubs[1]  # (the second submit is smaller: everything fits)
    c, fc = b[(b["flags"] & CONT) != 0], full[1][0][(full[1][0]["flags"] & CONT) != 0]
    assert c["stream"].tolist() == [0, 1] and c[0].tobytes() == fc[0].tobytes()
    assert c[1]["best_at"] >= st.span and not sync.bits_of(c[1], wb)[:st.span].any()
    assert sync.bits_of(fc[1], full[1][1])[:st.span].any() and fc[1]["best_at"] < st.span


# ---- the other kinds of context
def test_the_golden_tfa_2_scene_with_all_five_measurements_and_none():
    x = golden_iq()
    st = sync.Settings(17240, WORD, 16, 1)
    with api.Receiver(1, 0x2F, 500, 0, max_blocks=4, all_flushes=True) as r:
        plain_mem = r.memory()
        r.submit(x)
        plain = r.drain()
    with api.Receiver(1, 0x2F, 500, 0, max_blocks=4, all_flushes=True, levels=True) as r:
        r.enable_capture(256, 4 * B)
        r.enable_burst_track(11)
        trk_mem = r.memory()
        r.submit(x)
        plain_runs = r.read_captures()
        plain_track = r.read_burst_tracks()
        r.drain()
    with api.Receiver(1, 0x2F, 500, 0, max_blocks=4, all_flushes=True, levels=True) as r:
        r.enable_capture(256, 4 * B)
        r.enable_burst_track(11)
        assert r.memory() == trk_mem  # a track without the call holds what it held
        r.enable_burst_sync(17240, WORD, 16, 1)
        m = r.memory()
        assert m["device_bytes"] - trk_mem["device_bytes"] == sync.device_bytes(1, 256, 4 * B)
        assert m["pinned_host_bytes"] - trk_mem["pinned_host_bytes"] == sync.pinned_bytes(1)
        r.enable_burst_clock()
        r.enable_burst_meter()
        r.enable_burst_envelope()
        r.submit(x)
        trecs, twords, decs, _ = read_track(r, 4, [0], 11, [0], None)
        got, words, _ = read_sync(r, st, None, trecs, twords)
        read_clock(r, 4, [0])  # the clock's records, exact
        env = read_envelope(r, 4, zeros(1), [0])[0]  # the envelope's
        bursts = r.read_bursts()
        tab = r.read_captures()
        ev = r.drain()
    with api.Receiver(1, 0x2F, 500, 0, max_blocks=4, all_flushes=True) as r:
        assert r.memory() == plain_mem  # a context without the call holds what it held
    assert bursts.tobytes() == burst.bursts(decs, tab[0], zeros(1)).tobytes() and len(bursts) == len(got) == 2
    assert np.array_equal(env["last_over"], trecs["last_over"])
    assert trecs.tobytes() == plain_track[0].tobytes() and twords.tobytes() == plain_track[1].tobytes()
    R.assert_tables(tab, plain_runs)
    assert parity.sort_events(ev).tobytes() == parity.sort_events(plain).tobytes() and len(ev) >= 1
    tch, sch = track.chains([(trecs, twords)]), sync.chains([(got, words)])
    assert [sync.plateaus(s.bits) for s in sch] == [[p] for p in PLATEAUS["tfa_2"]]
    lines = [sync.line("f", s, f) for t, s in zip(tch, sch) for f in sync.frames(t, s, st, 4)]
    assert lines == ["frame f 10003 10533 0 + 32 96070960", "frame f 25583 26113 0 + 32 98812225"]


def test_the_refusals():
    x = scene()[:3, :api.BLOCK_BYTES]
    with api.Receiver(3, CTX_TYPES, 500, 0, max_blocks=2) as r:
        raises(api.E_INVAL, r.enable_burst_sync, 17240, WORD, 16)  # no recorder, no track
        raises(api.E_INVAL, r.read_burst_syncs)
        r.enable_capture(64, 1024)
        raises(api.E_INVAL, r.enable_burst_sync, 17240, WORD, 16)  # the recorder alone: no track
        r.enable_burst_track(11)
        m = r.memory()
        for bad in ((999, WORD, 16), (96001, WORD, 16), (17240, WORD, 7), (17240, WORD, 65), (17240, WORD, 16, 8), (17240, WORD, 16, -1),
                    (4315, WORD, 25), (2 ** 31, WORD, 16), (17240, WORD, 2 ** 31)):
            raises(api.E_INVAL, r.enable_burst_sync, *bad)
        assert r.L.tfrec_amd_enable_burst_sync(r.h, 17240, WORD, 16, 0, 2) == api.E_INVAL  # an unknown flag
        assert r.memory() == m
        raises(api.E_INVAL, r.read_burst_syncs)  # not enabled
        r.enable_burst_sync(4315, 0xFFAA2DD4, 24, 11, True)  # span 2047, the largest E; the bits above P are ignored
        m2 = r.memory()
        assert m2["device_bytes"] - m["device_bytes"] == sync.device_bytes(3, 64, 1024) and m2["pinned_host_bytes"] == m["pinned_host_bytes"]
        raises(api.E_INVAL, r.enable_burst_sync, 17240, WORD, 16)  # a second call: refused, and nothing changes
        assert r.memory() == m2
        raises(api.E_STATE, r.read_burst_syncs)  # nothing undrained
        r.submit(x)
        nr, nw = api.C.c_uint32(0), api.C.c_uint64(0)
        buf = np.full(48, 0x55, dtype=np.uint8)  # the caller's room too small: E_INVAL, nothing written, the counts set
        f = r.L.tfrec_amd_read_burst_syncs
        assert f(r.h, buf.ctypes.data, 0, api.C.byref(nr), None, 0, api.C.byref(nw)) == api.E_INVAL and (buf == 0x55).all()
        trecs, twords = r.read_burst_tracks()
        assert nr.value == len(trecs) == len(r.read_captures()[0]) == 1 and nw.value == len(twords)
        assert f(r.h, buf.ctypes.data, 1, api.C.byref(nr), None, 5, api.C.byref(nw)) == api.E_INVAL  # no words, yet room for some
        assert f(r.h, buf.ctypes.data, 1, api.C.byref(nr), None, 0, api.C.byref(nw)) == api.E_OK  # the records alone
        got, words, _ = read_sync(r, sync.Settings(4315, 0xAA2DD4, 24, 11, True), None, trecs, twords)
        assert buf.tobytes() == got.tobytes()
        r.drain()
    with api.Receiver(3, CTX_TYPES, 500, 0, max_blocks=2) as r:
        r.enable_capture(64, 1024)
        r.enable_burst_track(11)
        r.submit(x)
        raises(api.E_STATE, r.enable_burst_sync, 17240, WORD, 16)  # after the first submit
        r.drain()


def test_a_submit_runs_replay_gives_the_recordings_sync():
    """The golden TFA_2 scene recorded by a u8 context (1 + 3 blocks) and replayed through sparse submits (2 + 2)."""
    x = golden_iq()
    L = 11
    st = sync.Settings(17240, WORD, 16, 1)
    with api.Receiver(1, 0x2F, 500, 0, max_blocks=3, all_flushes=True, levels=True) as r:
        r.enable_capture(256, 4 * B)
        r.enable_capture_pre()
        r.enable_burst_track(L)
        r.enable_burst_sync(17240, WORD, 16, 1)
        tabs, recs, pos, tst, sst = [], [], 0, None, None
        for p, nb in zip(parity.cut(x, (1, 3)), (1, 3)):
            r.submit(p)
            tabs.append(r.read_captures(pre=True))
            g, w, _, tst = read_track(r, nb, [pos * B], L, [0], tst)
            sg, sw, sst = read_sync(r, st, sst, g, w)
            recs.append((sg, sw))
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
        r.enable_burst_sync(17240, WORD, 16, 1)
        rep, tst, sst = [], None, None
        for k in range(2):
            t, p, q = decin.rebase(runs, pool, pre, 2 * k * B, 2 * B)
            assert r.submit_runs(t, p, q, 2) == 2
            g, w, _, tst = read_track(r, 2, [2 * k * B], L, [0], tst, levels=False)
            sg, sw, sst = read_sync(r, st, sst, g, w)
            rep.append((sg, sw))
            r.drain()
    a, b = sync.chains(recs), sync.chains(rep)
    assert len(a) == len(b) == 2
    same_chains("sync", b, a, "the replay")
    assert all(u.bits.any() for u in a)


# ---- tfrec_gpu -G -Y
def test_cli_frame_lines_of_the_golden_tfa_2_scene_cut_into_three_batches(tmp_path):
    parity.build_cli()
    x, bits = shifted_tfa_2()  # both telegrams lie across a batch boundary
    f = str(tmp_path / "tfa2.iq")
    x.tofile(f)
    bits = [ln % f for ln in bits]
    base = ["-T", "2f", "-t", "500", "-b", "2"]
    either = ("bits", "frame")  # both kinds of line, in the order they were printed
    plain = cli_lines(["-G", "17240"] + base + ["-L", f], either)
    assert plain[either] == bits
    got = cli_lines(["-G", "17240", "-Y", "2dd4,0,4"] + base + ["-L", f], either, "bits", "frame")
    assert got["telegrams"] == plain["telegrams"] and got["bits"] == bits
    assert [ln.split()[0] for ln in got[either]] == ["bits", "frame", "bits", "frame"]
    frames = [ln.split() for ln in got["frame"]]
    assert [fr[7] for fr in frames] == list(PAYLOADS["tfa_2"]) and all(fr[1] == f and fr[4:7] == ["0", "+", "32"] for fr in frames)
    for fr, b, p in zip(frames, bits, PLATEAUS["tfa_2"]):
        assert fr[2] == b.split()[2] and int(fr[3]) - int(fr[2]) == (p[0] + p[1]) >> 1
    # the complemented word: the same frames, read as -, bit for bit the complement
    both = cli_lines(["-Y", "d22b,1,4,1", "-G", "17240"] + base + ["-L", f], "frame")
    assert [ln.split()[4:] for ln in both["frame"]] == [["0", "-", "32", "%08x" % (int(p, 16) ^ 0xFFFFFFFF)] for p in PAYLOADS["tfa_2"]]
