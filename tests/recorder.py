"""The harness the recorder family's tests share: what touches a receiver, real or modelled -- the byte-for-byte comparisons of
records, words, tables and merged chains, the table of the five measurements on the run table (meter, envelope, clock, track,
sync), one read per measurement that holds the oldest undrained submit to its restatement on what the context itself returned,
the channel-rate receiver for hand-made rows, the aimed u8 scene's receiver and its one submit, and tfrec_gpu's lines picked by
their first word.  tests/recorder_rows.py holds the inputs; tests/recorder_campaign.py drives the reads with generated plans, on a
GPU and on a model of the receiver.  Imported as a plain module (`import recorder`); pytest does not rewrite its assertions, so
each carries its own message."""
import collections
import functools
import subprocess

import numpy as np
import pytest

import parity
import recorder_rows as RR
from tfrec_amd import api, burst, capture, clock, decin, envelope, sync, track

B = api.BLOCK_DEC
W = 694  # the largest window of -T 2f
T = 100  # the hand-made rows' threshold: their quiet parts stay below it (|I| + |Q| <= 80)
CONT, OPEN = capture.RUN_CONTINUES, capture.RUN_OPEN
TABLE_FIELDS = ("stream", "flags", "start_sample", "n_samples", "thresh")  # what every measurement's record repeats of its run

Stage = collections.namedtuple("Stage", "module dtype enable read total word")  # (the last four: api.Receiver's names, tfrec_gpu's line)
STAGES = {"meter": Stage(burst, burst.BURST_DTYPE, "enable_burst_meter", "read_bursts", "burst_total", "burst"),
          "envelope": Stage(envelope, envelope.ENVELOPE_DTYPE, "enable_burst_envelope", "read_burst_envelopes", "envelope_total", "extent"),
          "clock": Stage(clock, clock.CLOCK_DTYPE, "enable_burst_clock", "read_burst_clocks", "clock_total", "clock"),
          "track": Stage(track, track.TRACK_DTYPE, "enable_burst_track", "read_burst_tracks", "track_total", "bits"),
          "sync": Stage(sync, sync.SYNC_DTYPE, "enable_burst_sync", "read_burst_syncs", "sync_total", "frame")}


def raises(code, f, *a, **kw):
    with pytest.raises(api.TfrecAmdError) as e:
        f(*a, **kw)
    assert e.value.code == code, e.value


def zeros(n):
    return [np.zeros(2, dtype=np.int16)] * n


def last_pairs(decs):
    return [np.asarray(d).reshape(-1, 2)[-1] for d in decs]


# ---- the comparisons: byte for byte, and a message that says where
def same_records(got, want, label=""):
    """Byte for byte; the message names the first differing record and field."""
    assert got.dtype == want.dtype, "%s: records of dtype %s, want %s" % (label, got.dtype, want.dtype)
    assert len(got) == len(want), "%s: %d records, want %d" % (label, len(got), len(want))
    for f in want.dtype.names:
        bad = np.flatnonzero((got[f] != want[f]).reshape(len(got), -1).any(axis=1)) if len(got) else []
        assert len(bad) == 0, "%s: record %d field %s: got %s want %s" % (
            label, bad[0], f, got[f][bad[0]].tolist(), want[f][bad[0]].tolist())
    assert got.tobytes() == want.tobytes(), "%s: the records' bytes differ outside their fields" % label


def same_words(got, want, label=""):
    assert got.dtype == np.uint32 and len(got) == len(want), "%s: %d words of %s, want %d of uint32" % (label, len(got), got.dtype, len(want))
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, "%s: %d words differ, the first at %d: got %08x want %08x" % (label, len(bad), bad[0], got[bad[0]], want[bad[0]])


def table_of(recs):
    """The run table a submit's track or sync records repeat: their first 24 bytes and bit_offset."""
    t = np.zeros(len(recs), dtype=capture.RUN_DTYPE)
    for f in TABLE_FIELDS:
        t[f] = recs[f]
    t["pool_offset"] = recs["bit_offset"]
    return t


def same_table(got, runs, label=""):
    """The records repeat the run table's first len(got) entries in TABLE_FIELDS (a prefix is what an overflow delivers)."""
    assert len(got) <= len(runs), "%s: %d records repeat a table of %d runs" % (label, len(got), len(runs))
    for f in TABLE_FIELDS:
        bad = np.flatnonzero(got[f] != runs[f][:len(got)])
        assert len(bad) == 0, "%s: record %d repeats table field %s wrongly: %s, the table has %s" % (
            label, bad[0], f, got[f][bad[0]], runs[f][bad[0]])


def same_chains(m, got, want, label=""):
    """Measurement m's merged chains, in the same order on both sides, byte for byte; the track's and the sync's without a
    piece's place in its own submit's pool, and their bits."""
    assert len(got) == len(want), "%s %s: %d chains, want %d" % (label, m, len(got), len(want))
    for i, (a, b) in enumerate(zip(got, want)):
        if m in ("track", "sync"):
            strip = RR.stripped if m == "track" else RR.sync_stripped
            assert strip(a.rec) == strip(b.rec), "%s %s: chain %d: got %s want %s" % (label, m, i, strip(a.rec), strip(b.rec))
            assert np.array_equal(a.bits, b.bits), "%s %s: chain %d (stream %d from %d): bits" % (
                label, m, i, a["stream"], a["start_sample"])
        else:
            for f in a.dtype.names:
                assert np.array_equal(a[f], b[f]), "%s %s: chain %d (stream %d from %d) field %s: got %s want %s" % (
                    label, m, i, a["stream"], a["start_sample"], f, a[f].tolist(), b[f].tolist())
            assert a.tobytes() == b.tobytes(), "%s %s: chain %d: bytes outside the fields" % (label, m, i)


def assert_tables(got, want, label=""):
    """(run table, pool) against the restatement's."""
    (runs, pool), (wruns, wpool) = got, want
    assert runs.dtype == capture.RUN_DTYPE and pool.dtype == np.int16, "%s: a table of %s, a pool of %s" % (label, runs.dtype, pool.dtype)
    same_records(runs, wruns, label + " table")
    assert pool.shape == wpool.shape and np.array_equal(pool, wpool), "%s pool: %s pairs, want %s, the first difference at %s" % (
        label, pool.shape, wpool.shape, np.argwhere(pool != wpool)[:1].tolist() if pool.shape == wpool.shape else "-")


def pre_of(decs, runs, prev=None, base=0):
    return decin.pre_samples(np.stack([d.reshape(-1, 2) for d in decs]), runs, prev, base)


def same_events(a, b):
    a, b = parity.sort_events(a), parity.sort_events(b)
    assert len(a) == len(b), "%d events, want %d" % (len(a), len(b))
    assert a.tobytes() == b.tobytes(), "the events differ, the first at %s" % np.flatnonzero(a != b)[:1].tolist()


# ---- one submit read back: each measurement against its restatement on what the context itself returned
def submit_view(r, nb, decs=None, levels=True):
    """The oldest undrained submit of nb blocks -> (every stream's decimated samples, the run table, the thresholds): per block as
    the level meter reports them (levels), each stream's own fixed one (levels=False), or None where nothing needs them
    (levels=None).  decs: that submit's decimated samples where a later submit is queued behind it (tfrec_amd_read_decimated
    returns the last submit's)."""
    n = r.n_streams
    if decs is None:
        decs = [r.decimated(s, nb * B) for s in range(n)]
    runs = r.read_captures(allow_overflow=True)[0]
    if levels:  # the threshold in force in every block, as the level meter reports it
        lev = r.read_levels()
        thr = [np.repeat(lev[s]["thresh"].astype(np.int64), B) for s in range(n)]
    else:  # a fixed threshold: the run's own
        thr = [int(r.thresh(s)) for s in range(n)] if levels is not None else None
    return decs, runs, thr


def _read(r, m, runs, overflow):
    """Measurement m's read of the oldest undrained submit.  Where the recorder did not overflow, it has a record for every run,
    its total says so, and the records repeat the table."""
    got = getattr(r, STAGES[m].read)(allow_overflow=overflow)
    recs, total = got[0] if isinstance(got, tuple) else got, getattr(r, STAGES[m].total)
    assert recs.dtype == STAGES[m].dtype, "%s: records of dtype %s" % (m, recs.dtype)
    if not r.capture_overflow:
        assert len(runs) == len(recs) == total, "%s: %d records and a total of %d for %d runs" % (m, len(recs), total, len(runs))
        same_table(recs, runs, m)
    return got


def read_meter(r, nb, prev, base, overflow=False, decs=None):
    """The oldest undrained submit's meter records against the restatement -> (records, decimated samples, the run table)."""
    decs, runs, _ = submit_view(r, nb, decs, levels=None)
    got = _read(r, "meter", runs, overflow)
    same_records(got, burst.bursts(decs, got[list(TABLE_FIELDS)], prev, base=base), "meter")
    assert (got["hist"].sum(axis=1) == got["n_products"]).all(), "meter: a record's histogram does not sum to its products"
    return got, decs, runs


def read_envelope(r, nb, prev, base, levels=True, overflow=False, decs=None):
    """... the envelope records -> (records, decimated samples, the run table)."""
    decs, runs, thr = submit_view(r, nb, decs, levels)
    got = _read(r, "envelope", runs, overflow)
    same_records(got, envelope.envelopes(decs, thr, got[list(TABLE_FIELDS)], prev, base=base), "envelope")
    return got, decs, runs


def read_clock(r, nb, base, overflow=False, decs=None):
    """... the clock records -> (records, decimated samples, the run table)."""
    decs, runs, _ = submit_view(r, nb, decs, levels=None)
    got = _read(r, "clock", runs, overflow)
    same_records(got, clock.clocks(decs, got[list(TABLE_FIELDS)], base=base), "clock")
    return got, decs, runs


def read_track(r, nb, base, L, centres, state, overflow=False, decs=None, levels=True):
    """... the track records and words -> (records, words, decimated samples, the state behind the submit)."""
    decs, runs, thr = submit_view(r, nb, decs, levels)
    got, words = _read(r, "track", runs, overflow)
    if not r.capture_overflow:
        assert np.array_equal(got["bit_offset"], runs["pool_offset"]), "track: bit_offset is not the run's pool_offset"
    want, wwords, state = track.tracks(decs, thr, table_of(got), L, centres, state, base=base, max_samples=r._capture[1])
    same_records(got, want, "track")
    same_words(words, wwords, "track")
    return got, words, decs, state


def read_amp(r, nb, base, L, lv, state, overflow=False, decs=None, levels=True):
    """The oldest undrained submit's track records and words against amplitude_tracks on what the context itself returned ->
    (records, words, decimated samples, the state behind the submit)."""
    decs, runs, thr = submit_view(r, nb, decs, levels)
    got, words = _read(r, "track", runs, overflow)
    if not r.capture_overflow:
        assert np.array_equal(got["bit_offset"], runs["pool_offset"]), "track: bit_offset is not the run's pool_offset"
    want, wwords, state = track.amplitude_tracks(decs, thr, table_of(got), L, lv, state, base=base, max_samples=r._capture[1])
    same_records(got, want, "amplitude track")
    same_words(words, wwords, "amplitude track")
    return got, words, decs, state


def _read_centres(r, got, overflow, label):
    cen = r.read_burst_track_centres(allow_overflow=overflow)
    assert cen.dtype == track.CENTRE_DTYPE and len(cen) == len(got) and r.centre_total == r.track_total, (
        "%s: %d records of %s for %d track records, totals %d and %d" % (label, len(cen), cen.dtype, len(got), r.centre_total, r.track_total))
    same_table(cen, table_of(got), label)  # (the track's records repeat the table: _read; a full pool cuts the table short, not the records)
    return cen


def read_auto(r, nb, base, L, K, fb, state, overflow=False, decs=None, levels=True):
    """The oldest undrained submit's centre records, track records and words against auto_tracks on what the context itself
    returned -> (centre records, track records, words, decimated samples, the state behind the submit)."""
    decs, runs, thr = submit_view(r, nb, decs, levels)
    got, words = _read(r, "track", runs, overflow)
    cen = _read_centres(r, got, overflow, "centre")
    wcen, want, wwords, state = track.auto_tracks(decs, thr, table_of(got), L, K, fb, state, base=base, max_samples=r._capture[1])
    same_records(cen, wcen, "centre")
    same_records(got, want, "auto-centre track")
    same_words(words, wwords, "auto-centre track")
    assert np.array_equal(cen["index"], [track.index_of(h) for h in cen["centre_hz"]]) and not cen["reserved"].any(), "centre: index or reserved"
    return cen, got, words, decs, state


def read_phase(r, nb, base, L, m, K, fb, state, overflow=False, decs=None, levels=True):
    """The oldest undrained submit's carrier records, track records and words against phase_tracks on what the context itself
    returned -> (carrier records, track records, words, decimated samples, the state behind the submit)."""
    decs, runs, thr = submit_view(r, nb, decs, levels)
    got, words = _read(r, "track", runs, overflow)
    cen = _read_centres(r, got, overflow, "carrier")
    wcen, want, wwords, state = track.phase_tracks(decs, thr, table_of(got), L, m, K, fb, state, base=base, max_samples=r._capture[1])
    same_records(cen, wcen, "carrier")
    same_records(got, want, "phase track")
    same_words(words, wwords, "phase track")
    assert not cen["reserved"].any() and not cen["deviation_hz"].any(), "carrier: reserved or deviation_hz"
    return cen, got, words, decs, state


# ---- the track's modes: None (the frequency track about a set centre), ("amplitude", levels), ("auto", K), ("phase", K, lag)
def mode_tracks(mode, decs, thr, runs, L, centres, state=None, base=None, max_samples=None, brute=False):
    """One submit's restatement in the track's mode -> (centre records or None, track records, words, the state behind the submit:
    the track's alone, or (the track's, the centres') in the modes that have centre records).  centres: the set centres, which
    are the fallbacks of auto and phase; the amplitude mode has the mode's own levels in their place."""
    kw = dict(base=base, max_samples=max_samples)
    if mode is None:
        return (None,) + (track.tracks_bruteforce if brute else track.tracks)(decs, thr, runs, L, centres, state, **kw)
    if mode[0] == "amplitude":
        return (None,) + (track.amplitude_tracks_bruteforce if brute else track.amplitude_tracks)(decs, thr, runs, L, mode[1], state, **kw)
    if mode[0] == "auto":
        return track.auto_tracks(decs, thr, runs, L, mode[1], centres, state, brute=brute, **kw)
    return (track.phase_tracks_bruteforce if brute else track.phase_tracks)(decs, thr, runs, L, mode[2], mode[1], centres, state, **kw)


def enable_mode(r, mode, L):
    if mode is None:
        r.enable_burst_track(L)
    elif mode[0] == "amplitude":
        r.enable_burst_track_amplitude(L)
    elif mode[0] == "auto":
        r.enable_burst_track_auto(L, mode[1])
    else:
        r.enable_burst_track_phase(L, mode[1], mode[2])


def read_mode(r, mode, nb, base, L, centres, state, overflow=False, decs=None, levels=True):
    """read_track, read_amp, read_auto or read_phase by the mode -> (centre records or None, records, words, decimated samples,
    the state behind the submit)."""
    kw = dict(overflow=overflow, decs=decs, levels=levels)
    if mode is None:
        return (None,) + read_track(r, nb, base, L, centres, state, **kw)
    if mode[0] == "amplitude":
        return (None,) + read_amp(r, nb, base, L, mode[1], state, **kw)
    if mode[0] == "auto":
        return read_auto(r, nb, base, L, mode[1], centres, state, **kw)
    return read_phase(r, nb, base, L, mode[2], mode[1], centres, state, **kw)


def read_sync(r, st, state, trecs, twords, overflow=False):
    """The oldest undrained submit's sync records and words against the restatement on the track records and words the context
    returned for it -> (records, words, the state behind the submit)."""
    got, words = r.read_burst_syncs(allow_overflow=overflow)
    assert got.dtype == sync.SYNC_DTYPE, "sync: records of dtype %s" % got.dtype
    if not r.capture_overflow:
        assert len(got) == len(trecs) == r.sync_total, "sync: %d records and a total of %d for %d track records" % (
            len(got), r.sync_total, len(trecs))
    want, wwords, state = sync.syncs(trecs, twords, st, state, r.n_streams, max_samples=r._capture[1])
    same_records(got, want, "sync")
    same_words(words, wwords, "sync")
    assert len(got) == len(trecs), "sync: %d records for %d track records" % (len(got), len(trecs))
    same_table(got, trecs, "sync")
    assert np.array_equal(got["bit_offset"], trecs["bit_offset"]), "sync: bit_offset is not the track record's"
    return got, words, state


# ---- receivers
def enable(r, stages):
    """stages: the measurements' names, or {name: the enable call's arguments}."""
    for m in stages:
        getattr(r, STAGES[m].enable)(*(stages[m] if isinstance(stages, dict) else ()))


def hand_receiver(n, nb, stages, thresh=T, cap=None, levels=True, **kw):
    """A channel-rate context for hand-made rows with the recorder and `stages` (see enable); the pool holds every pair where a
    track needs it and nothing otherwise."""
    r = api.Receiver(n, 0x2F, thresh, 0, max_blocks=nb, decimated=True, levels=levels, **kw)
    r.enable_capture(*(cap or (32 * n, n * nb * B if "track" in stages else 1)))
    enable(r, stages)
    return r


def receiver(max_blocks=RR.NB, cap=(4096, RR.N * RR.M), n=RR.N, **kw):
    """The aimed u8 scene's context; n > N: stream s is set up for the scene's row s mod N."""
    r = api.Receiver(n, RR.CTX_TYPES, 500, 0, max_blocks=max_blocks, all_flushes=True, **kw)
    own = [s for s in range(n) if s % RR.N in (2, 6, 7)]
    r.configure_streams(own, types_mask=[RR.TYPES[s % RR.N] for s in own], thresh=[RR.THRESH[s % RR.N] for s in own])
    if cap:
        r.enable_capture(*cap)
    return r


@functools.lru_cache(maxsize=None)
def one_submit(serial=False):
    """-> ((table, pool), the restatement's, events, every stream's decimated samples, thresholds read back, the final states)."""
    with receiver(serial_chains=serial) as r:
        r.submit(RR.scene())
        decs = [r.decimated(s, RR.M) for s in range(RR.N)]
        got = r.read_captures()
        assert r.capture_totals == (len(got[0]), len(got[1])) and not r.capture_overflow, "totals %s overflow %s for %d runs, %d pairs" % (
            r.capture_totals, r.capture_overflow, len(got[0]), len(got[1]))
        again = r.read_captures()  # reading pops nothing
        assert again[0].tobytes() == got[0].tobytes() and again[1].tobytes() == got[1].tobytes(), "a second read differs"
        ev = r.drain()
        th = [r.thresh(s) for s in range(RR.N)]
    states = [None] * RR.N
    want = RR.want_tables(decs, states)
    return got, want, ev, decs, th, states


# ---- tfrec_gpu
def pick(stdout, *words):
    """-> {word: the lines that start with the word and a space, "telegrams": parity.telegram_lines}; a word given as a tuple of
    words takes the lines of any of them, in the order of the output."""
    starts = {w: tuple(v + " " for v in ((w,) if isinstance(w, str) else w)) for w in words}
    out = {w: [ln for ln in stdout.splitlines() if ln.startswith(starts[w])] for w in words}
    out["telegrams"] = parity.telegram_lines(stdout)
    return out


def cli_lines(args, *words, timeout=300):
    out = subprocess.run([parity.CLI] + args, capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stderr
    return pick(out.stdout, *words)
