"""The burst demodulator (tfrec_amd_enable_burst_demod, include/tfrec_amd.h: tfrec_amd_demod) restated in numpy -- no GPU
needed.  Written from the header's definition alone; exact integers throughout.

Per run of the recorder's table one int16 soft decision per symbol: the burst correlator's soft sample summed over each symbol (or
the difference of a Manchester bit's two chips), at a symbol timing measured on the chain's first piece.  Nothing here has been
measured on real recordings.

  Settings           the rate, the code and the centre, checked as the enable call checks them, with b, g, Pn and Nt;
  demods             vectorised, on prefix sums: one submit's records and decision pool from every stream's decimated samples, its run
                     table, the pair ahead of every stream's first sample and the state the submit before left;
  demods_bruteforce  the same position by position, in Python integers, as the header words it;
  time_phase, decide the timing and the decisions of a soft sequence (what both are made of);
  decisions_of       a record's decisions out of its submit's pool;  Piece, merge, chains: the merged bursts (burst.chains' walk);
  bits, line         the hard bits;  tfrec_gpu -w's output line;
  device_bytes       what tfrec_amd_enable_burst_demod adds to tfrec_amd_get_memory (pinned_bytes: nothing).
"""
from __future__ import annotations

import numpy as np

from . import burst, corr
from .capture import RUN_CONTINUES, RUN_OPEN

SPAN = 384  # a decision's samples at the most; the soft samples carried from submit to submit
HEAD = 8192  # the timed decisions end within HEAD samples behind the phase
MAX_TIMED, MIN_TIMED = 64, 8
KEEP = 2048  # the hard bits of a line
NONE, MEASURED, FLAGGED, INHERITED = 0, 1, 2, 3
DEMOD_DTYPE = np.dtype([("stream", "<u4"), ("flags", "<u4"), ("start_sample", "<i8"), ("n_samples", "<u4"), ("thresh", "<i4"),
                        ("phase", "<u4"), ("timing", "<u4"), ("n_timed", "<u4"), ("n_symbols", "<u4"), ("e_best", "<u8"),
                        ("e_sum", "<u8"), ("first_symbol", "<u8"), ("pool_offset", "<u8")])
assert DEMOD_DTYPE.itemsize == 72


class Settings:
    """What tfrec_amd_enable_burst_demod fixes; a ValueError where it returns E_INVAL."""

    def __init__(self, rate: int, code: str = "nrz", centre_hz: int = 0):
        self.rate, self.code, self.centre_hz = int(rate), code, int(centre_hz)
        if code not in ("nrz", "man"):
            raise ValueError("code %r is neither nrz nor man" % (code,))
        self.man = code == "man"
        if not 1000 <= self.rate <= (48000 if self.man else 96000):
            raise ValueError("rate %d outside 1000 .. 96000 (man: 48000)" % self.rate)
        if abs(self.centre_hz) > 192000:
            raise ValueError("centre %d Hz outside +-192000" % self.centre_hz)
        self.c = (self.centre_hz + 3000) // 6000  # (Python's //: a true floor)
        self.Rc = 2 * self.rate if self.man else self.rate
        self.Pn = -(-384000 // self.rate)
        self.Nt = max(N for N in range(MAX_TIMED + 1) if self.g(N) <= HEAD)

    def b(self, i: int) -> int:
        return 384000 * int(i) // self.Rc

    def g(self, j: int) -> int:
        return 384000 * int(j) // self.rate

    def ended(self, x: int, p: int) -> int:
        """The decisions that end ahead of chain sample x: the m >= 1 with p + g(m) <= x."""
        return 0 if x < p else ((x - p + 1) * self.rate - 1) // 384000


def fresh_state(n_streams: int) -> dict:
    """What a context carries before its first submit: nothing."""
    return {"soft": [np.zeros(SPAN, dtype=np.int64) for _ in range(n_streams)], "ahead": [0] * n_streams, "phase": [0] * n_streams}


def _spans(st: Settings, j0: int, j1: int, p: int):
    """The decisions j0 .. j1 - 1 under the phase p -> their first samples, their middles (the second chip's first) and their ends."""
    j = np.arange(j0, j1, dtype=object)  # (Python integers: a chain may be long)
    lo, hi = p + 384000 * j // st.rate, p + 384000 * (j + 1) // st.rate
    mid = p + 384000 * (2 * j + 1) // (2 * st.rate) if st.man else hi
    return lo.astype(np.int64), mid.astype(np.int64), hi.astype(np.int64)


def decide(u, st: Settings, p: int, j0: int, j1: int, origin: int = 0) -> np.ndarray:
    """D_j0 .. D_j1-1 of the soft samples u, whose first is the chain's sample `origin`, on their prefix sum (int64)."""
    P = np.concatenate([[0], np.cumsum(np.asarray(u, dtype=np.int64))])
    lo, mid, hi = _spans(st, j0, j1, p)
    lo, mid, hi = lo - origin, mid - origin, hi - origin
    return 2 * P[mid] - P[lo] - P[hi] if st.man else P[hi] - P[lo]


def _decide_brute(u, st, p, j0, j1, origin=0):
    ul = [int(v) for v in u]
    out = []
    for j in range(j0, j1):
        if st.man:
            out.append(sum(ul[p + st.b(2 * j) - origin:p + st.b(2 * j + 1) - origin]) - sum(ul[p + st.b(2 * j + 1) - origin:p + st.b(2 * j + 2) - origin]))
        else:
            out.append(sum(ul[p + st.b(j) - origin:p + st.b(j + 1) - origin]))
    return np.array(out, dtype=np.int64)


def time_phase(u, st: Settings, each=decide):
    """The timing of a chain's first piece u -> (p*, timing, Ns, E[p*], the sum of E)."""
    n = len(u)
    ns = sum(1 for j in range(st.Nt) if st.Pn - 1 + st.g(j + 1) <= n)
    if ns < MIN_TIMED:
        return 0, FLAGGED, ns, 0, 0
    u = u[:st.Pn - 1 + st.g(ns)]  # (what the phases reach)
    E =[int(np.abs(each(u, st, p, 0, ns)).sum()) for p in range(st.Pn)]
    best = max(range(st.Pn), key=lambda p: (E[p], -p))  # the first of the largest
    return best, MEASURED, ns, E[best], sum(E)


def _walk(dec, runs, prev, st, state, n_streams, max_samples, base, each, brute):
    if n_streams is None:
        n_streams = len(state["soft"]) if state is not None else len(dec)
    state = fresh_state(n_streams) if state is None else state
    nxt = fresh_state(n_streams)
    out = np.zeros(len(runs), dtype=DEMOD_DTYPE)
    pairs, fits = 0, True
    for r in runs:  # the prefix of whole runs that fit the pool
        fits = fits and (max_samples is None or int(r["pool_offset"]) + int(r["n_samples"]) <= max_samples)
        if fits:
            pairs = int(r["pool_offset"]) + int(r["n_samples"])
    pool = np.zeros(pairs, dtype=np.int16)
    for e, r in enumerate(runs):
        s, n, at = int(r["stream"]), int(r["n_samples"]), int(r["pool_offset"])
        o = out[e]
        for f in ("stream", "flags", "start_sample", "n_samples", "thresh", "pool_offset"):
            o[f] = r[f]
        if at + n > pairs:
            continue  # not looked at
        z = np.asarray(dec[s]).reshape(-1, 2).astype(np.int64)
        a = int(r["start_sample"]) - (int(base[s]) if base is not None else 0)
        assert 0 <= a and a + n <= len(z) and n >= 1
        cont = bool(int(r["flags"]) & RUN_CONTINUES)
        u = corr.soft(z, a, n, prev[s], cont, st.c)
        if cont:
            A, p, h = state["ahead"][s], state["phase"][s], state["soft"][s]
            o["phase"], o["timing"] = p, INHERITED
        else:
            A, h = 0, np.zeros(SPAN, dtype=np.int64)
            p, o["timing"], o["n_timed"], o["e_best"], o["e_sum"] = time_phase(u, st, each)
            o["phase"] = p
        ext = np.concatenate([h, u])  # the chain's samples A - 384 .. A + n - 1
        if brute:  # the decisions whose last sample lies in the piece, found one by one
            j0 = 0
            while p + st.g(j0 + 1) - 1 < A:
                j0 += 1
            j1 = j0
            while p + st.g(j1 + 1) - 1 < A + n:
                j1 += 1
        else:
            j0, j1 = st.ended(A, p), st.ended(A + n, p)
        d = each(ext, st, p, j0, j1, A - SPAN)
        assert len(d) <= n and (np.abs(d) <= 64 * SPAN).all()
        o["first_symbol"], o["n_symbols"] = j0, j1 - j0
        pool[at:at + len(d)] = d
        if int(r["flags"]) & RUN_OPEN:
            nxt["soft"][s], nxt["ahead"][s], nxt["phase"][s] = ext[-SPAN:], A + n, p
    return out, pool, nxt


def demods(dec, runs, prev, settings: Settings, state=None, n_streams=None, max_samples=None, base=None):
    """One submit.  dec[s], runs, prev[s], base[s]: as burst.bursts takes them (runs: RUN_DTYPE, with the entry's place in the pool);
    state: what the submit before returned (default: a fresh context's); max_samples: the pool's size (default: everything fits)
    -> (a DEMOD_DTYPE array, one record per table entry; the int16 decision pool; the state behind the submit)."""
    return _walk(dec, runs, prev, settings, state, n_streams, max_samples, base, decide, False)


def demods_bruteforce(dec, runs, prev, settings: Settings, state=None, n_streams=None, max_samples=None, base=None):
    """The same, one sample at a time in Python integers: every chip a sum over its samples, every decision found by its last sample."""
    return _walk(dec, runs, prev, settings, state, n_streams, max_samples, base, _decide_brute, True)


def decisions_of(rec, pool) -> np.ndarray:
    """A record's decisions out of its submit's pool -> int16 [n_symbols]."""
    at = int(rec["pool_offset"])
    return np.asarray(pool, dtype=np.int16)[at:at + int(rec["n_symbols"])]


class Piece:
    """A record with its decisions; read like the record (burst.chains looks at stream and flags)."""

    def __init__(self, rec, dec):
        self.rec, self.dec = rec, np.asarray(dec, dtype=np.int16)

    def __getitem__(self, f):
        return self.rec[f]

    def __setitem__(self, f, v):
        self.rec[f] = v


def merge(pieces):
    """A chain of pieces (in order, as for burst.merge) -> one Piece, that of the uncut run where the first piece held the timing
    window: the decisions concatenated, n_samples and n_symbols added, everything else the first piece's; the flags as burst.merge's."""
    pieces = list(pieces)
    o = pieces[0].rec.copy()
    for p in pieces[1:]:
        assert p["stream"] == o["stream"] and int(p["flags"]) & RUN_CONTINUES
        o["n_samples"] = int(o["n_samples"]) + int(p["n_samples"])
        o["n_symbols"] = int(o["n_symbols"]) + int(p["n_symbols"])
    o["flags"] = (int(pieces[0]["flags"]) & RUN_CONTINUES) | (int(pieces[-1]["flags"]) & RUN_OPEN)
    return Piece(o, np.concatenate([p.dec for p in pieces]))


def chains(submits, restarts=None):
    """submits: one (records, pool) per submit, in order -> the merged bursts as Pieces, in burst.chains' order."""
    return burst.chains([[Piece(r, decisions_of(r, pool)) for r in recs] for recs, pool in submits], restarts, join=merge)


def bits(dec) -> list:
    """The hard bits: D > 0."""
    return [int(v > 0) for v in np.asarray(dec).tolist()]


def line(name: str, piece, settings: Settings) -> str:
    """tfrec_gpu -w: demod <file> <start_sample> <n_samples> <phase> <m|f|i> <quality_c|-> <n_symbols>[+] <hex|->: quality_c =
    floor(100 E[p*] Pn / sum of E) of a measured timing; the first 2048 hard bits, MSB first, the last nibble zero-padded (then the +
    behind n_symbols: there are more)."""
    rec = piece.rec
    q = "-"
    if int(rec["timing"]) == MEASURED and int(rec["e_sum"]):
        q = "%d" % (100 * int(rec["e_best"]) * settings.Pn // int(rec["e_sum"]))
    n = int(rec["n_symbols"])
    hard = bits(piece.dec[:KEEP])
    return "demod %s %d %d %d %s %s %d%s %s" % (name, int(rec["start_sample"]), int(rec["n_samples"]), int(rec["phase"]),
                                                "-mfi"[int(rec["timing"])], q, n, "+" if n > KEEP else "",
                                                "".join("%x" % int("".join(map(str, (hard + [0, 0, 0])[i:i + 4])), 2)
                                                        for i in range(0, len(hard), 4)) if hard else "-")


def device_bytes(n_streams: int, max_blocks: int, max_runs: int, max_samples: int) -> int:
    """What tfrec_amd_enable_burst_demod adds to tfrec_amd_get_memory's device bytes: per FIFO set the records and the int16 pool;
    once, the soft bytes, the tile list (a stream's runs hold at most 2 max_blocks whole tiles and a partial one each), the list of
    the runs to time, the two lengths, and per stream the carried 384 bytes, A and p*."""
    from .api import FIFO_DEPTH
    stage_cap = max_blocks * 8192 // 356 + 3
    return (FIFO_DEPTH * (max_runs * DEMOD_DTYPE.itemsize + 2 * max_samples) + max_samples + 8 * n_streams * (2 * max_blocks + stage_cap)
            + 4 * n_streams * stage_cap + 8 + n_streams * (SPAN + 8 + 4))


def pinned_bytes(n_streams: int) -> int:
    """... and to its page-locked bytes: nothing."""
    return 0
