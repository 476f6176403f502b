"""Randomised exact-parity campaign for the squelched recorder and the four measurements on its run table: the burst meter, the
envelope, the clock and the track (capture.h, burst.h, envelope.h, clock.h, track.h).  Random stream counts, masks (per context and
per stream), cuts, submits in flight, resets, tight recorder caps and subsets of the measurements; rows made by hand so that every
run's edges are known and land on the kernels' own strides.  Every comparison is byte for byte with the restatements in
tfrec_amd/{capture,levels,burst,envelope,clock,track}.py; nothing here has a tolerance.
    python tests/recorder_campaign.py <seed> <rounds>      (tests/test_recorder_campaign_gpu.py runs a short fixed campaign,
                                                            tests/test_recorder_campaign_cpu.py holds the generator to its classes)

The rows are channel-rate input (tfrec_amd_create_decimated): int16 pairs on a quiet floor (|I| + |Q| <= 80 under a threshold of
100).  A stretch of over-threshold samples from a to l gives the run [a, l + W), W the stream's largest window.  The edge classes a
row is built from (classes_hit() measures them back from capture.captures on the rows):

   1  start and end = 0, 1, 31, 32, 33, 63 mod 64          7  a run that ends one sample behind a submit cut
   2  start or end at a multiple of 256 and of 1024, +-1   8  a run from ahead of a submit cut through the whole next submit
   3  end == B, and end == B - 1                           9  two runs one uncaptured sample apart
   4  start == B                                          10  a trigger at exactly `end`: one run
   5  a run across a block boundary, 1 .. 16 ahead of it  11  a not-over gap of W - 1 inside a run: in a block, across a block
   6  the same at a submit cut                                boundary, across a submit cut
                                                          12  a run of 2046 samples from 1024 q + 1, and one of 2047
"""
import functools
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (_HERE, os.path.join(_HERE, "..")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import test_capture_gpu as TC  # noqa: E402
import test_clock_gpu as TK  # noqa: E402
import test_envelope_gpu as TE  # noqa: E402
import test_track_gpu as TT  # noqa: E402
from test_clock_cpu import keyed  # noqa: E402
from test_track_cpu import stripped  # noqa: E402
from tfrec_amd import api, burst, capture, clock, decin, envelope, levels, track  # noqa: E402

B = api.BLOCK_DEC
T = 100  # the rows' threshold: their quiet parts stay below it
EDGE64 = (0, 1, 31, 32, 33, 63)
CTX_MASKS = (0x02, 0x01, 0x20, 0x08, 0x2F)
MEASURES = ("meter", "envelope", "clock", "track")
MODULES = {"meter": burst, "envelope": envelope, "clock": clock, "track": track}
DENSE_PERIOD = 357  # a window of mask 0x02 (356) and the one uncaptured sample behind it
ZONE = 1100  # the samples ahead of a block boundary kept for the boundary's own item
TABLE_FIELDS = ("stream", "flags", "start_sample", "n_samples", "thresh")
SEEDS = (12, 19, 21, 24)  # the fixed campaign of tests/test_recorder_campaign_gpu.py: ROUNDS rounds each
ROUNDS = 6
quiet = TE.quiet


def window(mask):
    return max(levels.windows(mask))


# ---- the rows
@functools.lru_cache(maxsize=None)
def _tone(nb, period, seed):
    k = keyed(nb, period, seed=seed).reshape(-1, 2)
    k.setflags(write=False)
    return k


def _loud(rng, n):
    """n pairs of noise, every one over the threshold."""
    i = rng.integers(T + 1, 501, n) * rng.choice((-1, 1), n)
    return np.stack([i, rng.integers(-400, 401, n)], axis=1).astype(np.int16)


def _paint(rng, row, a, l, W, kind=None):
    """Over-threshold samples from a to l (both included); its first and last sample are over whatever the kind."""
    n = l - a + 1
    kinds = ("tone", "const", "noise", "full") + (("gappy",) if n >= 3 else ())
    kind = kind or kinds[int(rng.integers(len(kinds)))]
    if kind == "tone":  # keyed: the clock's and the track's signal
        row[a:l + 1] = _tone(len(row) // B, (10, 22, 64)[int(rng.integers(3))], (3, 4)[int(rng.integers(2))])[a:l + 1]
    elif kind == "const":  # every cross product is 0
        row[a:l + 1] = ((3000, 0), (0, -2500), (-2000, 2000))[int(rng.integers(3))]
    elif kind == "full":  # full scale, and -32768, which the channel-rate input clamps
        row[a:l + 1, 0] = rng.choice((32767, -32768), n)
        row[a:l + 1, 1] = rng.choice((32767, -32768, -32767, 0), n)
    else:
        floor = row[a:l + 1].copy()
        row[a:l + 1] = _loud(rng, n)
        if kind == "gappy":  # not-over gaps inside the stretch, the longest below W
            for top in (min(W - 1, n - 2), min(8, n - 2), min(64, n - 2)):
                g = int(rng.integers(1, top + 1))
                o = int(rng.integers(1, n - g))
                row[a + o:a + o + g] = floor[o:o + g]


def _len(rng):
    return int((1, rng.integers(2, 41), rng.integers(41, 301))[int(rng.integers(3))])


def _up(x, m, r):
    """The smallest y >= x with y = r mod m."""
    return x + (r - x) % m


def _interior(rng, pos, lim, W):
    """One item of the classes that need no boundary: its first over sample at or behind pos, its last run's end at or ahead of lim
    -> [(first, last over sample)] of its stretches, or None where it does not fit."""
    c = int(rng.integers(7))
    if c == 0:  # class 1
        a = _up(pos, 64, EDGE64[int(rng.integers(6))])
        st = [(a, _up(a + _len(rng) - 1 + W, 64, EDGE64[int(rng.integers(6))]) - W)]
    elif c == 1:  # class 2
        m, d = (256, 1024)[int(rng.integers(2))], int(rng.integers(-1, 2))
        if rng.integers(2):
            a = _up(pos, m, d)
            st = [(a, a + _len(rng) - 1)]
        else:
            st = [(pos, _up(pos + _len(rng) - 1 + W, m, d) - W)]
    elif c == 2:  # class 9: the next trigger at end + 1
        l = pos + _len(rng) - 1
        st = [(pos, l), (l + W + 1, l + W + _len(rng))]
    elif c == 3:  # class 10: one over sample at exactly `end`
        l = pos + _len(rng) - 1
        st = [(pos, l), (l + W, l + W)]
    elif c == 4:  # class 11, inside a block
        l = pos + _len(rng) - 1
        st = [(pos, l), (l + W, l + W + _len(rng) - 1)]
    elif c == 5:  # class 12
        a = _up(pos, 1024, 1)
        st = [(a, a + 2046 + int(rng.integers(2)) - W)]
    else:
        st = [(pos, pos + _len(rng) - 1)]
    return st if st[-1][1] + W <= lim else None


def _boundary(rng, P, W, end, cut=False):
    """One item at the block boundary P (end: P is the row's end; cut: a submit cut, where the classes that need one are drawn more
    often) -> its stretches, [] for none."""
    n = _len(rng)
    if end:
        c = int(rng.integers(5))
        if c == 0:
            return []
        if c in (1, 2):  # class 3 at the row's end
            l = P - W - (c - 1)
            return [(l - n + 1, l)]
        d = (1, 2, 3, 5, 16, 100)[int(rng.integers(6))]  # a run open over the last d samples
        return [(P - d, int(rng.integers(P - d, P)))]
    c = int(rng.integers(4, 7)) if cut and rng.integers(2) else int(rng.integers(7))
    if c == 0:
        return []
    if c in (1, 2):  # class 3: end == P, end == P - 1
        l = P - W - (c - 1)
        return [(l - n + 1, l)]
    if c == 3:  # class 4
        return [(P, P + n - 1)]
    if c == 4:  # classes 5 and 6
        a = P - int(rng.integers(1, 17))
        return [(a, a + n - 1)]
    if c == 5:  # class 7: one sample behind P
        l = P + 1 - W
        return [(l - n + 1, l)]
    l = P - int(rng.integers(2, W))  # class 11 across P: the gap's W - 1 samples lie on both sides of it
    return [(l - n + 1, l), (l + W, l + W + _len(rng) - 1)]


def _fill_row(rng, row, W, cuts):
    nb = len(row) // B
    E = nb * B
    marks = sorted(set(cuts) | {nb})
    free = 0  # the first sample a new stretch may begin at: one uncaptured sample behind the run ahead of it
    k = 0
    while k < nb:
        P = (k + 1) * B
        pos = free if rng.integers(2) else free + int(rng.integers(1, 400))
        for _ in range(12):  # the block's interior
            st = _interior(rng, pos, P - ZONE, W)
            if st is None:
                continue
            for a, l in st:
                _paint(rng, row, a, l, W)
            free = st[-1][1] + W + 1
            pos = free + int(rng.integers(0, 3)) * int(rng.integers(0, 300))
        if P < E and (k + 1) in cuts and rng.integers(6) == 0:  # class 8
            a = P - int(rng.integers(1, 600))
            P2 = B * min(m for m in marks if m > k + 1)
            if a >= free:
                l = P2 + int(rng.integers(0, 300)) if P2 < E else E - 1
                _paint(rng, row, a, l, W, ("tone", "noise")[int(rng.integers(2))])
                free = l + W + 1
                k = P2 // B
                continue
        for _ in range(3):
            st = _boundary(rng, P, W, P == E, (k + 1) in cuts)
            if not st or (st[0][0] >= free and st[-1][1] < E):
                break
            st = []
        for a, l in st:
            _paint(rng, row, a, l, W)
        if st:
            free = st[-1][1] + W + 1
        k += 1


def rows(rng, n_streams, n_blocks, windows, cuts=()):
    """int16 [n_streams, n_blocks B, 2] for a channel-rate context; windows[s]: stream s's W; cuts: the block indices at which the
    input will be cut into submits (the classes at a submit cut are placed there).  Pure numpy, deterministic in rng."""
    out = np.stack([quiet(n_blocks, int(rng.integers(1 << 30))) for _ in range(n_streams)])
    for s in range(n_streams):
        _fill_row(rng, out[s], int(windows[s]), set(int(c) for c in cuts))
    return out


def dense(n_blocks):
    """The densest legal input of mask 0x02 (W = 356): one over sample every 357 -> int16 [n_blocks B, 2].  Every run is 356 long
    and one uncaptured sample lies between two runs: 276 runs in 12 blocks."""
    row = quiet(n_blocks, 7)
    row[::DENSE_PERIOD] = (3000, -3000)
    return row


# ---- the classes, measured back from the restatement
def _labels():
    out = ["1:start:%d" % r for r in EDGE64] + ["1:end:%d" % r for r in EDGE64]
    out += ["2:%d:%+d" % (m, d) for m in (256, 1024) for d in (-1, 0, 1)]
    return out + ["3:B", "3:B-1", "4", "5", "6", "7", "8", "9", "10", "11:block", "11:boundary", "11:cut", "12:2046", "12:2047"]


CLASSES = tuple(_labels())


def classes_hit(x, masks, thresh, sizes):
    """The edge classes the rows x hold, from capture.captures on each uncut row and its over bits -> a set of CLASSES' labels.
    sizes: the submits' block counts."""
    hit = set()
    nb = x.shape[1] // B
    cuts = set(np.cumsum(sizes)[:-1].tolist())
    marks = sorted(cuts | {0, nb})
    for s in range(len(x)):
        W = window(masks[s])
        z = decin.clamp(x[s]).astype(np.int64)
        runs = capture.captures(decin.clamp(x[s]), masks[s], thresh[s])[0]
        a = runs["start_sample"].astype(np.int64)
        e = a + runs["n_samples"]
        for r in EDGE64:
            hit |= {"1:start:%d" % r} if (a % 64 == r).any() else set()
            hit |= {"1:end:%d" % r} if (e % 64 == r).any() else set()
        for m in (256, 1024):
            for d in (-1, 0, 1):
                if ((a % m == d % m) | (e % m == d % m)).any():
                    hit.add("2:%d:%+d" % (m, d))
        if (e % B == 0).any():
            hit.add("3:B")
        if (e % B == B - 1).any():
            hit.add("3:B-1")
        if ((a % B == 0) & (a > 0)).any():
            hit.add("4")
        P = (a // B + 1) * B  # the first boundary behind each start
        ahead = (P - a <= 16) & (e > P)
        is_cut = np.isin(P // B, sorted(cuts))
        if (ahead & ~is_cut & (P < nb * B)).any():
            hit.add("5")
        if (ahead & is_cut).any():
            hit.add("6")
        for c in cuts:
            if ((a < c * B) & (e == c * B + 1)).any():
                hit.add("7")
        for m0, m1 in zip(marks[1:], marks[2:]):
            if ((a < m0 * B) & (e >= m1 * B)).any():
                hit.add("8")
        if (a[1:] == e[:-1] + 1).any():
            hit.add("9")
        for n in (2046, 2047):
            if ((a % 1024 == 1) & (e - a == n)).any():
                hit.add("12:%d" % n)
        over = np.flatnonzero(np.abs(z[:, 0]) + np.abs(z[:, 1]) > thresh[s])
        for i in np.flatnonzero(np.diff(over) == W):  # W - 1 not-over samples between two over ones: one run
            lo, hi = int(over[i]), int(over[i + 1])
            P = (lo // B + 1) * B
            if lo + 1 < P < hi:  # not-over samples on both sides of P
                hit.add("11:cut" if P // B in cuts else "11:boundary")
            else:
                hit.add("11:block")
                if i + 2 == len(over) or over[i + 2] > hi + 1:
                    hit.add("10")
    return hit


# ---- one round's plan: everything that is drawn, and what the restatements expect of it
def restate(p, sizes, reset=None, measure=()):
    """The restatements over the plan's rows cut into submits of `sizes` blocks, the streams of reset[1] restarted with submit
    reset[0] -> one dict per submit: the full table and pool (no caps), the level records, and the records of `measure`."""
    n, x = p["n"], p["dec"]
    cst, lst, base, prev, tst, pos, out = [None] * n, [None] * n, [0] * n, TE.zeros(n), None, 0, []
    for k, nb in enumerate(sizes):
        if reset and reset[0] == k:
            for s in reset[1]:
                cst[s] = lst[s] = None
                base[s] = 0
        decs = [np.ascontiguousarray(x[s, pos * B:(pos + nb) * B]).reshape(-1) for s in range(n)]
        per, lev = [], []
        for s in range(n):
            runs, pool, cst[s] = capture.captures(decs[s], p["masks"][s], p["thresh"][s], cst[s])
            per.append((runs, pool))
            rec, lst[s] = levels.levels(decs[s], p["masks"][s], p["thresh"][s], lst[s])
            lev.append(rec)
        table = capture.table(per)
        e = dict(nb=nb, decs=decs, base=list(base), prev=prev, table=table, levels=np.stack(lev))
        thr = [np.repeat(v["thresh"].astype(np.int64), B) for v in lev]
        if "meter" in measure:
            e["meter"] = burst.bursts(decs, table[0], prev, base=base)
        if "envelope" in measure:
            e["envelope"] = envelope.envelopes(decs, thr, table[0], prev, base=base)
        if "clock" in measure:
            e["clock"] = clock.clocks(decs, table[0], base=base)
        if "track" in measure:
            recs, words, tst = track.tracks(decs, thr, table[0], p["L"], p["centres"], tst, base=base)
            e["track"] = (recs, words)
        out.append(e)
        prev, pos, base = TE.last_pairs(decs), pos + nb, [v + nb * B for v in base]
    return out


def finish(p):
    """The derived parts of a plan: the clamped rows (a channel-rate context's own samples) and what every submit must give."""
    p["dec"] = decin.clamp(p["x"])
    p["windows"] = [window(m) for m in p["masks"]]
    p["expect"] = restate(p, p["sizes"], p.get("reset"))
    return p


def make_plan(x, ctx_mask, masks, sizes, L=5, centres=None, thresh=None, drains=None, reset=None, cap=None, measure=MEASURES):
    """A plan from its parts.  configured: the streams whose settings are not the context's (tfrec_amd_configure_streams)."""
    n = len(x)
    thresh = list(thresh or [T] * n)
    return finish(dict(n=n, nb=x.shape[1] // B, x=np.ascontiguousarray(x), ctx_mask=ctx_mask, masks=list(masks), sizes=tuple(sizes),
                       thresh=thresh, configured=[s for s in range(n) if masks[s] != ctx_mask or thresh[s] != T], L=L,
                       centres=list(centres or [0] * n), drains=list(drains or [None] * len(sizes)), reset=reset, cap=cap,
                       measure=tuple(measure)))


def full_cap(p):
    """Room for every run and pair a submit of the plan can hold."""
    mb = max(p["sizes"])
    return p["n"] * (mb * B // 356 + 3), p["n"] * mb * B


def _submasks(rng, ctx_mask):
    bits = [b for b in (0x01, 0x02, 0x04, 0x08, 0x20) if ctx_mask & b]
    while True:
        m = sum(b for b in bits if rng.integers(2))
        if m:
            return m


def plan(rng, rnd=0):
    """Draw one round."""
    kind = int(rng.integers(10))  # 0: the dense row alone, 12 blocks under mask 0x02; 1, 2: it is one stream beside ordinary rows
    if kind == 0:
        n, nb, ctx_mask = int(rng.integers(1, 4)), 12, 0x02
    else:
        n, nb, ctx_mask = int(rng.integers(1, 10)), int(rng.integers(2, 5)), int(rng.choice(CTX_MASKS))
        if kind <= 2:
            ctx_mask = 0x2F
    configure = bool(rng.integers(2))
    masks = [_submasks(rng, ctx_mask) if configure else ctx_mask for _ in range(n)]
    thresh = [int(rng.integers(80, T + 1)) if configure else T for _ in range(n)]  # the floor is at most 80: the same over bits
    n_sub = int(rng.integers(1, 5))
    if kind == 0 and rng.integers(2):  # uncut: more runs in one submit than a workgroup has lanes
        n_sub = 1
    cuts = sorted(set(int(c) for c in rng.integers(1, nb, size=n_sub - 1)))
    sizes = np.diff([0] + cuts + [nb]).tolist()
    at = None
    if kind == 0:
        x = np.stack([dense(nb)] * n)
    else:
        if 1 <= kind <= 2:
            at = int(rng.integers(n))
            masks[at] = 0x02
        x = rows(rng, n, nb, [window(m) for m in masks], cuts)
        if at is not None:
            x[at] = dense(nb)
    drains, pend = [], 0
    for _ in sizes:  # as stress_gpu.py: up to FIFO_DEPTH submits in flight, and sometimes the younger ones stay in flight
        pend += 1
        if pend == api.FIFO_DEPTH or rng.integers(2):
            pend = int(rng.integers(0, pend))
            drains.append(pend)
        else:
            drains.append(None)
    reset = None
    if len(sizes) >= 2 and rng.integers(3) == 0:
        streams = sorted(set(int(s) for s in rng.integers(0, n, size=int(rng.integers(1, n + 1)))))
        reset = (int(rng.integers(1, len(sizes))), streams)
    measure = MEASURES if rnd % 3 == 0 else tuple(m for m in MEASURES if rng.integers(2)) or (MEASURES[int(rng.integers(4))],)
    L = int((1, 16, rng.integers(1, 17))[int(rng.integers(3))])
    edge = rng.integers(8, size=n)  # the centre's limits and 0 now and then
    centres = [(-192000, 192000, 0)[e] if e < 3 else int(v) for e, v in zip(edge, rng.integers(-192000, 192001, size=n))]
    p = make_plan(x, ctx_mask, masks, sizes, L=L, centres=centres, thresh=thresh, drains=drains, reset=reset, measure=measure)
    if rng.integers(3) == 0:  # tight caps: a prefix is delivered
        tabs = [e["table"][0] for e in p["expect"]]
        k = int(np.argmax([len(t) for t in tabs]))
        t = tabs[k]
        if len(t) >= 2:
            if rng.integers(2):  # max_runs lands between two runs, of a middle stream where there is one
                mid = np.flatnonzero((t["stream"] > t["stream"][0]) & (t["stream"] < t["stream"][-1]))
                inner = mid[1:] if len(mid) >= 2 else np.arange(1, len(t))
                p["cap"] = (int(inner[int(rng.integers(len(inner)))]), full_cap(p)[1])
            else:  # max_samples lands inside a run
                r = t[int(rng.integers(len(t)))]
                p["cap"] = (full_cap(p)[0], int(r["pool_offset"]) + max(1, int(rng.integers(0, int(r["n_samples"])))))
    return p


def describe(p):
    return "streams %d blocks %d ctx %02x masks %s thresh %s sizes %s drains %s L %d centres %s reset %s cap %s measure %s" % (
        p["n"], p["nb"], p["ctx_mask"], ["%02x" % m for m in p["masks"]] if p["configured"] else "-",
        p["thresh"] if p["configured"] else "-", list(p["sizes"]), p["drains"], p["L"], p["centres"], p["reset"], p["cap"],
        ",".join(p["measure"]))


# ---- one plan on the GPU
def same_records(got, want, label):
    """Byte for byte; the message names the first differing record and field."""
    assert got.dtype == want.dtype and len(got) == len(want), "%s: %d records, want %d" % (label, len(got), len(want))
    for f in want.dtype.names:
        bad = np.flatnonzero((got[f] != want[f]).reshape(len(got), -1).any(axis=1))
        assert len(bad) == 0, "%s: record %d field %s: got %s want %s" % (
            label, bad[0], f, got[f][bad[0]].tolist(), want[f][bad[0]].tolist())
    assert got.tobytes() == want.tobytes(), label


def _same_table(got, runs, label):
    for f in TABLE_FIELDS:
        bad = np.flatnonzero(got[f] != runs[f][:len(got)]) if len(got) <= len(runs) else [0]
        assert len(bad) == 0, "%s: record %d repeats table field %s wrongly" % (label, bad[0], f)


def _check_submit(r, p, k, measure, tst, newest):
    """Every read of the oldest undrained submit, which is the plan's k-th -> (what was read, the track's state behind it)."""
    e = p["expect"][k]
    nb, decs, base, prev = e["nb"], e["decs"], e["base"], e["prev"]
    label = "submit %d" % k
    cap = p["cap"] or full_cap(p)
    wr, wp, over = capture.prefix(e["table"][0], e["table"][1], *cap)
    got = dict(table=r.read_captures(allow_overflow=True))
    assert r.capture_overflow == over and r.capture_totals == (len(e["table"][0]), len(e["table"][1])), "%s: totals %s overflow %s" % (
        label, r.capture_totals, r.capture_overflow)
    TC.assert_tables(got["table"], (wr, wp), label)  # independent of the context: the restatement on the generated rows
    got["levels"] = r.read_levels()
    for f in levels.LEVEL_DTYPE.names:
        assert np.array_equal(got["levels"][f], e["levels"][f]), "%s: levels field %s" % (label, f)
    if newest:  # (tfrec_amd_read_decimated returns the last submit's samples)
        for s in range(p["n"]):
            assert np.array_equal(r.decimated(s, nb * B), decs[s]), "%s: stream %d's decimated samples" % (label, s)
    full = e["table"][0][:cap[0]]
    if "meter" in measure:
        m = r.read_bursts(allow_overflow=over)
        assert r.burst_total == len(e["table"][0])
        _same_table(m, full, label + " meter")
        same_records(m, burst.bursts(decs, m[list(TABLE_FIELDS)], prev, base=base), label + " meter")
        got["meter"] = m
    if "envelope" in measure:
        got["envelope"] = TE.read_submit(r, nb, prev, base, overflow=over, decs=decs)[0]
        _same_table(got["envelope"], full, label + " envelope")
    if "clock" in measure:
        got["clock"] = TK.read_submit(r, nb, base, overflow=over, decs=decs)[0]
        _same_table(got["clock"], full, label + " clock")
    if "track" in measure:
        recs, words, _, nxt = TT.read_submit(r, nb, base, p["L"], p["centres"], tst, overflow=over, decs=decs)
        _same_table(recs, full, label + " track")
        if over:  # the chains' carried state is the whole table's, not the delivered prefix's
            thr = [np.repeat(v["thresh"].astype(np.int64), B) for v in e["levels"]]
            nxt = track.tracks(decs, thr, e["table"][0], p["L"], p["centres"], tst, base=base)[2]
        got["track"], tst = (recs, words), nxt
    for m in measure:
        n_rec = len(got[m][0] if m == "track" else got[m])
        assert n_rec == len(full), "%s %s: %d records of %d" % (label, m, n_rec, len(full))
    return got, tst


def merged(m, pieces, restarts=None):
    """A measurement's chains over the submits' pieces, by stream (within a stream: in the order of the samples)."""
    return sorted(MODULES[m].chains(pieces, restarts), key=lambda c: int(c["stream"]))


def same_chains(m, got, want, label):
    assert len(got) == len(want), "%s %s: %d chains, want %d" % (label, m, len(got), len(want))
    for i, (a, b) in enumerate(zip(got, want)):
        if m == "track":
            assert stripped(a.rec) == stripped(b.rec), "%s track: chain %d: got %s want %s" % (label, i, stripped(a.rec), stripped(b.rec))
            assert np.array_equal(a.bits, b.bits), "%s track: chain %d (stream %d from %d): bits" % (
                label, i, a["stream"], a["start_sample"])
        else:
            for f in a.dtype.names:
                assert np.array_equal(a[f], b[f]), "%s %s: chain %d (stream %d from %d) field %s: got %s want %s" % (
                    label, m, i, a["stream"], a["start_sample"], f, a[f].tolist(), b[f].tolist())
            assert a.tobytes() == b.tobytes()


def run_plan(p, measure=None, receiver=None):
    """The plan on a context: every submit's reads checked in FIFO order; behind the last submit, where the rows were cut and
    nothing overflowed, the merged chains against the restatement on the rows cut at the reset alone (uncut without one) -> one
    dict of reads per submit.  receiver: what makes the context (default: api.Receiver)."""
    measure = p["measure"] if measure is None else tuple(measure)
    n, sizes = p["n"], p["sizes"]
    with (receiver or api.Receiver)(n, p["ctx_mask"], T, 0, max_blocks=max(sizes), decimated=True, levels=True) as r:
        if p["configured"]:
            own = p["configured"]
            r.configure_streams(own, types_mask=[p["masks"][s] for s in own], thresh=[p["thresh"][s] for s in own])
        r.enable_capture(*(p["cap"] or full_cap(p)))
        for m in measure:
            {"meter": r.enable_burst_meter, "envelope": r.enable_burst_envelope, "clock": r.enable_burst_clock,
             "track": lambda: r.enable_burst_track(p["L"])}[m]()
        if "track" in measure:
            r.set_burst_track_centre(range(n), p["centres"])
        reads, tst, pos = [], None, 0
        for k, nb in enumerate(sizes):
            if p["reset"] and p["reset"][0] == k:
                r.reset_streams(p["reset"][1])
            r.submit(np.ascontiguousarray(p["x"][:, pos * B:(pos + nb) * B]))
            pos += nb
            keep = p["drains"][k] if k + 1 < len(sizes) else 0
            while keep is not None and k + 1 - len(reads) > keep:
                got, tst = _check_submit(r, p, len(reads), measure, tst, newest=len(reads) == k)
                reads.append(got)
                r.drain()
        TE.raises(api.E_STATE, r.read_captures)  # nothing undrained
    overflowed = any(capture.prefix(e["table"][0], e["table"][1], *(p["cap"] or full_cap(p)))[2] for e in p["expect"])
    if measure and len(sizes) > 1 and not overflowed:
        j = p["reset"][0] if p["reset"] else None
        blocks = int(np.sum(sizes[:j])) if j else 0
        ref = restate(p, (blocks, p["nb"] - blocks) if j else (p["nb"],), (1, p["reset"][1]) if j else None, measure)
        for m in measure:
            same_chains(m, merged(m, [g[m] for g in reads], {j: p["reset"][1]} if j else None),
                        merged(m, [e[m] for e in ref], {1: p["reset"][1]} if j else None), "chains")
    return reads


def _round(rng, rnd, verbose=True, seed=None, receiver=None):
    p = plan(rng, rnd)
    try:
        reads = run_plan(p, receiver=receiver)
        runs = sum(len(g["table"][0]) for g in reads)
    except AssertionError as e:
        print("seed %s round %d: %s -> MISMATCH: %s" % (seed, rnd, describe(p), e), flush=True)
        return 1
    if verbose:
        print("seed %s round %d: %s runs %d -> ok" % (seed, rnd, describe(p), runs), flush=True)
    return 0


def campaign(seed: int, rounds: int, verbose: bool = True, receiver=None) -> int:
    """-> the number of bad rounds."""
    rng = np.random.default_rng(seed)
    return sum(_round(rng, rnd, verbose, seed, receiver) for rnd in range(rounds))


def plans(seed: int, rounds: int):
    """The plans campaign(seed, rounds) draws, without a GPU."""
    rng = np.random.default_rng(seed)
    return [plan(rng, rnd) for rnd in range(rounds)]


if __name__ == "__main__":
    n_bad = campaign(int(sys.argv[1]) if len(sys.argv) > 1 else 1, int(sys.argv[2]) if len(sys.argv) > 2 else 10)
    print("mismatches:", n_bad)
    sys.exit(1 if n_bad else 0)
