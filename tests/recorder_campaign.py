"""Randomised exact-parity campaign for the squelched recorder and the measurements on its run table: the burst meter, the envelope,
the clock, the track and the sync (capture.h, burst.h, envelope.h, clock.h, track.h, sync.h).  Random stream counts, masks (per
context and per stream), cuts, submits in flight, resets, tight recorder caps and subsets of the measurements; rows made by hand so
that every run's edges are known and land on the kernels' own strides.  Every comparison is byte for byte with the restatements in
tfrec_amd/{capture,levels,burst,envelope,clock,track,sync}.py; nothing here has a tolerance.
    python tests/recorder_campaign.py <seed> <rounds> [modes]   (tests/test_recorder_campaign_gpu.py runs a short fixed campaign,
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

The burst sync (sync.h, tfrec_amd/sync.py) is a fifth measurement, behind the track: about half the rounds have one.  Its settings
(draw_sync) come from a generator of their own, seeded (seed, SYNC_STREAM), so that a seed's rows, masks, cuts, drains, resets, caps,
L and centres are what they were without it; a round with a sync measures the track too.  Every submit's records and match bitmap
are compared with the restatement on the track the same context returned (recorder.read_sync), under the plan's caps as the
header's Bits paragraph states them, and the merged chains with the restatement on the uncut rows.  SYNC_CLASSES names the sync's
own edges; sync_classes_hit() measures them back from the restatement on a plan.

The track's modes (amplitude.h, centre.h, phase.h; tfrec_amd/track.py's amplitude_tracks, auto_tracks, phase_tracks): a plan's
`mode` is None (the frequency track about the set centres, as ever), ("amplitude", levels), ("auto", K) or ("phase", K, lag); for
the last two the plan's centres are the fallbacks.  With modes on (campaign(..., modes=True); MODE_SEEDS is the fixed list) round
rnd runs in the mode ("amplitude", "auto", "phase")[rnd % 3]; the mode and its settings (draw_mode) come from a third generator,
seeded (seed, MODE_STREAM), and the rows also hold the kinds of stretch MODE_KINDS.  The first round of each mode has a sync and a
quarter of the others.  restate(), _check_submit() and run_plan() dispatch on the mode (recorder.mode_tracks, enable_mode,
read_mode); the centre records are read and compared too.  Behind an overflow on max_runs the carried pairs and prior are the
whole table's and the carried index is the delivered records'.  In the merged check a chain of an auto or phase plan whose first
piece begins fewer than K samples ahead of a cut and reaches it has a shorter head than the uncut run: its flags and n_samples
alone are compared (exempt()); every other chain byte for byte, the centre record included.  MODE_CLASSES names the modes' own
edges; mode_classes_hit() measures them back.  Which classes needed a kind of stretch of their own: phase:zero-sums (turns),
auto:wrap and phase:index:2048 (wrap), auto:occ==limit with P % 16 == 1 (occ), phase:tie (tie), amp:sum==limit (const, with a
level drawn to match), and the psk and ook kinds give the phase and amplitude tracks something to read.  phase:tie: a search over
all 4096 r found 1048 samples v = (C[r] + C[r + 1], S[r] + S[r + 1]) (halved where needed) for which the candidates r and r + 1 have
equal least |cross| (tie_pairs); a stretch of (200, 0), v, a not-over sample, repeated, sums to a multiple of v.
"""
import functools
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (_HERE, os.path.join(_HERE, "..")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import recorder as R  # noqa: E402
from recorder import B, CONT, OPEN, STAGES, T, last_pairs, raises, same_chains, same_records, same_table, zeros  # noqa: E402, F401
import amplitude_rows  # noqa: E402
import centre_rows  # noqa: E402
import phase_rows  # noqa: E402
from recorder_rows import keyed, quiet  # noqa: E402
from tfrec_amd import api, burst, capture, clock, decin, envelope, levels, sync, track, tune  # noqa: E402

EDGE64 = (0, 1, 31, 32, 33, 63)
CTX_MASKS = (0x02, 0x01, 0x20, 0x08, 0x2F)
MEASURES = ("meter", "envelope", "clock", "track")
DENSE_PERIOD = 357  # a window of mask 0x02 (356) and the one uncaptured sample behind it
ZONE = 1100  # the samples ahead of a block boundary kept for the boundary's own item
SEEDS = (12, 19, 21, 24, 35, 91)  # the fixed campaign of tests/test_recorder_campaign_gpu.py: ROUNDS rounds each (35 and 91 came
# with the sync: a store with D < 0, a continuing piece with nothing defined, a hit behind 2047 carried bits)
ROUNDS = 6
MODE_SEEDS = (112, 120, 122, 130, 131, 143)  # the fixed campaign with the track's modes on (round rnd: mode rnd % 3), ROUNDS rounds each:
# chosen on the CPU, the fewest of the seeds 100 .. 147 that reach every label of MODE_CLASSES between them
MODE_STREAM = 0x6D6F6465  # ... and so are the track's mode and its settings, seeded (seed, this)
SYNC_STREAM = 0x73796E63  # the sync's settings are drawn from a generator of their own, seeded (seed, this): the plan's draws stay


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


MODE_KINDS = ("psk", "ook", "turns", "wrap", "occ", "tie")  # the stretches the rounds with a mode add (rows' extra)
PSK_HZ = (0, 46, 94, 36000, -36000, 96000, -96000, 144000, -144000, 191900, -191900)  # at and beside the carrier search's quarter points
PSK_SPB = (1, 2, 10, 16, 64)


@functools.lru_cache(maxsize=None)
def tie_pairs():
    """The samples v = (C[r] + C[r + 1], S[r] + S[r + 1]), halved where that does not fit int16 and is exact, for which the
    phase track's carrier search has two candidates of positive score and equal least |cross| (r and r + 1: their cross terms are
    opposite) -> [(I, Q, the two candidates)].  Found by trying every r against the search's own terms: 1048 of the 4096, among
    them r = 4095, whose candidates are 0 and 4095; track.carrier_index and carrier_index_bruteforce keep the smaller."""
    c, s_ = (t.astype(np.int64) for t in tune.table())
    out = []
    for r in range(4096):
        i, q = int(c[r] + c[(r + 1) % 4096]), int(s_[r] + s_[(r + 1) % 4096])
        if max(abs(i), abs(q)) > 32767:
            if i % 2 or q % 2:
                continue
            i, q = i // 2, q // 2
        cross = np.where(i * c + q * s_ > 0, np.abs(q * c - i * s_), np.iinfo(np.int64).max)
        best = np.flatnonzero(cross == cross.min())
        if len(best) == 2:
            out.append((i, q, tuple(best.tolist())))
    return out


def _paint_mode(rng, row, a, l, W, kind):
    n = l - a + 1
    if kind == "tie" and n >= 3:  # (200, 0), v, a not-over sample, and again: every counted product is 200 v, and so are their sums
        ties = tie_pairs()
        i, q, _ = ties[(0, len(ties) - 1, int(rng.integers(len(ties))))[int(rng.integers(3))]]
        off = 2 * (n % 3 == 0)  # (so that the last sample is over too)
        k = np.arange(n - off)
        z = row[a + off:l + 1]
        z[k % 3 == 0], z[k % 3 == 1] = (200, 0), (i, q)
        row[a] = (200, 0)
        return
    if kind == "tie":
        kind = "turns"
    if kind == "psk":  # phase-keyed at a carrier offset: the phase track's signal (phase_rows.psk)
        hz = int(PSK_HZ[int(rng.integers(len(PSK_HZ)))] if rng.integers(2) else rng.integers(-192000, 192001))
        spb = PSK_SPB[int(rng.integers(len(PSK_SPB)))]
        row[a:l + 1] = phase_rows.psk(phase_rows.symbols(n // spb + 1, int(rng.integers(1 << 16))), hz, spb, phase=(0.0, 0.3)[int(rng.integers(2))])[:n]
    elif kind == "ook":  # on-off keyed: the amplitude track's signal (amplitude_rows.keyed); every gap is shorter than W
        ws, left = [], n
        while True:
            w = int(rng.integers(1, 161))
            if left - w < 2:
                ws.append(left)
                break
            g = int(rng.integers(1, min(W - 1, 160, left - w - 1) + 1))
            ws += [w, g]
            left -= w + g
        row[a:l + 1] = amplitude_rows.keyed(ws, True, int(rng.integers(1, 1 << 16)), on=(4000, 3000, 2500)[int(rng.integers(3))])
    elif kind == "occ" and n >= 70:  # centre_rows.exact_pair at the stretch's own length: a tone at +30 kHz (bin 5) and in its middle
        # as many products at -48 kHz (bin -8) as an occupied bin needs, or one less.  Not-over samples near its end -- single
        # ones drop 2 products each, two in a row 3 -- leave P = n - 1 - d counted products with P % 16 == 1, where (P + 15) // 16
        # and P // 16 differ
        d = (n - 2) % 16
        d += 16 * (d == 1)
        singles, floor = (d - 3 * (d % 2)) // 2, row[a:l + 1].copy()
        limit = (n - 1 - d + 15) // 16
        f = np.full(n, 30000)
        f[20:20 + limit - int(rng.integers(2))] = -48000
        row[a:l + 1] = centre_rows.tone(f)
        off = [n - 1 - 2 * (i + 1) for i in range(singles)] + ([n - 2 * singles - 5, n - 2 * singles - 4] if d % 2 else [])
        row[a + np.array(off, dtype=np.int64)] = floor[off]
    elif kind == "occ":
        row[a:l + 1] = centre_rows.tone(np.full(n, 30000))
    elif kind == "turns":  # quarter turns: counted products whose sums are (A, B) = (0, 0) where their number is even
        row[a:l + 1] = phase_rows.quarter_turns(n)
    elif rng.integers(2):  # "wrap": a tone at 192 kHz, a little to either side: the carrier index at 2048 ...
        sign = 1 - 2 * (np.arange(n) % 2)
        row[a:l + 1, 0], row[a:l + 1, 1] = 6000 * sign, sign * rng.integers(-40, 41, n)
    else:  # ... or products at +186 kHz and at -192 kHz: the histogram's bins 31 and -32, its two ends, both occupied
        row[a:l + 1] = centre_rows.tone(np.where(rng.integers(2, size=n), 186000, -192000))


def _paint(rng, row, a, l, W, kind=None, extra=()):
    """Over-threshold samples from a to l (both included); its first and last sample are over whatever the kind.  extra: further
    kinds to draw from (MODE_KINDS)."""
    n = l - a + 1
    kinds = ("tone", "const", "noise", "full") + (("gappy",) if n >= 3 else ()) + tuple(extra)
    kind = kind or kinds[int(rng.integers(len(kinds)))]
    if kind in MODE_KINDS:
        _paint_mode(rng, row, a, l, W, kind)
    elif kind == "tone":  # keyed: the clock's and the track's signal
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


def _fill_row(rng, row, W, cuts, kind=None, extra=()):
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
                _paint(rng, row, a, l, W, kind, extra)
            free = st[-1][1] + W + 1
            pos = free + int(rng.integers(0, 3)) * int(rng.integers(0, 300))
        if P < E and (k + 1) in cuts and rng.integers(6) == 0:  # class 8
            a = P - int(rng.integers(1, 600))
            P2 = B * min(m for m in marks if m > k + 1)
            if a >= free:
                l = P2 + int(rng.integers(0, 300)) if P2 < E else E - 1
                _paint(rng, row, a, l, W, kind or (("tone", "noise") + tuple(extra))[int(rng.integers(2 + len(extra)))])
                free = l + W + 1
                k = P2 // B
                continue
        for _ in range(3):
            st = _boundary(rng, P, W, P == E, (k + 1) in cuts)
            if not st or (st[0][0] >= free and st[-1][1] < E):
                break
            st = []
        for a, l in st:
            _paint(rng, row, a, l, W, kind, extra)
        if st:
            free = st[-1][1] + W + 1
        k += 1


def rows(rng, n_streams, n_blocks, windows, cuts=(), kind=None, extra=()):
    """int16 [n_streams, n_blocks B, 2] for a channel-rate context; windows[s]: stream s's W; cuts: the block indices at which the
    input will be cut into submits (the classes at a submit cut are placed there); kind: every stretch is of this kind of _paint's
    (default: drawn); extra: further kinds to draw from (MODE_KINDS; default: none, and the rows are what they were).  Pure numpy,
    deterministic in rng."""
    out = np.stack([quiet(n_blocks, int(rng.integers(1 << 30))) for _ in range(n_streams)])
    for s in range(n_streams):
        _fill_row(rng, out[s], int(windows[s]), set(int(c) for c in cuts), kind, extra)
    return out


def dense(n_blocks):
    """The densest legal input of mask 0x02 (W = 356): one over sample every 357 -> int16 [n_blocks B, 2].  Every run is 356 long
    and one uncaptured sample lies between two runs: 276 runs in 12 blocks."""
    row = quiet(n_blocks, 7)
    row[::DENSE_PERIOD] = (3000, -3000)
    return row


def _carrier(j):
    """Stretch j's carrier in Hz: neighbours lie 37 histogram bins apart, and 127 in a row are all different."""
    return (j * 37 % 127 - 63) * 3000


def dense_heads(n_blocks, swaps):
    """The dense row with a head to measure in the periods `swaps` (none next to another): period i's over sample and the next one's
    become one stretch of 358 over samples from 357 i -- phase-keyed and a plain tone in turn, each at its own carrier --, so the
    run is [357 i, 357 i + 713), one uncaptured sample still lies behind it, and the row holds one run less per swap.  Every other
    run has one over sample: 0 counted products, the fallback."""
    row = dense(n_blocks)
    for j, i in enumerate(swaps):
        a = DENSE_PERIOD * i
        sym = phase_rows.symbols(36, j) if j % 2 == 0 else [1] * 36
        row[a:a + DENSE_PERIOD + 1] = phase_rows.psk(sym, _carrier(j))[:DENSE_PERIOD + 1]
    return row


LOUD_HEAD = 66  # over samples: 65 counted products, one more than a measured centre needs
LOUD_PERIOD = LOUD_HEAD - 1 + 356 + 1  # the run of such a stretch under mask 0x02, and the uncaptured sample behind it


def dense_loud(n_blocks, first, count, seed):
    """The dense row, but runs first .. first + count - 1 begin with a tone of LOUD_HEAD over samples, run j's at _carrier(j + seed):
    these runs are 421 samples long instead of 356, every other one is the dense row's -> int16 [n_blocks B, 2]."""
    row = quiet(n_blocks, 7)
    pos, j = 0, 0
    while pos < len(row):
        if first <= j < first + count:
            z = phase_rows.psk([1] * (LOUD_HEAD // 10 + 1), _carrier(j + seed))[:LOUD_HEAD]
            row[pos:pos + LOUD_HEAD] = z[:len(row) - pos]
            pos += LOUD_PERIOD
        else:
            row[pos] = (3000, -3000)
            pos += DENSE_PERIOD
        j += 1
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
def sync_on(p, measure):
    """The sync sits on the track: a plan's settings are in force where the track is measured."""
    return p.get("sync") is not None and "track" in measure


def restate(p, sizes, reset=None, measure=(), caps=True):
    """The restatements over the plan's rows cut into submits of `sizes` blocks, the streams of reset[1] restarted with submit
    reset[0] -> one dict per submit: the full table and pool (no caps), the level records, and the records of `measure`.  With
    the track and a plan's sync: "sync", the sync's records and words, and "sync_state", what the submit before left.  The track is
    the plan's mode's; "centres": the centre records of the auto and phase modes, whose carried index is a capped context's too (an
    OPEN entry at or beyond max_runs has no record and leaves index -1, the header's rule; the carried pairs and prior are the whole
    table's).  Otherwise the sync alone is a capped context's (caps: the plan's, if it has any): it looks at the delivered records -- those below max_runs -- and
    at the runs that fit max_samples, and carries what these leave (the header's Bits paragraph)."""
    n, x = p["n"], p["dec"]
    cst, lst, base, prev, tst, pos, out = [None] * n, [None] * n, [0] * n, zeros(n), None, 0, []
    sst = sync.fresh_state(n)
    mr, ms = (p.get("cap") if caps else None) or (None, None)
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
            mode = p.get("mode")
            cen, recs, words, tst = R.mode_tracks(mode, decs, thr, table[0], p["L"], p["centres"], tst, base=base)
            e["track"] = (recs, words)
            e["track_state"] = tst  # (what the submit leaves)
            if cen is not None:
                e["centres"] = cen
                if mr is not None and len(cen) > mr:  # an OPEN entry without a record leaves no index behind; pairs and prior stay
                    tst = (tst[0], track._next_centre_state(n, cen[:mr]))
            if sync_on(p, measure):
                srecs, swords, nxt = sync.syncs(recs[:mr], words, p["sync"], sst, n, max_samples=ms)
                e["sync"], e["sync_state"], sst = (srecs, swords), sst, nxt
        out.append(e)
        prev, pos, base = last_pairs(decs), pos + nb, [v + nb * B for v in base]
    return out


def finish(p):
    """The derived parts of a plan: the clamped rows (a channel-rate context's own samples) and what every submit must give."""
    p["dec"] = decin.clamp(p["x"])
    p["windows"] = [window(m) for m in p["masks"]]
    p["expect"] = restate(p, p["sizes"], p.get("reset"))
    return p


def make_plan(x, ctx_mask, masks, sizes, L=5, centres=None, thresh=None, drains=None, reset=None, cap=None, measure=MEASURES, sync=None,
              mode=None):
    """A plan from its parts.  configured: the streams whose settings are not the context's (tfrec_amd_configure_streams).  sync:
    a sync.Settings or None; mode: the track's (None: the frequency track about the set centres; ("amplitude", levels), ("auto", K),
    ("phase", K, lag): `centres` are the fallbacks of the last two).  A plan that has either measures the track too (drawn: the
    measurements as they were given)."""
    n = len(x)
    thresh = list(thresh or [T] * n)
    drawn = tuple(measure)
    if sync is not None or mode is not None:
        measure = tuple(m for m in MEASURES if m in drawn or m == "track")
    return finish(dict(n=n, nb=x.shape[1] // B, x=np.ascontiguousarray(x), ctx_mask=ctx_mask, masks=list(masks), sizes=tuple(sizes),
                       thresh=thresh, configured=[s for s in range(n) if masks[s] != ctx_mask or thresh[s] != T], L=L,
                       centres=list(centres or [0] * n), drains=list(drains or [None] * len(sizes)), reset=reset, cap=cap,
                       measure=tuple(measure), drawn=drawn, sync=sync, mode=mode))


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


def sync_rng(seed):
    """The generator the sync's settings are drawn from: the plan's own generator draws what it drew without a sync."""
    return np.random.default_rng([int(seed), SYNC_STREAM])


def min_rate(P):
    """The smallest legal rate for P pattern bits: its span is the largest there is (2047 where no rate steps over it)."""
    R = max(1000, 384000 * (P - 1) // 2048)
    while sync.deltas(R, P)[-1] > sync.HISTORY:
        R += 1
    return R


def draw_sync(srng, rnd=0):
    """A round's sync.Settings, or None: every round with rnd % 3 == 0 has one and a quarter of the others, half of all.  The
    settings at which the kernel's arithmetic changes are drawn as often as the ones in between: P = 8 and 64, E = 0 and its
    limit, a span inside one lane's word (below 32: P = 8 and a rate above 85333), the largest span, and the patterns of one
    bit value, which the tracks of constant samples and of the dense row's holds meet."""
    if rnd % 3 and srng.integers(4):
        return None
    P = int((8, 64, srng.integers(9, 64))[int(srng.integers(3))])
    k = int(srng.integers(5))
    if k == 0:  # span < 32
        P, rate = 8, int(srng.integers(85334, 96001))
    elif k == 1:  # the largest span
        rate = min_rate(P)
    else:  # in between, short spans more often than long ones: most runs are a few hundred samples
        lo = min_rate(P)
        rate = int(lo * (96000 / lo) ** (1 - float(srng.random()) ** 2))
    E = int((0, (P - 1) // 2, srng.integers(0, (P - 1) // 2 + 1))[int(srng.integers(3))])
    ones = (1 << P) - 1
    pattern = (0, ones, 0xAAAAAAAAAAAAAAAA & ones, int(srng.integers(0, 1 << 63)) * 2 + int(srng.integers(2)) & ones)[int(srng.integers(4))]
    return sync.Settings(rate, pattern, P, E, bool(srng.integers(2)))


def mode_rng(seed):
    """The generator a round's mode and its settings are drawn from, as sync_rng: the plan's own generator draws what it drew."""
    return np.random.default_rng([int(seed), MODE_STREAM])


def _between(mrng, lo, hi):
    """lo, hi, and a value between them, the small ones more often than the large: each of the three as often as the others."""
    return int((lo, hi, lo * (hi / lo) ** (float(mrng.random()) ** 2))[int(mrng.integers(3))])


def draw_mode(mrng, rnd, p):
    """Round rnd's mode, ("amplitude", "auto", "phase")[rnd % 3], with its settings, for the plan p as it was drawn -> (mode, L).
    The settings at which the arithmetic changes are drawn as often as the ones in between: K = 64, 65 and 66 (63, 64 and 65
    products at the most), 4096, a first piece's own length and one less (n == K, n == K + 1), and between 64 and 4096 the small
    ones more often (most runs are a few hundred samples, and a chain cut inside its head is exempt from the merged check); lag 1
    and 64, and (L, lag) = (16, 64), the carried pairs' limit L + m = 80, now and then; a level per stream of 0, 65535, the
    stream's threshold, a `const` stretch's |I| + |Q| (3000, 2500, 4000: sum == L * level exactly, bit 0) and one below it."""
    name, L = ("amplitude", "auto", "phase")[rnd % 3], p["L"]
    if name == "amplitude":
        lv = []
        for s in range(p["n"]):
            k = int(mrng.integers(8))
            lv.append(int((0, 65535, p["thresh"][s], 3000, 2999, 2500, 3999)[k] if k < 7 else mrng.integers(0, 65536)))
        return (name, lv), L
    k = int(mrng.integers(6))
    if k < 4:
        K = (64, 65, 66, 4096)[k]
    elif k == 4:
        K = _between(mrng, 64, 4096)
    else:  # a first piece's length, or one less
        t = np.concatenate([e["table"][0] for e in p["expect"]])
        n = t["n_samples"][(t["flags"] & CONT == 0) & (t["n_samples"] >= 65) & (t["n_samples"] <= 4096)]
        K = int(n[int(mrng.integers(len(n)))]) - int(mrng.integers(2)) if len(n) else 64
    if name == "auto":
        return (name, K), L
    lag = _between(mrng, 1, 64)
    if mrng.integers(4) == 0:
        L, lag = 16, 64
    return (name, K, lag), L


def plan(rng, rnd=0, srng=None, mrng=None):
    """Draw one round; srng: the generator of the sync's settings (default: no sync); mrng: the generator of the track's mode and
    its settings (default: the frequency track, and every draw is what it was)."""
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
        x = rows(rng, n, nb, [window(m) for m in masks], cuts, extra=MODE_KINDS if mrng is not None else ())
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
    p = make_plan(x, ctx_mask, masks, sizes, L=L, centres=centres, thresh=thresh, drains=drains, reset=reset, measure=measure,
                  sync=draw_sync(srng, rnd if mrng is None else rnd // 3) if srng is not None else None)
    if mrng is not None:  # (a sync in the first round of each mode and in a quarter of the others)
        p["mode"], p["L"] = draw_mode(mrng, rnd, p)
        p["measure"] = tuple(m for m in MEASURES if m in p["measure"] or m == "track")
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


def describe(p, with_sync=True):
    """with_sync=False: the plan as it was drawn ahead of the sync's settings, which also add the track to `measure`."""
    st = p.get("sync")
    text = "streams %d blocks %d ctx %02x masks %s thresh %s sizes %s drains %s L %d centres %s reset %s cap %s measure %s" % (
        p["n"], p["nb"], p["ctx_mask"], ["%02x" % m for m in p["masks"]] if p["configured"] else "-",
        p["thresh"] if p["configured"] else "-", list(p["sizes"]), p["drains"], p["L"], p["centres"], p["reset"], p["cap"],
        ",".join(p["measure"] if with_sync else p["drawn"]))
    if not with_sync:
        return text
    mode = p.get("mode")
    if mode is not None:  # (centres: the fallbacks)
        text += " mode " + ("amplitude levels %s" % mode[1] if mode[0] == "amplitude" else "auto K %d" % mode[1] if mode[0] == "auto" else
                            "phase K %d lag %d" % mode[1:])
    return text + (" sync -" if st is None else " sync rate %d pattern %x P %d E %d both %d span %d" % (
        st.rate, st.pattern, st.P, st.E, st.both, st.span))


# ---- the sync's own classes, measured back from the restatement on a plan
SYNC_CLASSES = (
    "P:8", "P:64", "E:0", "E:limit", "both:on", "both:off", "span:<32", "span:2047", "pattern:zeros", "pattern:ones", "pattern:mixed",
    "defined-inside",        # a CONTINUES record whose first defined sample lies inside it: 0 < span - H < n_samples
    "defined-inside:H<32",   # ... with 0 < H < 32
    "continues:none",        # a CONTINUES record that is not OPEN and has no defined sample
    "H2047:early-hit",       # a CONTINUES record with H = 2047 and a hit among its first span samples
    "hit:continues-first",   # a hit at sample 0 of a CONTINUES record
    "hit:open-last",         # a hit at the last sample of an OPEN record
    "word:shared",           # a run's last sample is a hit, its bit is not a word's last, and another run follows in the pool
    "word:D<0",              # hits in the pool's first run, which starts off a lane's first sample: the store with D < 0
    "across:block",          # a hit at a k for which k and k - span lie in different blocks of one submit
    "across:cut",            # ... in different submits
    "both:plain", "both:complement", "both:tie",  # under BOTH: where a record's best comes from
    "min:two-blocks",        # the smallest distance is attained in two blocks of a record (best_at: the earlier)
    "min:two-words",         # ... in two 32-sample words of one block
    "dense:>256",            # a stream with more than 256 sync records in one submit
    "overflow:max_runs", "overflow:max_samples",  # a submit that overflows, with a sync
    "continues:H=0",         # a CONTINUES record whose predecessor did not fit: it starts without history
    "reset:mid-chain")       # a reset between two submits: the reset stream's chain is dropped, another stream's continues


def _distances(st, h, t):
    """The header's Distance, counted in place: a piece's track t with the available history h -> (the first defined k, d[k] from
    there on)."""
    H, n = len(h), len(t)
    k0 = max(0, st.span - H)
    ext = np.concatenate([h, t]).astype(np.int64)
    d = np.zeros(max(0, n - k0), dtype=np.int64)
    for j in range(st.P):
        a = H + k0 - st.delta[j]
        d += ext[a:a + len(d)] != st.bit[j]
    return k0, d


def sync_classes_hit(p):
    """The sync's edge classes a plan holds, from the restatement of its submits (under its caps) -> a set of SYNC_CLASSES'
    labels; none for a plan without a sync."""
    st = p["sync"]
    if st is None:
        return set()
    ones = (1 << st.P) - 1
    hit = {"both:on" if st.both else "both:off",
           "pattern:zeros" if st.pattern == 0 else "pattern:ones" if st.pattern == ones else "pattern:mixed"}
    hit |= {lab for lab, on in (("P:8", st.P == 8), ("P:64", st.P == 64), ("E:0", st.E == 0), ("E:limit", st.E == (st.P - 1) // 2),
                                ("span:<32", st.span < 32), ("span:2047", st.span == 2047)) if on}
    sub = restate(p, p["sizes"], p["reset"], ("track",))
    ms = p["cap"][1] if p["cap"] else None
    for e in sub:
        (trecs, twords), (recs, words), state = e["track"], e["sync"], e["sync_state"]
        if len(recs) and np.bincount(recs["stream"]).max() > 256:
            hit.add("dense:>256")
        if p["cap"] and len(e["table"][0]) > p["cap"][0]:
            hit.add("overflow:max_runs")
        if p["cap"] and len(e["table"][1]) > p["cap"][1]:
            hit.add("overflow:max_samples")
        for i, r in enumerate(recs):
            if not sync._fits(r, ms):
                continue
            s, a, n, cont = int(r["stream"]), int(r["start_sample"]), int(r["n_samples"]), bool(int(r["flags"]) & CONT)
            h = np.asarray(state["bits"][s], dtype=np.uint8)[-sync.HISTORY:] if cont else np.zeros(0, dtype=np.uint8)
            H = len(h)
            m, t = sync.bits_of(r, words), track.bits_of(trecs[i], twords)
            k0, d = _distances(st, h, t)
            assert np.array_equal(m[k0:], (d <= st.E) | (st.both & (d >= st.P - st.E))) and not m[:k0].any()
            if cont:
                if 0 < st.span - H < n:
                    hit |= {"defined-inside"} | ({"defined-inside:H<32"} if 0 < H < 32 else set())
                if not int(r["flags"]) & OPEN and int(r["best"]) == sync.NONE:
                    hit.add("continues:none")
                if H == 0:
                    hit.add("continues:H=0")
                if m[:st.span].any():
                    hit |= {"across:cut"} | ({"H2047:early-hit"} if H == sync.HISTORY else set())
                if m[0]:
                    hit.add("hit:continues-first")
            if int(r["flags"]) & OPEN and m[-1]:
                hit.add("hit:open-last")
            if m[-1] and (int(r["bit_offset"]) + n) % 32 and i + 1 < len(recs) and sync._fits(recs[i + 1], ms):
                hit.add("word:shared")
            if int(r["bit_offset"]) == 0 and a % 32 and m[:32 - a % 32].any():
                hit.add("word:D<0")
            at = np.flatnonzero(m)
            at = at[at >= st.span]
            if ((a + at) // B != (a + at - st.span) // B).any():
                hit.add("across:block")
            if len(d):
                if st.both:
                    lo, hi = int(d.min()), st.P - int(d.max())
                    hit.add("both:plain" if lo < hi else "both:complement" if hi < lo else "both:tie")
                f = np.minimum(d, st.P - d) if st.both else d
                where = a + k0 + np.flatnonzero(f == f.min())
                if len(set((where // B).tolist())) > 1:
                    hit.add("min:two-blocks")
                if any(len(set((where[where // B == b] // 32).tolist())) > 1 for b in set((where // B).tolist())):
                    hit.add("min:two-words")
    if p["reset"]:
        j, streams = p["reset"]
        prev, cur = sub[j - 1]["sync"][0], sub[j]["sync"][0]
        for s in streams:
            mine = cur[cur["stream"] == s]
            dropped = ((prev["stream"] == s) & (prev["flags"] & OPEN != 0)).any() and len(mine) and not int(mine[0]["flags"]) & CONT
            if dropped and ((cur["flags"] & CONT != 0) & ~np.isin(cur["stream"], streams)).any():
                hit.add("reset:mid-chain")
    return hit


# ---- the modes' own classes, measured back from the restatement on a plan
MODE_CLASSES = (
    # the heads of the auto and phase modes: label + ":auto" and ":phase"
    *(lab + ":" + m for m in ("auto", "phase") for lab in (
        "n<K", "n==K", "n==K+1",  # a first piece's length against K
        "K:64", "K:4096",
        "head:across-block",      # a block boundary inside the head, within one submit
        "head:cut",               # an OPEN first piece shorter than K, and its INHERITED continuation in the next submit
        "counted:63", "counted:64", "counted:65",
        "counted:<products",      # the mask test dropped a product
        "head:configured",        # a head with 64 and more counted products under a configured stream's own mask or threshold
        "continues:index-1",      # a CONTINUES entry that falls back: the OPEN entry ahead of it had no record under max_runs
        "reset:first-piece",      # the piece behind a reset, measured as a first piece, while another stream inherits
        "fallback:+192000", "fallback:-192000")),  # an entry that falls back to a centre at a limit
    "auto:occ==limit",            # a bin with hist exactly (P + 15) // 16, with P % 16 == 1 (P // 16 is one less)
    "auto:occ==limit-1",          # a bin one below the limit
    "auto:lo==hi",                # one occupied bin
    "auto:wrap",                  # bins -32 and 31 both occupied
    "phase:zero-sums",            # P >= 64 and (A, B) == (0, 0)
    "phase:tie",                  # two candidates of positive score and equal least |cross|: the smaller index is kept
    "phase:index:0", "phase:index:1024", "phase:index:2048", "phase:index:3072", "phase:index:between",
    # the tracks
    "lag:1", "lag:64", "L+lag:80",
    "chain<lag",                  # a chain shorter than the lag with another run behind it in the same 32-sample word
    "prior:<lag",                 # a continuing piece whose first products are undefined
    "prior:1..79", "prior:80",
    "start:behind-boundary:block",  # a run whose first sample lies fewer than 80 behind a block boundary inside a submit,
    "start:behind-boundary:cut",    # ... and behind a cut: those lanes read the slots ahead of the block
    "amp:sum==limit",             # the sum equals L * level: bit 0
    "amp:sum==limit+1..L",        # ... and a sum just above it: bit 1
    "amp:level0", "amp:level65535",
    "amp:prior<L",                # a continuing piece with a prior below L
    "dense:amplitude", "dense:auto", "dense:phase")  # a stream with more than 256 runs in one submit


def _head_products(e, r, K):
    """Entry r's head as the header counts it -> (dot, crs) of its counted products."""
    s = int(r["stream"])
    a = int(r["start_sample"]) - e["base"][s]
    nh = min(int(r["n_samples"]), K)
    z = burst._pairs(e["decs"][s])[a:a + nh].astype(np.int64)
    over = np.abs(z[:, 0]) + np.abs(z[:, 1]) > np.repeat(e["levels"][s]["thresh"].astype(np.int64), B)[a:a + nh]
    both = over[1:] & over[:-1]
    I, Q, Ip, Qp = z[1:, 0], z[1:, 1], z[:-1, 0], z[:-1, 1]
    return (I * Ip + Q * Qp)[both], (Q * Ip - I * Qp)[both]


def mode_classes_hit(p):
    """The modes' edge classes a plan holds, from the restatement of its submits (under its caps) -> a set of MODE_CLASSES'
    labels; none for a plan without a mode."""
    mode = p.get("mode")
    if mode is None:
        return set()
    name, L, hit = mode[0], p["L"], set()
    sub = restate(p, p["sizes"], p["reset"], ("track",))
    mr = p["cap"][0] if p["cap"] else None
    lim = track.PHASE_AHEAD if name == "phase" else track.AHEAD
    for k, e in enumerate(sub):
        t = e["table"][0][:mr]
        if len(t) and np.bincount(t["stream"]).max() > 256:
            hit.add("dense:" + name)
        before = sub[k - 1]["track_state"] if k else None
        prior = (before[0] if isinstance(before, tuple) else before)["prior"] if before is not None else np.zeros(p["n"], dtype=np.int64)
        for i, r in enumerate(t):
            s, fl, n = int(r["stream"]), int(r["flags"]), int(r["n_samples"])
            a = int(r["start_sample"]) - e["base"][s]
            pr = int(prior[s]) if fl & CONT else 0
            if name == "phase":
                m = mode[2]
                hit |= {lab for lab, on in (("lag:1", m == 1), ("lag:64", m == 64), ("L+lag:80", L + m == 80)) if on}
                if not fl & CONT and n < m and (int(r["pool_offset"]) + n) % 32 and i + 1 < len(t):
                    hit.add("chain<lag")
                if fl & CONT:
                    hit |= {"prior:<lag"} if pr < m else set()
                    hit.add("prior:80" if pr == lim else "prior:1..79")
                if not fl & CONT and a >= B and a % B < lim:
                    hit.add("start:behind-boundary:block")
                if k and a < lim:
                    hit.add("start:behind-boundary:cut")
            if name == "amplitude":
                lv = mode[1][s]
                hit |= {lab for lab, on in (("amp:level0", lv == 0), ("amp:level65535", lv == 65535), ("amp:prior<L", fl & CONT and pr < L)) if on}
                z = burst._pairs(e["decs"][s])[max(0, a - L + 1):a + n].astype(np.int64)  # (the samples of this submit: enough to find one)
                cs = np.concatenate([[0], np.cumsum(np.abs(z[:, 0]) + np.abs(z[:, 1]))])
                sums = cs[L:] - cs[:-L]
                hit |= {"amp:sum==limit"} if (sums == L * lv).any() else set()
                hit |= {"amp:sum==limit+1..L"} if ((sums > L * lv) & (sums <= L * lv + L)).any() else set()
            if name not in ("auto", "phase"):
                continue
            K, c = mode[1], e["centres"][i]
            tag = lambda lab: hit.add(lab + ":" + name)  # noqa: E731
            src, cnt = int(c["source"]), int(c["n_counted"])
            if src == track.FALLBACK and abs(int(c["centre_hz"])) == 192000:
                tag("fallback:%+d" % int(c["centre_hz"]))
            if fl & CONT:
                if src == track.FALLBACK:
                    tag("continues:index-1")
                continue
            for lab, on in (("n<K", n < K), ("n==K", n == K), ("n==K+1", n == K + 1), ("K:64", K == 64), ("K:4096", K == 4096),
                            ("head:across-block", a % B + min(n, K) > B), ("counted:%d" % cnt, cnt in (63, 64, 65)),
                            ("counted:<products", cnt < min(n, K) - 1), ("head:configured", cnt >= 64 and s in p["configured"])):
                if on:
                    tag(lab)
            if fl & OPEN and n < K and k + 1 < len(sub):
                nxt = sub[k + 1]["centres"][:mr] if "centres" in sub[k + 1] else []
                if any(int(q["stream"]) == s and int(q["flags"]) & CONT and int(q["source"]) == track.INHERITED for q in nxt):
                    tag("head:cut")
            if cnt < track.COUNT_MIN:
                continue
            dot, crs = _head_products(e, r, K)
            assert len(dot) == cnt, "the classes' count of products is not the restatement's"
            if name == "auto":
                h = np.bincount(burst._bins(dot, crs), minlength=burst.N_BINS)
                limit = (cnt + 15) // 16
                hit |= {"auto:occ==limit"} if cnt % 16 == 1 and (h == limit).any() else set()
                hit |= {"auto:occ==limit-1"} if (h == limit - 1).any() else set()
                occ = np.flatnonzero(h >= limit)
                hit |= {"auto:lo==hi"} if len(occ) == 1 else set()
                hit |= {"auto:wrap"} if h[burst.N_BINS // 2] >= limit and h[burst.N_BINS // 2 - 1] >= limit else set()
            else:
                if not dot.sum() and not crs.sum():
                    hit.add("phase:zero-sums")
                elif src == track.MEASURED:
                    idx = int(c["index"])
                    tc, ts = (v.astype(object) for v in tune.table())  # (Python integers: the sums reach 2^43)
                    A, Bs = int(dot.sum()), int(crs.sum())
                    cross = [abs(Bs * int(u) - A * int(v)) for u, v in zip(tc, ts) if A * int(u) + Bs * int(v) > 0]
                    hit |= {"phase:tie"} if cross.count(min(cross)) == 2 else set()
                    hit.add("phase:index:%d" % idx if idx % 1024 == 0 else "phase:index:between")
        if p["reset"] and p["reset"][0] == k and name in ("auto", "phase"):
            cur, prev = e["centres"][:mr], sub[k - 1]["centres"][:mr]
            for s in p["reset"][1]:
                mine = cur[cur["stream"] == s]
                dropped = (((prev["stream"] == s) & (prev["flags"] & OPEN != 0)).any() and len(mine) and not int(mine[0]["flags"]) & CONT
                           and int(mine[0]["start_sample"]) == 0)
                if dropped and ((cur["source"] == track.INHERITED) & ~np.isin(cur["stream"], p["reset"][1])).any():
                    hit.add("reset:first-piece:" + name)
    return hit


# ---- one plan on the GPU
def _check_submit(r, p, k, measure, states, newest):
    """Every read of the oldest undrained submit, which is the plan's k-th; states: the track's and the sync's state ahead of it
    -> (what was read, the two states behind it).  The reads are recorder.py's: each holds its records to the restatement on what
    the context itself returned; here they are also held to the restatement on the generated rows."""
    tst, sst = states
    e = p["expect"][k]
    nb, decs, base, prev = e["nb"], e["decs"], e["base"], e["prev"]
    cap = p["cap"] or full_cap(p)
    wr, wp, over = capture.prefix(e["table"][0], e["table"][1], *cap)
    got = dict(table=r.read_captures(allow_overflow=True))
    assert r.capture_overflow == over and r.capture_totals == (len(e["table"][0]), len(e["table"][1])), "totals %s overflow %s" % (
        r.capture_totals, r.capture_overflow)
    R.assert_tables(got["table"], (wr, wp))  # independent of the context: the restatement on the generated rows
    got["levels"] = r.read_levels()
    for f in levels.LEVEL_DTYPE.names:
        assert np.array_equal(got["levels"][f], e["levels"][f]), "levels field %s" % f
    if newest:  # (tfrec_amd_read_decimated returns the last submit's samples)
        for s in range(p["n"]):
            assert np.array_equal(r.decimated(s, nb * B), decs[s]), "stream %d's decimated samples" % s
    if "meter" in measure:
        got["meter"] = R.read_meter(r, nb, prev, base, overflow=over, decs=decs)[0]
    if "envelope" in measure:
        got["envelope"] = R.read_envelope(r, nb, prev, base, overflow=over, decs=decs)[0]
    if "clock" in measure:
        got["clock"] = R.read_clock(r, nb, base, overflow=over, decs=decs)[0]
    if "track" in measure:
        mode = p.get("mode")
        cen, recs, words, _, nxt = R.read_mode(r, mode, nb, base, p["L"], p["centres"], tst, overflow=over, decs=decs)
        if over:  # the chains' carried pairs and prior are the whole table's, not the delivered prefix's; the carried index of the
            # auto and phase modes is the delivered records': -1 where the OPEN entry had none
            thr = [np.repeat(v["thresh"].astype(np.int64), B) for v in e["levels"]]
            whole = R.mode_tracks(mode, decs, thr, e["table"][0], p["L"], p["centres"], tst, base=base)[3]
            nxt = whole if cen is None else (whole[0], nxt[1])
        got["track"], tst = (recs, words), nxt
        if cen is not None:
            got["centres"] = cen
        if sync_on(p, measure):
            # read_sync's rule: the restatement on the track records and words this context returned for the submit.  The state
            # it returns is what the delivered records leave -- behind an overflow too: a run that does not fit max_samples leaves
            # H = 0, and so does an OPEN run beyond max_runs, which has no record
            srecs, swords, sst = R.read_sync(r, p["sync"], sst, recs, words, overflow=over)
            assert len(swords) == (len(wp) + 31) // 32, "sync: %d words for %d delivered pairs" % (len(swords), len(wp))
            got["sync"] = (srecs, swords)
    full = e["table"][0][:cap[0]]
    for m in tuple(measure) + (("sync",) if "sync" in got else ()):  # under an overflow too: the total, and the table's prefix
        recs, total = got[m][0] if m in ("track", "sync") else got[m], getattr(r, STAGES[m].total)
        assert total == len(e["table"][0]), "%s: a total of %d for %d runs" % (m, total, len(e["table"][0]))
        same_table(recs, full, m)
        assert len(recs) == len(full), "%s: %d records of %d" % (m, len(recs), len(full))
    if "centres" in got:
        assert r.centre_total == r.track_total == len(e["table"][0]), "centres: a total of %d for %d runs" % (r.centre_total, len(e["table"][0]))
        same_table(got["centres"], full, "centres")
        assert len(got["centres"]) == len(full), "centres: %d records of %d" % (len(got["centres"]), len(full))
    return got, (tst, sst)


def merged(m, pieces, restarts=None):
    """A measurement's chains over the submits' pieces, by stream (within a stream: in the order of the samples)."""
    return sorted(STAGES[m].module.chains(pieces, restarts), key=lambda c: int(c["stream"]))


def has_heads(p, measure):
    return p.get("mode") is not None and p["mode"][0] in ("auto", "phase") and "track" in measure


def reference_cut(p):
    """What the merged chains are compared against: the rows cut at the reset alone (uncut without one) -> (sizes, reset, the
    restarts of the plan's own cut, the reference's)."""
    j = p["reset"][0] if p["reset"] else None
    blocks = int(np.sum(p["sizes"][:j])) if j else 0
    return ((blocks, p["nb"] - blocks) if j else (p["nb"],), (1, p["reset"][1]) if j else None,
            {j: p["reset"][1]} if j else None, {1: p["reset"][1]} if j else None)


def head_lengths(K, centres, restarts):
    """Per merged chain, in merged()'s order: the samples its centre was measured on, min(K, the first piece's n_samples)."""
    first = sorted(burst.chains(centres, restarts, join=lambda ps: ps[0].copy()), key=lambda c: int(c["stream"]))
    return [min(K, int(c["n_samples"])) for c in first]


def exempt(p, got_centres, ref_centres):
    """The chains of an auto or phase plan whose first piece begins fewer than K samples ahead of a cut and reaches it: their head
    is shorter than the uncut run's, so their centre, track and sync may differ -> one bool per merged chain.  A condition on
    the pieces' lengths, not a measurement."""
    _, _, mine, theirs = reference_cut(p)
    a, b = head_lengths(p["mode"][1], got_centres, mine), head_lengths(p["mode"][1], ref_centres, theirs)
    assert len(a) == len(b), "chains: %d, want %d" % (len(a), len(b))
    return [u != v for u, v in zip(a, b)]


def checked_by_merging(p):
    overflowed = any(capture.prefix(e["table"][0], e["table"][1], *(p["cap"] or full_cap(p)))[2] for e in p["expect"])
    return len(p["sizes"]) > 1 and not overflowed


def exempt_counts(p):
    """-> (the exempt chains, all chains) of an auto or phase plan to which run_plan's merged check applies; (0, 0) of any other."""
    if not has_heads(p, p["measure"]) or not checked_by_merging(p):
        return 0, 0
    rsizes, rreset, _, _ = reference_cut(p)
    ex = exempt(p, [e["centres"] for e in restate(p, p["sizes"], p["reset"], ("track",))],
                [e["centres"] for e in restate(p, rsizes, rreset, ("track",), caps=False)])
    return sum(ex), len(ex)


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
        R.enable(r, [m for m in measure if m != "track"])
        if "track" in measure:
            mode = p.get("mode")
            R.enable_mode(r, mode, p["L"])
            if mode is not None and mode[0] == "amplitude":
                r.set_burst_track_level(range(n), mode[1])
            else:
                r.set_burst_track_centre(range(n), p["centres"])
        if sync_on(p, measure):
            st = p["sync"]
            R.enable(r, {"sync": (st.rate, st.pattern, st.P, st.E, st.both)})
        reads, states, pos = [], (None, None), 0
        for k, nb in enumerate(sizes):
            if p["reset"] and p["reset"][0] == k:
                r.reset_streams(p["reset"][1])
            r.submit(np.ascontiguousarray(p["x"][:, pos * B:(pos + nb) * B]))
            pos += nb
            keep = p["drains"][k] if k + 1 < len(sizes) else 0
            while keep is not None and k + 1 - len(reads) > keep:
                try:
                    got, states = _check_submit(r, p, len(reads), measure, states, newest=len(reads) == k)
                except AssertionError as err:
                    raise AssertionError("submit %d: %s" % (len(reads), err)) from None
                reads.append(got)
                r.drain()
        raises(api.E_STATE, r.read_captures)  # nothing undrained
    overflowed = any(capture.prefix(e["table"][0], e["table"][1], *(p["cap"] or full_cap(p)))[2] for e in p["expect"])
    if measure and len(sizes) > 1 and not overflowed:
        rsizes, rreset, mine, theirs = reference_cut(p)
        ref = restate(p, rsizes, rreset, measure, caps=False)
        skip = exempt(p, [g["centres"] for g in reads], [e["centres"] for e in ref]) if has_heads(p, measure) else None
        for m in tuple(measure) + (("sync",) if sync_on(p, measure) else ()):
            a, b = merged(m, [g[m] for g in reads], mine), merged(m, [e[m] for e in ref], theirs)
            if skip is not None and m in ("track", "sync"):  # a shorter head: the flags and the length alone
                assert len(a) == len(b) == len(skip), "chains %s: %d, want %d" % (m, len(a), len(b))
                for u, v, ex in zip(a, b, skip):
                    assert not ex or (int(u["flags"]), int(u["n_samples"])) == (int(v["flags"]), int(v["n_samples"])), "chains %s: an exempt chain" % m
                a, b = [u for u, ex in zip(a, skip) if not ex], [v for v, ex in zip(b, skip) if not ex]
            same_chains(m, a, b, "chains")
        if skip is not None:  # the centre records: a chain keeps its first piece's (track.merge_centres)
            key = lambda c: int(c["stream"])  # noqa: E731
            a = sorted(track.centre_chains([g["centres"] for g in reads], mine), key=key)
            b = sorted(track.centre_chains([e["centres"] for e in ref], theirs), key=key)
            for i, (u, v, ex) in enumerate(zip(a, b, skip)):
                if ex:
                    assert (int(u["flags"]), int(u["n_samples"])) == (int(v["flags"]), int(v["n_samples"])), "chains centres: an exempt chain"
                else:
                    assert u.tobytes() == v.tobytes(), "chains centres: chain %d (stream %d from %d): got %s want %s" % (
                        i, u["stream"], u["start_sample"], u.tolist(), v.tolist())
    return reads


def _round(rng, rnd, verbose=True, seed=None, receiver=None, srng=None, mrng=None):
    p = plan(rng, rnd, srng, mrng)
    try:
        reads = run_plan(p, receiver=receiver)
        runs = sum(len(g["table"][0]) for g in reads)
    except AssertionError as e:
        print("seed %s round %d: %s -> MISMATCH: %s" % (seed, rnd, describe(p), e), flush=True)
        return 1
    if verbose:
        print("seed %s round %d: %s runs %d -> ok" % (seed, rnd, describe(p), runs), flush=True)
    return 0


def campaign(seed: int, rounds: int, verbose: bool = True, receiver=None, modes: bool = False) -> int:
    """-> the number of bad rounds.  modes: round rnd runs the track in the mode ("amplitude", "auto", "phase")[rnd % 3]."""
    rng, srng, mrng = np.random.default_rng(seed), sync_rng(seed), mode_rng(seed) if modes else None
    return sum(_round(rng, rnd, verbose, seed, receiver, srng, mrng) for rnd in range(rounds))


def plans(seed: int, rounds: int, modes: bool = False):
    """The plans campaign(seed, rounds, modes=modes) draws, without a GPU."""
    rng, srng, mrng = np.random.default_rng(seed), sync_rng(seed), mode_rng(seed) if modes else None
    return [plan(rng, rnd, srng, mrng) for rnd in range(rounds)]


if __name__ == "__main__":
    n_bad = campaign(int(sys.argv[1]) if len(sys.argv) > 1 else 1, int(sys.argv[2]) if len(sys.argv) > 2 else 10, modes="modes" in sys.argv[3:])
    print("mismatches:", n_bad)
    sys.exit(1 if n_bad else 0)
