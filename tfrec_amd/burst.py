"""The burst meter (tfrec_amd_enable_burst_meter, include/tfrec_amd.h: tfrec_amd_burst) restated in numpy -- no GPU
needed.  Written from the header's definition alone; exact integers throughout.

Per run of the recorder's table: a histogram over 64 directions of the products z[k] conj(z[k-1]) of consecutive decimated samples
(fm_dev's cr, cj: the instantaneous frequency, bin b = 6000 b Hz at 384 kS/s), their sums, the run's energy and its peak.

  bursts             vectorised, from the definition: one submit's records from every stream's decimated samples, its run table
                     and the pair ahead of every stream's first sample;
  bursts_bruteforce  the same sample by sample, in Python integers;
  bin_of / bin_fast  the argmax bin of one product, and the evaluation the kernel uses (a quarter turn and 16 comparisons);
  merge              a chain of pieces -> one record;  chains: the chains of a sequence of submits;
  summary            centre and deviation of a record;  line: tfrec_gpu -M's output line.
"""
from __future__ import annotations

import numpy as np

from . import tune
from .capture import RUN_CONTINUES, RUN_OPEN

N_BINS = 64
BIN_HZ = 6000  # 384000 / 64
BURST_DTYPE = np.dtype([("stream", "<u4"), ("flags", "<u4"), ("start_sample", "<i8"), ("n_samples", "<u4"), ("thresh", "<i4"),
                        ("pwr_max", "<i4"), ("n_products", "<u4"), ("sum_dot", "<i8"), ("sum_crs", "<i8"), ("energy", "<u8"),
                        ("hist", "<u4", (N_BINS,)), ("reserved", "<u4", (2,))])
assert BURST_DTYPE.itemsize == 320
SUMMED = ("n_samples", "n_products", "sum_dot", "sum_crs", "energy", "hist")


def directions():
    """(C[64 j], S[64 j]), j = 0..63, of the project's one table, as Python ints."""
    c, s = tune.table()
    return [int(v) for v in c[::64]], [int(v) for v in s[::64]]


_C64, _S64 = directions()


def bin_of(dot: int, crs: int):
    """The definition: the j that maximises dot C[64 j] + crs S[64 j], the lowest on a tie; None for the zero product."""
    dot, crs = int(dot), int(crs)
    if dot == 0 and crs == 0:
        return None
    best, arg = None, 0
    for j in range(N_BINS):
        v = dot * _C64[j] + crs * _S64[j]
        if best is None or v > best:
            best, arg = v, j
    return arg


# boundary k of the first quarter, between directions k and k + 1: direction k + 1 scores higher iff y DS[k] > x DC[k]
_DS = [_S64[k + 1] - _S64[k] for k in range(16)]
_DC = [_C64[k] - _C64[k + 1] for k in range(16)]


def bin_fast(dot: int, crs: int):
    """The kernel's evaluation.  The table is exact under a quarter turn (C[64 (j + 16)] = -S[64 j], S[64 (j + 16)] = C[64 j]), so the
    product is turned into x > 0, y >= 0 by q quarter turns; there the score rises up to the argmax and falls behind it, because
    the ratios DC[k] / DS[k] increase strictly with k: the argmax is the count of boundaries with y DS[k] > x DC[k].  A tie keeps
    the lower direction, except between 63 and 0, which only the last quarter's last boundary can produce."""
    dot, crs = int(dot), int(crs)
    if dot == 0 and crs == 0:
        return None
    if dot > 0 and crs >= 0:
        q, x, y = 0, dot, crs
    elif dot <= 0 and crs > 0:
        q, x, y = 1, crs, -dot
    elif dot < 0 and crs <= 0:
        q, x, y = 2, -dot, -crs
    else:
        q, x, y = 3, -crs, dot
    n = 0
    for k in range(16):
        a, b = y * _DS[k], x * _DC[k]
        n += a > b or (k == 15 and q == 3 and a == b)
    return (16 * q + n) % N_BINS


def signed_bin(j: int) -> int:
    return j if j < N_BINS // 2 else j - N_BINS


def _pairs(a):
    a = np.asarray(a)
    assert a.dtype == np.int16, a.dtype
    return a.reshape(-1, 2)


def _bins(dot, crs):
    """bin_of over int64 arrays (no zero products among them): exact, the scores stay below 2^47."""
    c, s = np.array(_C64, dtype=np.int64), np.array(_S64, dtype=np.int64)
    out = np.empty(len(dot), dtype=np.int64)
    for i in range(0, len(dot), 1 << 16):  # (chunks: [n, 64] scores)
        sc = dot[i:i + (1 << 16), None] * c[None, :] + crs[i:i + (1 << 16), None] * s[None, :]
        out[i:i + (1 << 16)] = np.argmax(sc, axis=1)  # (the first maximum: the lowest j)
    return out


def _copied(run):
    o = np.zeros((), dtype=BURST_DTYPE)
    for f in ("stream", "flags", "n_samples", "thresh"):
        o[f] = run[f]
    o["start_sample"] = int(run["start_sample"])
    return o


def bursts(dec, runs, prev, base=None):
    """One submit's records.  dec[s]: stream s's decimated samples of the submit (int16 pairs, as tfrec_amd_read_decimated returns
    them); runs: the submit's table (RUN_DTYPE); prev[s]: the pair ahead of the submit's first sample (the stream's last pair of
    the submit before; only a CONTINUES run reads it); base[s]: the start_sample of the submit's first sample of stream s (default:
    0, a table relative to the submit) -> a BURST_DTYPE array, one record per table entry."""
    out = np.zeros(len(runs), dtype=BURST_DTYPE)
    for e, r in enumerate(runs):
        s = int(r["stream"])
        z = _pairs(dec[s]).astype(np.int64)
        a = int(r["start_sample"]) - (int(base[s]) if base is not None else 0)
        n = int(r["n_samples"])
        assert 0 <= a and a + n <= len(z) and n >= 1
        o = _copied(r)
        I, Q = z[a:a + n, 0], z[a:a + n, 1]
        o["pwr_max"] = int((np.abs(I) + np.abs(Q)).max())
        o["energy"] = int((I * I + Q * Q).sum())
        k0 = 0 if int(r["flags"]) & RUN_CONTINUES else 1
        if a > 0:
            p = z[a - 1]
        else:
            p = np.asarray(prev[s], dtype=np.int64).reshape(2)
        Ip, Qp = np.concatenate([[p[0]], I[:-1]])[k0:], np.concatenate([[p[1]], Q[:-1]])[k0:]
        dot = I[k0:] * Ip + Q[k0:] * Qp
        crs = Q[k0:] * Ip - I[k0:] * Qp
        live = (dot != 0) | (crs != 0)
        dot, crs = dot[live], crs[live]
        o["n_products"] = len(dot)
        o["sum_dot"], o["sum_crs"] = int(dot.sum()), int(crs.sum())
        o["hist"] = np.bincount(_bins(dot, crs), minlength=N_BINS)
        out[e] = o
    return out


def bursts_bruteforce(dec, runs, prev, base=None):
    """The same, one sample at a time in Python integers."""
    out = np.zeros(len(runs), dtype=BURST_DTYPE)
    for e, r in enumerate(runs):
        s = int(r["stream"])
        z = _pairs(dec[s]).tolist()
        a = int(r["start_sample"]) - (int(base[s]) if base is not None else 0)
        n = int(r["n_samples"])
        cont = bool(int(r["flags"]) & RUN_CONTINUES)
        hist = [0] * N_BINS
        pmax = np_ = sd = sc = en = 0
        for k in range(n):
            i, q = z[a + k]
            pmax = max(pmax, abs(i) + abs(q))
            en += i * i + q * q
            if k == 0 and not cont:
                continue
            ip, qp = z[a + k - 1] if a + k > 0 else [int(v) for v in np.asarray(prev[s]).reshape(2)]
            dot, crs = i * ip + q * qp, q * ip - i * qp
            j = bin_of(dot, crs)
            if j is None:
                continue
            hist[j] += 1
            np_ += 1
            sd += dot
            sc += crs
        o = _copied(r)
        o["pwr_max"], o["n_products"], o["sum_dot"], o["sum_crs"], o["energy"], o["hist"] = pmax, np_, sd, sc, en, hist
        out[e] = o
    return out


def merge(pieces):
    """A chain of pieces (in order; piece i + 1 has CONTINUES, piece i OPEN, one stream) -> one record: the first piece's stream,
    start_sample and thresh, the first piece's CONTINUES and the last one's OPEN, the sums added, the largest pwr_max."""
    pieces = list(pieces)
    o = pieces[0].copy()
    for p in pieces[1:]:
        assert p["stream"] == o["stream"] and int(p["flags"]) & RUN_CONTINUES
        for f in SUMMED:
            o[f] = o[f] + p[f]
        o["pwr_max"] = max(int(o["pwr_max"]), int(p["pwr_max"]))
    o["flags"] = (int(pieces[0]["flags"]) & RUN_CONTINUES) | (int(pieces[-1]["flags"]) & RUN_OPEN)
    return o


def chains(submits, restarts=None, join=None):
    """submits: one BURST_DTYPE array per submit, in order -> the merged bursts, in the order in which they end (per submit: table
    order), a chain still open behind the last submit last (by stream).  restarts: {submit index: streams that restart with it}:
    their open chains end there.  join: what merges a chain's pieces (default: merge; envelope.py passes its own).
    A chain whose last piece is OPEN and which the next submit does not continue ended with that piece's last sample, the submit's
    last: the trigger's hold ran out exactly there.  Its record is complete, and OPEN is cleared, as in the uncut run's record."""
    join = join or merge
    open_, out = {}, []

    def ended(o):  # (a restart's and the last submit's chains keep OPEN: what lies behind them is not known)
        o["flags"] = int(o["flags"]) & ~RUN_OPEN
        return o

    for k, recs in enumerate(submits):
        for s in sorted((restarts or {}).get(k, ())):
            if s in open_:
                out.append(join(open_.pop(s)))
        seen = set()
        for r in recs:
            s = int(r["stream"])
            fl = int(r["flags"])
            if fl & RUN_CONTINUES and s in open_:
                open_[s].append(r)
            else:
                if s in open_:  # the chain ended with the submit before; this run began later in this one
                    out.append(ended(join(open_.pop(s))))
                open_[s] = [r]
            seen.add(s)
            if not fl & RUN_OPEN:
                out.append(join(open_.pop(s)))
        for s in sorted(set(open_) - seen):  # open, and nothing of the stream at this submit's first sample: the trigger ended there
            out.append(ended(join(open_.pop(s))))
    for s in sorted(open_):
        out.append(join(open_[s]))
    return out


def summary(rec):
    """-> (centre_hz, deviation_hz), or None when no bin is occupied (no carrier: noise spreads over the bins).  A bin is occupied
    iff P = n_products > 0 and hist[j] >= (P + 15) // 16; lo, hi: the smallest and largest signed index of an occupied bin."""
    P = int(rec["n_products"])
    if P == 0:
        return None
    thr = (P + 15) // 16
    occ = [signed_bin(j) for j in range(N_BINS) if int(rec["hist"][j]) >= thr]
    if not occ:
        return None
    lo, hi = min(occ), max(occ)
    return 3000 * (lo + hi), 3000 * (hi - lo)


def line(name: str, rec) -> str:
    """tfrec_gpu -M: burst <file> <start_sample> <n_samples> <pwr_max> <centre_hz|-> <deviation_hz|->"""
    sm = summary(rec)
    return "burst %s %d %d %d %s %s" % (name, int(rec["start_sample"]), int(rec["n_samples"]), int(rec["pwr_max"]),
                                        "-" if sm is None else "%d" % sm[0], "-" if sm is None else "%d" % sm[1])
