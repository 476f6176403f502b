"""The burst correlator (tfrec_amd_enable_burst_corr, include/tfrec_amd.h: tfrec_amd_corr) restated in numpy -- no GPU
needed.  Written from the header's definition alone; exact integers throughout.

Per run of the recorder's table and per sync template (a word at a rate, up to 16): the largest and the smallest score of a soft
matched filter over the burst's per-sample direction (the burst meter's 6 kHz bin about one centre), where each ends, the defined
positions and the sum of |score|.  Nothing here has been measured on real recordings.

  Settings           the templates and the centre, checked as the enable call checks them;  template: one template's taps;
  soft               a run's soft samples u[k];
  corrs              vectorised, from the definition: one submit's records from every stream's decimated samples, its run table, the
                     pair ahead of every stream's first sample and the state the submit before left;
  corrs_bruteforce   the same position by position, in Python integers, as the header words it;
  merge              a chain of pieces -> the record of the uncut run;  chains: the chains of a sequence of submits (burst.chains' walk);
  summary            per template (polarity, dev_hz, quality_c, end) and the best one;  line: tfrec_gpu -y's output line;
  device_bytes       what tfrec_amd_enable_burst_corr adds to tfrec_amd_get_memory (pinned_bytes: nothing).
"""
from __future__ import annotations

import numpy as np

from . import burst
from .capture import RUN_CONTINUES, RUN_OPEN

HISTORY = 2047  # the soft samples carried from submit to submit
MAX_TAPS = 2048
MAX_TEMPLATES = 16
NONE_PEAK, NONE_TROUGH = -(1 << 31), (1 << 31) - 1
SCORE_DTYPE = np.dtype([("peak", "<i4"), ("peak_at", "<u4"), ("trough", "<i4"), ("trough_at", "<u4"), ("n_pos", "<u4"),
                        ("reserved", "<u4"), ("sum_abs", "<u8")])
CORR_DTYPE = np.dtype([("stream", "<u4"), ("flags", "<u4"), ("start_sample", "<i8"), ("n_samples", "<u4"), ("thresh", "<i4"),
                       ("t", SCORE_DTYPE, (MAX_TEMPLATES,))])
assert SCORE_DTYPE.itemsize == 32 and CORR_DTYPE.itemsize == 536


def template(pattern: int, n_bits: int, rate: int) -> np.ndarray:
    """T[0 .. K - 1], K = b(P): symbol i (0: the first transmitted, the pattern's bit P - 1) covers the taps [b(i), b(i + 1)), b(i) =
    floor(384000 i / R), +1 for a 1 bit and -1 for a 0 bit (int64)."""
    P, R = int(n_bits), int(rate)
    b = [384000 * i // R for i in range(P + 1)]
    t = np.zeros(b[P], dtype=np.int64)
    for i in range(P):
        t[b[i]:b[i + 1]] = 1 if (int(pattern) >> (P - 1 - i)) & 1 else -1
    return t


class Settings:
    """What tfrec_amd_enable_burst_corr fixes; a ValueError where it returns E_INVAL.  templates: (pattern, n_bits, rate) each."""

    def __init__(self, templates, centre_hz: int = 0):
        self.templates = [(int(p) & ((1 << int(b)) - 1), int(b), int(r)) for p, b, r in templates]
        self.centre_hz = int(centre_hz)
        if not 1 <= len(self.templates) <= MAX_TEMPLATES:
            raise ValueError("%d templates outside 1 .. 16" % len(self.templates))
        if abs(self.centre_hz) > 192000:
            raise ValueError("centre %d Hz outside +-192000" % self.centre_hz)
        for _, b, r in self.templates:
            if not 1000 <= r <= 96000:
                raise ValueError("rate %d outside 1000 .. 96000" % r)
            if not 8 <= b <= 64:
                raise ValueError("%d pattern bits outside 8 .. 64" % b)
            if 384000 * b // r > MAX_TAPS:
                raise ValueError("%d taps above %d" % (384000 * b // r, MAX_TAPS))
        self.c = (self.centre_hz + 3000) // 6000  # (Python's //: a true floor)
        self.taps = [template(*t) for t in self.templates]
        self.K = [len(t) for t in self.taps]
        self.Kp = (max(self.K) + 63) // 64 * 64

    def arrays(self):
        """(patterns uint64, bits int32, rates int32), as the C call takes them."""
        return (np.array([t[0] for t in self.templates], dtype=np.uint64), np.array([t[1] for t in self.templates], dtype=np.int32),
                np.array([t[2] for t in self.templates], dtype=np.int32))


def fresh_state(n_streams: int) -> dict:
    """What a context carries before its first submit: no history."""
    return {"soft": [np.zeros(0, dtype=np.int64) for _ in range(n_streams)]}


def soft(z, a: int, n: int, prev, cont: bool, c: int) -> np.ndarray:
    """u[0 .. n - 1] of the run at [a, a + n) of a stream's pairs z (int64 [m, 2]); prev: the pair ahead of z[0] (int64)."""
    I, Q = z[a:a + n, 0], z[a:a + n, 1]
    p = z[a - 1] if a > 0 else np.asarray(prev, dtype=np.int64).reshape(2)
    Ip, Qp = np.concatenate([[p[0]], I[:-1]]), np.concatenate([[p[1]], Q[:-1]])
    dot, crs = I * Ip + Q * Qp, Q * Ip - I * Qp
    live = (dot != 0) | (crs != 0)
    if not cont:
        live[0] = False
    u = np.zeros(n, dtype=np.int64)
    j = burst._bins(dot[live], crs[live])
    u[live] = np.where(j < burst.N_BINS // 2, j, j - burst.N_BINS) - c
    return u


def _copied(run):
    o = np.zeros((), dtype=CORR_DTYPE)
    for f in ("stream", "flags", "n_samples", "thresh"):
        o[f] = run[f]
    o["start_sample"] = int(run["start_sample"])
    o["t"]["peak"], o["t"]["trough"] = NONE_PEAK, NONE_TROUGH
    return o


def _fits(run, max_samples) -> bool:
    return max_samples is None or int(run["pool_offset"]) + int(run["n_samples"]) <= max_samples


def _walk(dec, runs, prev, settings, state, n_streams, max_samples, base, score):
    """What corrs and corrs_bruteforce share: the runs' soft samples and histories, the records' copied fields, the next state."""
    if n_streams is None:
        n_streams = len(state["soft"]) if state is not None else len(dec)
    state = fresh_state(n_streams) if state is None else state
    nxt = fresh_state(n_streams)
    out = np.zeros(len(runs), dtype=CORR_DTYPE)
    for e, r in enumerate(runs):
        s = int(r["stream"])
        o = _copied(r)
        if _fits(r, max_samples):
            z = np.asarray(dec[s]).reshape(-1, 2).astype(np.int64)
            a = int(r["start_sample"]) - (int(base[s]) if base is not None else 0)
            n = int(r["n_samples"])
            assert 0 <= a and a + n <= len(z) and n >= 1
            cont = bool(int(r["flags"]) & RUN_CONTINUES)
            u = soft(z, a, n, prev[s], cont, settings.c)
            h = state["soft"][s][-HISTORY:] if cont else np.zeros(0, dtype=np.int64)
            for t in range(len(settings.K)):
                score(o["t"][t], h, u, settings.taps[t])
            if int(r["flags"]) & RUN_OPEN:
                nxt["soft"][s] = np.concatenate([h, u])[-HISTORY:]
        out[e] = o
    return out, nxt


def _score_fast(o, h, u, T):
    H, K, n = len(h), len(T), len(u)
    k0 = max(0, K - 1 - H)  # the first defined k
    if k0 >= n:
        return
    ext = np.concatenate([h, u])
    y = np.correlate(ext[H + k0 - K + 1:], T, mode="valid")  # y[i] = Y[k0 + i] (int64: exact)
    ip, it = int(np.argmax(y)), int(np.argmin(y))  # (the first of each)
    o["peak"], o["peak_at"], o["trough"], o["trough_at"] = int(y[ip]), k0 + ip, int(y[it]), k0 + it
    o["n_pos"], o["sum_abs"] = len(y), int(np.abs(y).sum())


def _score_brute(o, h, u, T):
    hl, ul, Tl = [int(v) for v in h], [int(v) for v in u], [int(v) for v in T]
    H, K = len(hl), len(Tl)

    def at(k):  # u[k], k >= -H
        return ul[k] if k >= 0 else hl[H + k]

    peak, trough, peak_at, trough_at, n_pos, sum_abs = NONE_PEAK, NONE_TROUGH, 0, 0, 0, 0
    for k in range(len(ul)):
        if k + H < K - 1:
            continue
        y = sum(at(k - K + 1 + i) * Tl[i] for i in range(K))
        if n_pos == 0 or y > peak:
            peak, peak_at = y, k
        if n_pos == 0 or y < trough:
            trough, trough_at = y, k
        n_pos += 1
        sum_abs += abs(y)
    o["peak"], o["peak_at"], o["trough"], o["trough_at"], o["n_pos"], o["sum_abs"] = peak, peak_at, trough, trough_at, n_pos, sum_abs


def corrs(dec, runs, prev, settings: Settings, state=None, n_streams=None, max_samples=None, base=None):
    """One submit.  dec[s], runs, prev[s], base[s]: as burst.bursts takes them (runs: RUN_DTYPE, with the entry's place in the pool);
    state: what the submit before returned (default: a fresh context's); max_samples: the pool's size (default: everything fits)
    -> (a CORR_DTYPE array, one record per table entry; the state behind the submit)."""
    return _walk(dec, runs, prev, settings, state, n_streams, max_samples, base, _score_fast)


def corrs_bruteforce(dec, runs, prev, settings: Settings, state=None, n_streams=None, max_samples=None, base=None):
    """The same, one position at a time in Python integers: Y_t[k] = sum over i < K_t of u[k - K_t + 1 + i] T_t[i]."""
    return _walk(dec, runs, prev, settings, state, n_streams, max_samples, base, _score_brute)


def merge(pieces):
    """A chain of pieces (in order, as for burst.merge) -> the record of the uncut run: n_samples, n_pos and sum_abs added, the larger
    peak and the smaller trough -- on a tie the earlier piece's -- with *_at offset by the samples ahead; the flags as burst.merge's."""
    pieces = list(pieces)
    o = pieces[0].copy()
    for p in pieces[1:]:
        assert p["stream"] == o["stream"] and int(p["flags"]) & RUN_CONTINUES
        ahead = int(o["n_samples"])
        for t in range(MAX_TEMPLATES):
            a, b = o["t"][t], p["t"][t]
            if int(b["n_pos"]) and (not int(a["n_pos"]) or int(b["peak"]) > int(a["peak"])):
                a["peak"], a["peak_at"] = int(b["peak"]), ahead + int(b["peak_at"])
            if int(b["n_pos"]) and (not int(a["n_pos"]) or int(b["trough"]) < int(a["trough"])):
                a["trough"], a["trough_at"] = int(b["trough"]), ahead + int(b["trough_at"])
            a["n_pos"] = int(a["n_pos"]) + int(b["n_pos"])
            a["sum_abs"] = int(a["sum_abs"]) + int(b["sum_abs"])
        o["n_samples"] = ahead + int(p["n_samples"])
    o["flags"] = (int(pieces[0]["flags"]) & RUN_CONTINUES) | (int(pieces[-1]["flags"]) & RUN_OPEN)
    return o


def chains(submits, restarts=None):
    """submits: one CORR_DTYPE array per submit, in order -> the merged bursts, in burst.chains' order."""
    return burst.chains(submits, restarts, join=merge)


def summary(rec, settings: Settings):
    """-> (best, figures): figures[t] = (polarity, dev_hz, quality_c or None, end) or None where n_pos is 0 -- m = max(peak, -trough),
    polarity '+' iff peak >= -trough, dev_hz = floor(6000 m / K_t), quality_c = floor(100 m n_pos / sum_abs), end = the winning
    extreme's run-relative position --; best = the index of the largest dev_hz, the lowest on a tie, or None."""
    fig, best = [], None
    for t, K in enumerate(settings.K):
        x = rec["t"][t]
        if not int(x["n_pos"]):
            fig.append(None)
            continue
        peak, trough = int(x["peak"]), int(x["trough"])
        plus = peak >= -trough
        m = max(peak, -trough)
        sa = int(x["sum_abs"])
        fig.append(("+" if plus else "-", 6000 * m // K, 100 * m * int(x["n_pos"]) // sa if sa else None,
                    int(x["peak_at"] if plus else x["trough_at"])))
        if best is None or fig[t][1] > fig[best][1]:
            best = t
    return best, fig


def line(name: str, rec, settings: Settings) -> str:
    """tfrec_gpu -y: corr <file> <start_sample> <n_samples> <best|-> <end_sample|-> <+|-> <dev_hz|-> <quality_c|-> <dev_hz of every
    template, comma separated, - where undefined>"""
    best, fig = summary(rec, settings)
    start = int(rec["start_sample"])
    head = "corr %s %d %d" % (name, start, int(rec["n_samples"]))
    every = ",".join("-" if f is None else "%d" % f[1] for f in fig)
    if best is None:
        return "%s - - - - - %s" % (head, every)
    pol, dev, q, end = fig[best]
    return "%s %d %d %s %d %s %s" % (head, best, start + end, pol, dev, "-" if q is None else "%d" % q, every)


def device_bytes(n_streams: int, max_blocks: int, max_runs: int, max_samples: int, settings: Settings) -> int:
    """What tfrec_amd_enable_burst_corr adds to tfrec_amd_get_memory's device bytes: per FIFO set the records; once, the soft bytes, the
    work list (a stream's runs hold at most 32 max_blocks whole tiles and a partial one each) with its length, the bank, and per stream
    the carried 2048 bytes and H."""
    from .api import FIFO_DEPTH
    stage_cap = max_blocks * 8192 // 356 + 3
    return (FIFO_DEPTH * max_runs * CORR_DTYPE.itemsize + max_samples + 8 * n_streams * (32 * max_blocks + stage_cap) + 4
            + 16 * settings.Kp + n_streams * (2048 + 4))


def pinned_bytes(n_streams: int) -> int:
    """... and to its page-locked bytes: nothing."""
    return 0
