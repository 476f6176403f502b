"""The squelched recorder (tfrec_amd_enable_capture, include/tfrec_amd.h: tfrec_amd_run) restated in numpy -- no GPU
needed.

Sample n of a stream is captured iff it is `triggered` in the sense of tfrec_amd_level: a sample n' with pwr > thresh lies in
(n - W, n], W the largest window of the stream's registered demodulators.  A run is a maximal set of consecutive captured
samples within one call (one submit); the pool holds the runs' (I, Q) pairs back to back.  Two forms, as in levels.py:

  captures             vectorised, from the definition in the header;
  captures_bruteforce  a per-sample simulation from the reference's text: one timeout_cnt per registered demodulator, set to its
                       window at pwr > thresh, counted while non-zero, then decremented (tfa1.cpp:147-164, tfa2.cpp:351-375,
                       whb.cpp:636-657); a sample is captured when any demodulator returned non-zero (fm_demod.cpp:48-52).

Both take ONE stream's decimated samples as tfrec_amd_read_decimated returns them, its -T mask and its -t (0: auto), and a `state`
to continue the stream over several calls; both return (runs, pool, state): runs a RUN_DTYPE array with stream = 0 and pool_offset
counted within this call's pool, pool an int16 array [n_pairs, 2].  table() puts several streams' results together as
tfrec_amd_read_captures returns them, prefix() cuts a table as a device-side overflow does.
"""
from __future__ import annotations

import numpy as np

from . import levels
from .levels import BLOCK_DEC

RUN_CONTINUES = 1
RUN_OPEN = 2
RUN_DTYPE = np.dtype([("stream", "<u4"), ("flags", "<u4"), ("start_sample", "<i8"), ("n_samples", "<u4"), ("thresh", "<i4"),
                      ("pool_offset", "<u8")])
assert RUN_DTYPE.itemsize == 32


def _pairs(dec):
    a = np.asarray(dec)
    assert a.dtype == np.int16, a.dtype
    a = a.reshape(-1, 2)
    assert len(a) % BLOCK_DEC == 0, "whole blocks of %d decimated samples" % BLOCK_DEC
    return a


def _runs_of(captured, thr, prev, n0, pairs):
    """The runs of one call: captured[M] bool, thr[M] the threshold in force at every sample, prev: the sample before the call's
    first was captured (and no restart lies between), n0: the stream's samples before this call."""
    M = len(captured)
    c = captured.astype(np.int8)
    edge = np.diff(np.concatenate([[0], c, [0]]))
    starts, ends = np.flatnonzero(edge == 1), np.flatnonzero(edge == -1)  # [start, end)
    runs = np.zeros(len(starts), dtype=RUN_DTYPE)
    runs["start_sample"] = n0 + starts
    runs["n_samples"] = ends - starts
    runs["thresh"] = thr[starts] if len(starts) else 0
    runs["flags"] = np.where((starts == 0) & prev, RUN_CONTINUES, 0) | np.where(ends == M, RUN_OPEN, 0)
    runs["pool_offset"] = np.concatenate([[0], np.cumsum(ends - starts)[:-1]]) if len(starts) else 0
    pool = np.ascontiguousarray(pairs[captured])
    return runs, pool


def captures(dec, types_mask: int, thresh: int, state: dict | None = None):
    """-> (runs, pool, state).  state: None for a fresh stream (or one that restarts here), else what an earlier call returned
    for the samples just before these."""
    pairs = _pairs(dec)
    I, Q = pairs[:, 0].astype(np.int64), pairs[:, 1].astype(np.int64)
    W = max(levels.windows(types_mask))
    st = dict(state) if state is not None else dict(levels._start(thresh), n=0)
    nb = len(I) // BLOCK_DEC
    idx = np.arange(BLOCK_DEC, dtype=np.int64)
    last = st["last_trig"]  # relative to the current block's first sample
    prev = -1 - last < W  # the sample before this call's first lies inside a trigger's window
    captured = np.zeros(len(I), dtype=bool)
    thr = np.zeros(len(I), dtype=np.int64)
    for b in range(nb):
        sl = slice(b * BLOCK_DEC, (b + 1) * BLOCK_DEC)
        over = np.abs(I[sl]) + np.abs(Q[sl]) > st["thresh"]
        st["runs"] += 1
        lt = np.maximum(np.maximum.accumulate(np.where(over, idx, levels._NO_WINDOW)), last)
        captured[sl] = idx - lt < W
        thr[sl] = st["thresh"]
        levels._step(st, int(np.count_nonzero(captured[sl])))
        last = max(int(lt[-1]) - BLOCK_DEC, levels._NO_WINDOW)
    st["last_trig"] = last
    runs, pool = _runs_of(captured, thr, prev, st["n"], pairs)
    st["n"] += len(I)
    return runs, pool, st


def captures_bruteforce(dec, types_mask: int, thresh: int, state: dict | None = None):
    """The same from a sample-by-sample run of the reference's loops.  Its state carries the demodulators' timeout counters (and
    whether the last sample was captured) instead of a last trigger; the two kinds of state are not interchangeable."""
    pairs = _pairs(dec)
    win = levels.windows(types_mask)
    if state is not None:
        st = dict(state)
        cnt = list(st["timeout_cnt"])
    else:
        st = dict(levels._start(thresh), n=0, prev=False)
        del st["last_trig"]
        cnt = [0] * len(win)  # tfa1.cpp:140, tfa2.cpp:319, whb.cpp:608
    Il, Ql = pairs[:, 0].tolist(), pairs[:, 1].tolist()
    M = len(Il)
    captured = np.zeros(M, dtype=bool)
    thr = np.zeros(M, dtype=np.int64)
    for b in range(M // BLOCK_DEC):
        st["runs"] += 1  # fm_demod.cpp:37
        th = st["thresh"]
        triggered = 0
        for n in range(b * BLOCK_DEC, (b + 1) * BLOCK_DEC):
            pwr = abs(Il[n]) + abs(Ql[n])  # fm_demod.cpp:45
            t = 0
            for k, w in enumerate(win):  # demodulator::demod, fm_demod.cpp:48-49
                if pwr > th:
                    cnt[k] = w
                if cnt[k]:
                    t += 1
                    cnt[k] -= 1
            if t:
                triggered += 1  # fm_demod.cpp:51-52
                captured[n] = True
            thr[n] = th
        levels._step(st, triggered)
    runs, pool = _runs_of(captured, thr, st["prev"], st["n"], pairs)
    st["timeout_cnt"] = cnt
    st["prev"] = bool(M and captured[-1])
    st["n"] += M
    return runs, pool, st


def table(per_stream):
    """per_stream: [(runs, pool)] of streams 0, 1, ... for one submit -> (table, pool) as tfrec_amd_read_captures returns them:
    ordered by (stream, start_sample), the pool in table order, pool_offset its exclusive prefix sum."""
    runs = [r.copy() for r, _ in per_stream]
    off = 0
    for s, (r, (_, p)) in enumerate(zip(runs, per_stream)):
        r["stream"] = s
        r["pool_offset"] += off
        off += len(p)
    pools = [p for _, p in per_stream]
    return (np.concatenate(runs) if runs else np.zeros(0, dtype=RUN_DTYPE),
            np.concatenate(pools) if pools else np.zeros((0, 2), dtype=np.int16))


def prefix(runs, pool, max_runs: int, max_samples: int):
    """What a context enabled with (max_runs, max_samples) delivers of a submit's table: the longest prefix that fits both limits,
    whole runs only -> (runs, pool, overflow)."""
    end = runs["pool_offset"].astype(np.int64) + runs["n_samples"]
    k = 0
    while k < len(runs) and k < max_runs and end[k] <= max_samples:
        k += 1
    n = int(end[k - 1]) if k else 0
    return runs[:k], pool[:n], len(runs) > max_runs or len(pool) > max_samples


def idx_line(file_index: int, run) -> str:
    """tfrec_gpu -S: one run's line of <prefix>.idx."""
    return "%d %d %d %d %d %d" % (file_index, int(run["stream"]), int(run["start_sample"]), int(run["n_samples"]), int(run["thresh"]),
                                  int(run["flags"]))
