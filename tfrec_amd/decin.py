"""Channel-rate input (tfrec_amd_create_decimated, tfrec_amd_enable_capture_pre, tfrec_amd_submit_runs; include/tfrec_amd.h, DESIGN.md
6n) restated in numpy -- no GPU needed.

A channel-rate context takes rows of int16 (I, Q) pairs at 384 kS/s, the samples process_iq produces.  Its front end is a clamp and
a comparison:

  clamp        v' = max(v, -32767) per component: what tfrec_amd_read_decimated returns;
  mask         |I'| + |Q'| > thresh, the trigger test of tfa1.cpp:147, tfa2.cpp:351 and whb.cpp:636.

The recorder (capture.py) keeps the triggered samples and their positions; a stream's flush events depend on one thing more, the
sample ahead of every run (the first fm_dev / fm_dev_nrzs of a window reads it: last_i / last_q are written outside the windows too,
tfa1.cpp:186-187, tfa2.cpp:438-439, whb.cpp:702-705):

  pre_samples  the pair ahead of every run of a submit's table (tfrec_amd_read_capture_pre);
  expand       what tfrec_amd_submit_runs means: the dense rows of a table, a pool and the pre samples, and per row the pair that
               replaces the carried "sample ahead of the submit" (a run at the submit's first sample brings its own);
  rebase       tables with absolute start_sample -> the table of one submit [base, base + M): runs are cut at the submit's
               boundaries (the second part's pre is the first part's last pair) and runs that touch are joined;
  check        the rule list of tfrec_amd_submit_runs -> None, or the rule that is violated.
"""
from __future__ import annotations

import numpy as np

from .capture import RUN_DTYPE
from .levels import BLOCK_DEC

FMT_DEC16 = 16  # TFREC_AMD_FMT_DEC16
BLOCK_BYTES = 4 * BLOCK_DEC


def clamp(x) -> np.ndarray:
    """int16 values -> max(v, -32767)."""
    a = np.asarray(x)
    assert a.dtype == np.int16, a.dtype
    return np.maximum(a, np.int16(-32767))


def mask(dec, thresh: int) -> np.ndarray:
    """The trigger bits of clamped pairs [..., 2] at a fixed threshold."""
    a = np.asarray(dec).astype(np.int64)
    if a.shape[-1] != 2:
        a = a.reshape(-1, 2)  # I and Q interleaved
    return np.abs(a[..., 0]) + np.abs(a[..., 1]) > thresh


def _pairs(a, what) -> np.ndarray:
    a = np.asarray(a)
    assert a.dtype == np.int16, (what, a.dtype)
    return a.reshape(-1, 2)


def pre_samples(dec, runs, prev_last=None, base=0) -> np.ndarray:
    """dec[n_streams, M, 2]: every stream's decimated samples of ONE submit; runs: the submit's table; prev_last[n_streams, 2]: every
    stream's last pair of the submit before, None or (0, 0) where nothing precedes; base: start_sample of the submit's first sample
    (one value, or one per stream) -> int16 [n_runs, 2]."""
    d = np.asarray(dec)
    assert d.dtype == np.int16 and d.ndim == 3 and d.shape[2] == 2, (d.dtype, d.shape)
    prev = np.zeros((d.shape[0], 2), dtype=np.int16) if prev_last is None else np.asarray(prev_last, dtype=np.int16).reshape(-1, 2)
    b = np.broadcast_to(np.asarray(base, dtype=np.int64), (d.shape[0],))
    out = np.zeros((len(runs), 2), dtype=np.int16)
    for i, r in enumerate(runs):
        s = int(r["stream"])
        rel = int(r["start_sample"]) - int(b[s])
        assert 0 <= rel < d.shape[1]
        out[i] = d[s, rel - 1] if rel > 0 else prev[s]
    return out


def expand(runs, pool, pre, n_blocks: int, n_rows: int):
    """-> (rows int16 [n_rows, M, 2], override {row: (I, Q)}): the dense rows tfrec_amd_submit_runs stands for -- not yet clamped, as
    little as the rows of a dense submit are -- and, for every row with a run at sample 0, the pair that is that row's sample ahead
    of the submit."""
    M = n_blocks * BLOCK_DEC
    p, q = _pairs(pool, "pool"), _pairs(pre, "pre")
    rows = np.zeros((n_rows, M, 2), dtype=np.int16)
    override = {}
    for i, r in enumerate(runs):
        s, a, n, o = int(r["stream"]), int(r["start_sample"]), int(r["n_samples"]), int(r["pool_offset"])
        rows[s, a:a + n] = p[o:o + n]
        if a > 0:
            rows[s, a - 1] = q[i]
        else:
            override[s] = (int(q[i][0]), int(q[i][1]))
    return rows, override


def check(runs, n_pairs: int, n_blocks: int, n_streams: int, max_runs: int | None = None, max_samples: int | None = None,
          mapped: bool = False):
    """The rules of tfrec_amd_submit_runs -> None when the table is accepted, else a word for the rule it violates."""
    M = n_blocks * BLOCK_DEC
    if mapped:
        return "mapped"
    if (max_runs is not None and len(runs) > max_runs) or (max_samples is not None and n_pairs > max_samples):
        return "limits"
    total = 0
    for i, r in enumerate(runs):
        s, a, n, o = int(r["stream"]), int(r["start_sample"]), int(r["n_samples"]), int(r["pool_offset"])
        if not 0 <= s < n_streams:
            return "stream"
        if not 0 <= a < M:
            return "start"
        if n < 1 or a + n > M:
            return "length"
        if o != total:
            return "pool_offset"
        if i:
            ps, pa, pn = int(runs[i - 1]["stream"]), int(runs[i - 1]["start_sample"]), int(runs[i - 1]["n_samples"])
            if s < ps or (s == ps and a <= pa):
                return "order"
            if s == ps and a < pa + pn + 1:
                return "gap"
        total += n
    return None if total == n_pairs else "n_pairs"


def rebase(runs, pool, pre, base: int, M: int):
    """runs with start_sample counted from the stream's start (several submits' tables put together, pool_offset into `pool`, pre[i]
    ahead of run i) -> (runs, pool, pre) of the submit that covers [base, base + M): start_sample relative to base, runs cut at both
    ends -- a part that begins inside a run has the run's pair before it as its pre --, runs of a stream that touch joined, the
    pool repacked in table order.  flags and thresh are kept from the run a part begins in."""
    p, q = _pairs(pool, "pool"), _pairs(pre, "pre")
    order = np.lexsort((runs["start_sample"], runs["stream"]))
    out, pools, pres = [], [], []
    for i in order:
        r = runs[i]
        s, a, n, o = int(r["stream"]), int(r["start_sample"]), int(r["n_samples"]), int(r["pool_offset"])
        lo, hi = max(a, base), min(a + n, base + M)
        if lo >= hi:
            continue
        part = p[o + lo - a:o + hi - a]
        if out and int(out[-1]["stream"]) == s and int(out[-1]["start_sample"] + out[-1]["n_samples"]) == lo - base:
            out[-1]["n_samples"] += hi - lo
            pools.append(part)
            continue
        e = np.zeros((), dtype=RUN_DTYPE)
        e["stream"], e["flags"], e["thresh"] = s, r["flags"], r["thresh"]
        e["start_sample"], e["n_samples"] = lo - base, hi - lo
        out.append(e)
        pools.append(part)
        pres.append(q[i] if lo == a else p[o + lo - a - 1])
    table = np.array(out, dtype=RUN_DTYPE) if out else np.zeros(0, dtype=RUN_DTYPE)
    if len(table):
        table["pool_offset"] = np.concatenate([[0], np.cumsum(table["n_samples"])[:-1]])
    return (table, np.concatenate(pools) if pools else np.zeros((0, 2), dtype=np.int16),
            np.array(pres, dtype=np.int16).reshape(-1, 2))
