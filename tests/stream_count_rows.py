"""The inputs of tests/test_stream_counts_gpu.py -- 65 and 97 streams: a full wave or workgroup of streams and a partial one behind
it --, their oracles, restatements and plans, without a GPU.  tests/test_stream_counts_cpu.py asserts every condition the GPU tests
assume about them.  Imported as a plain module (`import stream_count_rows`).

97 = 3 * 32 + 1 = 64 + 33: whb_chain_kernel's fourth workgroup holds one stream, the second step of 64 holds 33.
65 = 2 * 32 + 1 = 64 + 1:  the second step of 64 holds one stream."""
import functools

import numpy as np

import recorder_rows as RR
import segments
from input_rows import CFGS, DFLT, ROW_TUNES, ROWS
from oracle import oracle as O
from tfrec_amd import capture, synth

COUNTS = (65, 97)


def rows_of(n, unique):
    """The row stream s of n reads: its own among the first `unique`, a copy of row s mod unique behind them."""
    return np.arange(n) % unique


def per_stream(orc, n):
    """The oracle's events of n streams on the rows of rows_of."""
    return [orc[j] for j in rows_of(n, len(orc))]


# ---- 1. the main chain
CHAIN_UNIQUE, CHAIN_SIZES = 32, (1, 3, 2)


@functools.lru_cache(maxsize=None)
def chain_rows():
    iq = synth.gen_batch(97, 0, CHAIN_UNIQUE, sum(CHAIN_SIZES))
    iq.setflags(write=False)
    return iq


@functools.lru_cache(maxsize=None)
def chain_oracle():
    return O.process_many(chain_rows(), 0x2F, 500)


# ---- 2. the WHB check
WHB_UNIQUE, WHB_BLOCKS = 64, 24  # (a): the input of test_whb_speculation_is_verified_and_rarely_fails
REDO_SIZES = (2, 1, 4, 3, 2)     # (b): forced failures
CARRY_SIZES = (2, 3, 1, 1, 2, 3)  # (c): perturbed averages


@functools.lru_cache(maxsize=None)
def whb_rows():
    iq = synth.gen_batch(92, 0, WHB_UNIQUE, WHB_BLOCKS)
    iq.setflags(write=False)
    return iq


@functools.lru_cache(maxsize=None)
def whb_oracle():
    return O.process_many(whb_rows(), 0x20, 500)


@functools.lru_cache(maxsize=None)
def redo_rows():
    iq = synth.gen_batch(91, 3, WHB_UNIQUE, sum(REDO_SIZES))
    iq.setflags(write=False)
    return iq


@functools.lru_cache(maxsize=None)
def redo_oracle(types):
    return O.process_many(redo_rows(), types, 500)


# ---- 3. shared rows and per-stream operations
SHARED_N, SHARED_SIZES, SHARED_SEED = 97, (2, 1, 2, 1), 51
SHARED_CFGS = dict(CFGS)
SHARED_CFGS.update({31: (0x2F, 0, 0), 32: (0x03, 500, 1), 63: (0x21, 300, 0), 64: (0x2F, 900, 1), 65: (0x2F, 0, 0), 96: (0x0E, 500, 0)})
SHARED_BIG_RESET = list(range(20, 90))


def shared_plan():
    """test_shared_rows' scheme at 97 receivers -> (rows0, ops)."""
    n = SHARED_N
    rows0 = [s % ROWS for s in range(n)]
    tunes = [ROW_TUNES[s % ROWS][(s // ROWS) % 4] for s in range(n)]
    conf = sorted(SHARED_CFGS)
    ops = {0: [("map", list(range(n)), rows0), ("tune", list(range(n)), tunes), ("conf", conf, [SHARED_CFGS[s] for s in conf])],
           # 63 and 96 move to another row with one of that row's tunes, 64 is retuned on its own, all three and 11 are reset
           1: [("map", [63, 96, 9], [5, 2, 0]), ("tune", [63, 64, 96], [300000, -25000, 12345]), ("reset", [64, 11, 63, 96])],
           # 64 moves too; 96 goes back; a reset list longer than a wave
           3: [("map", [64, 96], [1, 0]), ("tune", [64, 63, 96], [150000, -500000, 200000]), ("reset", [96, 64, 63]),
               ("reset", SHARED_BIG_RESET)]}
    return rows0, ops


def planned_segments(ops, n_submits, n=SHARED_N, dflt=DFLT):
    """segments.run_segments' bookkeeping without a receiver: every stream's segments, unfed."""
    cfg, tn, row = [dflt] * n, [0] * n, list(range(n))
    book = {"map": row, "tune": tn, "conf": cfg}
    segs = [[] for _ in range(n)]
    for k in range(n_submits):
        restart = set()
        for op in ops.get(k, ()):
            if op[0] != "reset":
                for s, v in zip(op[1], op[2]):
                    book[op[0]][s] = v
            restart |= set(op[1])
        for s in range(n):
            if k == 0 or s in restart:
                segs[s].append(segments.Segment(k, cfg[s], tn[s], 0, row[s]))
    return segs


def decoding(segs):
    return [g for per in segs for g in per if any(e[7] == 1 for e in g.orc.events_full())]


def shared_segment_counts(segs):
    return [len(segs[s]) for s in (0, 9, 11, 19, 20, 63, 64, 89, 90, 96)]


SHARED_COUNTS = [1, 2, 2, 1, 2, 3, 3, 2, 1, 3]

# ---- 4. levels, capture, capture_pre and the replay
CAP_N = 97
CAP_CUT = 78  # reads row 6, triggered throughout: the longest run of the table


def cap_kind(s):
    """The row of recorder_rows.scene() stream s reads, with that row's TYPES and THRESH."""
    return s % RR.N


@functools.lru_cache(maxsize=None)
def cap_rows():
    iq = RR.scene()[[cap_kind(s) for s in range(CAP_N)]]
    iq.setflags(write=False)
    return iq


@functools.lru_cache(maxsize=None)
def cap_restated():
    """The restatement on the oracle's decimated samples (the context's front end is the oracle's, bit for bit) -> (table, pool)
    of one submit of the whole scene."""
    kinds = []
    for k in range(RR.N):
        o = O.Oracle(RR.TYPES[k], RR.THRESH[k], 0, keep_dec=True)
        o.process(RR.scene()[k])
        kinds.append(capture.captures(o.dec(), RR.TYPES[k], RR.THRESH[k])[:2])
    return capture.table([kinds[cap_kind(s)] for s in range(CAP_N)])


def cap_limits(runs, pool, short):
    """(max_runs, max_samples) that cut a table at stream CAP_CUT's run (every stream of the scene has one run at the most): by
    the run count, or by one pair less than the pool holds up to that run's end -- the pool is cut inside the run."""
    k = int(np.flatnonzero(runs["stream"] == CAP_CUT)[0])
    if short == "runs":
        return k, len(pool)
    return len(runs), int(runs["pool_offset"][k] + runs["n_samples"][k]) - 1
