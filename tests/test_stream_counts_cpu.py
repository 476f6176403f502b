"""The inputs of tests/test_stream_counts_gpu.py -- 65 and 97 streams: a full wave or workgroup of streams and a partial one behind
it -- and, without a GPU, every condition those tests assume about them, from the oracle and the numpy restatements.  A GPU test
there cannot pass on an empty comparison: that the events, runs and telegrams it compares exist, on the streams of the partial
groups too, is asserted here.

97 = 3 * 32 + 1 = 64 + 33: whb_chain_kernel's fourth workgroup holds one stream, the second step of 64 holds 33.
65 = 2 * 32 + 1 = 64 + 1:  the second step of 64 holds one stream.

Everything is an exact integer; nothing here has a tolerance."""
import functools

import numpy as np

import parity
import recorder_rows as RR
import segments
from oracle import oracle as O
from test_channels_gpu import CFGS, DFLT, ROW_TUNES, ROWS, make_rows
from tfrec_amd import api, capture, synth

B = api.BLOCK_DEC
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


def test_the_chain_rows_flush_in_every_slot_and_the_last_streams_row_decodes():
    orc = chain_oracle()
    assert sorted(set(np.concatenate([e["slot"] for e in orc]).tolist())) == [0, 1, 2, 3, 4]
    for n in COUNTS:
        last = per_stream(orc, n)[n - 1]  # (row 0: the last stream is the lone one of its group)
        assert (last["status"] == 1).any() and rows_of(n, CHAIN_UNIQUE)[n - 1] == 0
        # default mode: the comparison of the reported flushes is not one of empty lists either
        assert parity.reported_mask(last).any()
        every = per_stream(orc, n)
        assert sum(len(e) for e in every) > 5 * n and sum(int(parity.reported_mask(e).sum()) for e in every) > n


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


def test_every_row_behind_stream_64_has_a_whb_flush():
    """2(a): R97 - R64 counts the failures among rows 0..32; a row without a WHB window could not fail."""
    for e in whb_oracle()[:33]:
        assert (e["slot"] == 4).any()
    # 2(b), (c): a redo of a stream behind index 64 has WHB telegrams to get right on most of their rows, with all five protocols
    # and with WHB alone
    assert sum(CARRY_SIZES) == sum(REDO_SIZES) and max(CARRY_SIZES) <= 3
    for types in (0x2F, 0x20):
        assert sum(bool(((e["slot"] == 4) & (e["status"] == 1)).any()) for e in redo_oracle(types)[:33]) > 33 // 2
        for n in (64, 65, 97):
            assert sum(len(e) for e in per_stream(redo_oracle(types), n)) > (5 * n if types == 0x2F else n // 2)
    for n in (64, 97):
        assert sum(len(e) for e in per_stream(whb_oracle(), n)) > n


def test_a_whb_telegram_of_the_lone_streams_row_is_carried_into_a_redo():
    """2(c): stream 64 of 65 reads row 0.  One of its WHB telegrams begins in a submit that the hook lets pass and has the boundary
    to the next submit, which the hook fails, inside its bytes: the window is locked and open there, the passed submit carries
    its frozen average over the boundary and the redo continues it.  (TFREC_AMD_WHB_FORCE_FAIL=2 fails stream s in submit k iff
    s + k is even: whb_check_kernel.)"""
    ev = redo_oracle(0x20)[0]
    tel = ev[(ev["slot"] == 4) & (ev["status"] == 1)]
    bounds = np.concatenate([[0], np.cumsum(CARRY_SIZES)]) * B
    found = 0
    for e in tel:
        # a byte is 8 bits of 64 decimated samples; the flush comes behind the last byte
        first, last = int(e["end_sample"]) - 512 * int(e["byte_cnt"]), int(e["end_sample"]) - 512
        k = int(np.searchsorted(bounds, first, side="right")) - 1  # the submit the bytes begin in
        found += (64 + k) % 2 == 1 and first < bounds[k + 1] < last
    assert found >= 1


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


def test_the_shared_rows_plan_names_the_streams_around_64_and_half_its_segments_decode():
    rows0, ops = shared_plan()
    assert set(rows0[62:66]) == {2, 3, 4, 5} and {31, 32, 63, 64, 65, 96} <= set(SHARED_CFGS)
    auto = [s for s, c in SHARED_CFGS.items() if c[1] == 0]
    assert min(auto) < 64 < max(auto)
    for k in (1, 3):
        for kind in ("map", "tune", "reset"):
            named = set().union(*[set(op[1]) for op in ops[k] if op[0] == kind])
            assert named & {63, 64, 96}, (k, kind)
        assert {63, 64, 96} <= set().union(*[set(op[1]) for op in ops[k]])
    assert max(len(op[1]) for k in ops for op in ops[k] if op[0] == "reset") >= 65
    iq = make_rows(SHARED_SEED, sum(SHARED_SIZES))
    hosts = parity.cut(iq, SHARED_SIZES)
    segs = planned_segments(ops, len(SHARED_SIZES))
    for k in range(len(hosts)):
        for per in segs:
            g = [g for g in per if g.k <= k][-1]
            g.feed(hosts[k][g.row])
    assert shared_segment_counts(segs) == SHARED_COUNTS
    ok = decoding(segs)
    assert len(ok) >= SHARED_N // 2
    assert any(g.k > 0 for g in ok)  # a segment behind a restart decodes too


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


def test_the_capture_scene_has_runs_on_both_sides_of_stream_64_and_none_on_it():
    runs, pool = cap_restated()
    per = np.bincount(runs["stream"], minlength=CAP_N)
    assert per[64] == 0 and per[63] > 0 and cap_kind(64) == 0  # a step of the prefix scan begins with an empty entry
    assert per[:64].any() and per[65:].any()
    for k in range(RR.N):  # every row kind lands on both sides
        assert any(cap_kind(s) == k for s in range(64)) and any(cap_kind(s) == k for s in range(65, CAP_N))
    assert per[6::8].min() > 0 and (per[0::8] == 0).all() and (per[1:6] == 1).all()
    assert int(runs["pool_offset"][-1] + runs["n_samples"][-1]) == len(pool) > 2 ** 16
    for short in ("runs", "samples"):
        cap = cap_limits(runs, pool, short)
        wr, wp, ov = capture.prefix(runs, pool, *cap)
        # the cut falls behind stream 64: whole runs of streams 65 .. 77 are kept, the first one dropped is stream 78's
        assert ov and wr[-1]["stream"] == CAP_CUT - 1 and runs[len(wr)]["stream"] == CAP_CUT
        assert (wr["stream"] > 64).sum() >= 1 and len(wp) == int(runs["pool_offset"][len(wr)]) < len(pool)
