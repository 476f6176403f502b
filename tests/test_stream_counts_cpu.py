"""Without a GPU, every condition the tests of tests/test_stream_counts_gpu.py -- 65 and 97 streams: a full wave or workgroup of
streams and a partial one behind it -- assume about their inputs (tests/stream_count_rows.py), from the oracle and the numpy
restatements.  A GPU test there cannot pass on an empty comparison: that the events, runs and telegrams it compares exist, on the
streams of the partial groups too, is asserted here.

Everything is an exact integer; nothing here has a tolerance."""
import numpy as np

import parity
import recorder_rows as RR
from input_rows import make_rows
from stream_count_rows import (CAP_CUT, CAP_N, CARRY_SIZES, CHAIN_UNIQUE, COUNTS, REDO_SIZES, SHARED_CFGS, SHARED_COUNTS, SHARED_N,
                               SHARED_SEED, SHARED_SIZES, cap_kind, cap_limits, cap_restated, chain_oracle, decoding, per_stream,
                               planned_segments, redo_oracle, rows_of, shared_plan, shared_segment_counts, whb_oracle)
from tfrec_amd import api, capture

B = api.BLOCK_DEC


# ---- 1. the main chain
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
