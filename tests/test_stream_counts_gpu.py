"""The per-stream kernels at stream counts that straddle a wave: 65 and 97 streams, a full wave or workgroup of streams with a partial
one behind it, against the oracle and the numpy restatements, bit for bit.

Several kernels step over the streams in groups of 32 or 64: whb_chain_kernel (32 streams per workgroup, one per lane of the consumer
wave), the redo launch of whb_demod_kernel (a ballot over 64 streams at a time), commit_kernel (64 streams per workgroup),
capture_offsets_kernel (a prefix scan that carries its totals from one step of 64 streams to the next) and every per-stream table
indexed through a stream list.  97 = 3 * 32 + 1 = 64 + 33 and 65 = 2 * 32 + 1 = 64 + 1 put a second group and a ragged tail behind
the first.

The inputs are in tests/stream_count_rows.py; every condition assumed about them here -- that the compared events, runs and telegrams
exist, on the streams behind index 64 too -- is asserted in tests/test_stream_counts_cpu.py."""
import functools

import numpy as np
import pytest

import parity
import recorder as R
import recorder_rows as RR
import segments
import stream_count_rows as C
from input_rows import DFLT, make_rows
from parity import device_parts
from recorder import pre_of, same_events
from tfrec_amd import api, capture, decin, levels

pytestmark = pytest.mark.gpu

B = api.BLOCK_DEC


# ---- 1. the main chain
def assert_replicas(ev, n, unique):
    """Stream s and its copies s + k * unique have the same events, the stream index apart."""
    ev = parity.sort_events(ev)
    first = ev[ev["stream"] < unique]
    for k in range(1, -(-n // unique)):
        rep = ev[(ev["stream"] >= k * unique) & (ev["stream"] < (k + 1) * unique)].copy()
        rep["stream"] -= k * unique
        want = first[first["stream"] < n - k * unique]
        assert len(rep) == len(want) > 0 and rep.tobytes() == want.tobytes(), "copies %d" % k


@pytest.mark.parametrize("serial", [False, True], ids=["pipeline", "serial"])
@pytest.mark.parametrize("n", C.COUNTS)
def test_main_chain_every_stream_equals_the_oracle(n, serial):
    iq = C.chain_rows()[C.rows_of(n, C.CHAIN_UNIQUE)]
    with api.Receiver(n, 0x2F, 500, 0, max_blocks=max(C.CHAIN_SIZES), all_flushes=True, serial_chains=serial) as r:
        ev = np.concatenate(parity.run_fifo(r, parity.cut(iq, C.CHAIN_SIZES)))
        assert r.fm_stats()["host_mismatch"] == 0
    assert parity.assert_all_streams(ev, None, 0x2F, 500, orc=C.per_stream(C.chain_oracle(), n)) > 5 * n
    assert_replicas(ev, n, C.CHAIN_UNIQUE)


def test_main_chain_in_default_mode_with_one_submit_in_flight():
    n = 97
    iq = C.chain_rows()[C.rows_of(n, C.CHAIN_UNIQUE)]
    with api.Receiver(n, 0x2F, 500, 0, max_blocks=max(C.CHAIN_SIZES)) as r:
        ev = np.concatenate(parity.run_fifo(r, parity.cut(iq, C.CHAIN_SIZES), depth=1))
        assert r.fm_stats()["host_mismatch"] == 0
    assert parity.assert_all_streams(ev, None, 0x2F, 500, all_flushes=False, orc=C.per_stream(C.chain_oracle(), n)) > n
    assert_replicas(ev, n, C.CHAIN_UNIQUE)


# ---- 2. the WHB check
def whb_respeculated(n):
    """One submit of the 24 blocks, WHB alone, product library -> the streams the check sent to the exact kernel."""
    iq = C.whb_rows()[C.rows_of(n, C.WHB_UNIQUE)]
    with api.Receiver(n, 0x20, 500, 0, max_blocks=C.WHB_BLOCKS, all_flushes=True) as r:
        r.submit(iq)
        ev = r.drain()
        assert parity.assert_all_streams(ev, None, 0x20, 500, orc=C.per_stream(C.whb_oracle(), n)) > n
        return r.stats()["whb_respeculated"]


def test_whb_check_accepts_the_streams_of_a_partial_workgroup():
    """Parity cannot see a check that is too strict: the stream is redone by the exact kernel and the events stay right.  With one
    submit the count of redone streams is a per-stream function of the input; rows 64..96 are rows 0..32 again, so the 97-stream
    count is the 64-stream count plus the failures among rows 0..32: between once and twice that count.  Measured: R64 = 0,
    R97 = 0."""
    r64 = whb_respeculated(64)
    r97 = whb_respeculated(97)
    print("whb_respeculated: R64 = %d, R97 = %d" % (r64, r97))
    assert r64 <= 1
    assert r64 <= r97 <= 2 * r64


@pytest.mark.parametrize("deep", ["1", "0"])
@pytest.mark.parametrize("every", [2, 3])
def test_whb_forced_failures_are_redone_behind_stream_64(every, deep, monkeypatch):
    """TFREC_AMD_WHB_FORCE_FAIL fails every N-th (stream + submit): the redo launch looks through the flags 64 streams at a time.
    The events of all 97 streams are the oracle's, and more streams were redone than on the first 64 rows alone."""
    monkeypatch.setenv("TFREC_AMD_WHB_FORCE_FAIL", str(every))
    monkeypatch.setenv("TFREC_AMD_DEEP", deep)
    for types in (0x2F, 0x20):
        redone = {}
        for n in (97, 64):
            iq = C.redo_rows()[C.rows_of(n, C.WHB_UNIQUE)]
            with api.Receiver(n, types, 500, 0, max_blocks=max(C.REDO_SIZES), all_flushes=True, experiments=True) as r:
                assert r.layout() == (6 if deep == "1" else 4)
                ev = np.concatenate(parity.run_fifo(r, parity.cut(iq, C.REDO_SIZES)))
                assert not (ev["status"] == 0xFF).any()
                total = parity.assert_all_streams(ev, None, types, 500, orc=C.per_stream(C.redo_oracle(types), n))
                assert total > (5 * n if types == 0x2F else n // 2)
                redone[n] = r.stats()["whb_respeculated"]
            print("types %02x every %d deep %s: %d streams, %d redone" % (types, every, deep, n, redone[n]))
            assert redone[n] >= n * len(C.REDO_SIZES) // every // 2, redone
        assert redone[97] > redone[64], redone


def test_whb_perturbed_average_of_the_lone_stream_is_carried_into_a_redo(monkeypatch):
    """test_whb_frozen_average_off_by_some_is_carried_into_a_redo at 65 streams: the last workgroup of whb_chain_kernel and the
    second step of the redo's ballot hold stream 64 alone, and a telegram of its row is locked and open where a passed submit
    meets a failed one."""
    monkeypatch.setenv("TFREC_AMD_WHB_TEST_PERTURB", "3000")
    monkeypatch.setenv("TFREC_AMD_WHB_FORCE_FAIL", "2")
    n = 65
    iq = C.redo_rows()[C.rows_of(n, C.WHB_UNIQUE)]
    parts = parity.cut(iq, C.CARRY_SIZES)
    with api.Receiver(n, 0x20, 500, 0, max_blocks=max(C.CARRY_SIZES), all_flushes=True, experiments=True) as r:
        ev = np.concatenate(parity.run_fifo(r, parts))
        assert not (ev["status"] == 0xFF).any()
        assert parity.assert_all_streams(ev, None, 0x20, 500, orc=C.per_stream(C.redo_oracle(0x20), n)) > n // 2
        assert r.stats()["whb_respeculated"] >= n * len(parts) // 4
    assert (ev[ev["stream"] == 64]["status"] == 1).any()


# ---- 3. shared rows and per-stream operations
@pytest.mark.parametrize("mode", ["deep", "serial_chains"])
def test_shared_rows_and_stream_lists_across_index_64(mode, monkeypatch):
    """test_shared_rows' scheme with 97 receivers on its 6 rows: per-stream settings, remaps, retunes and resets that name streams
    63, 64 and 96, and one reset list longer than a wave."""
    kw, layout, _ = parity.mode_kwargs(mode, monkeypatch)
    n, sizes = C.SHARED_N, C.SHARED_SIZES
    _, ops = C.shared_plan()
    iq = make_rows(C.SHARED_SEED, sum(sizes))
    with api.Receiver(n, DFLT[0], DFLT[1], DFLT[2], max_blocks=max(sizes), **kw) as r:
        assert r.layout() == layout
        parts, hosts = device_parts(iq, sizes)
        total, segs = segments.run_segments(r, parts, ops, DFLT, hosts=hosts)
        assert [r.stream_input(s) for s in (9, 63, 64, 96)] == [0, 5, 1, 0]
    assert C.shared_segment_counts(segs) == C.SHARED_COUNTS
    assert total > 5 * n
    assert len(C.decoding(segs)) >= n // 2  # the planted bursts decode: the comparison is not one of empty lists


# ---- 4. levels, capture, capture_pre and the replay
N4 = C.CAP_N
NB, M = RR.NB, RR.M


def recorder(max_blocks=NB, cap=(4096, N4 * M)):
    r = R.receiver(max_blocks=max_blocks, cap=cap, n=N4, levels=True)
    r.enable_capture_pre()
    return r


def want_levels(decs, states):
    out = []
    for s, d in enumerate(decs):
        k = C.cap_kind(s)
        rec, states[s] = levels.levels(d, RR.TYPES[k], RR.THRESH[k], states[s])
        out.append(rec)
    return np.stack(out)


@functools.lru_cache(maxsize=None)
def kind_oracles():
    return [parity.fresh_oracle(RR.scene()[k], RR.TYPES[k], RR.THRESH[k]) for k in range(RR.N)]


def assert_oracle(ev):
    total = sum(parity.assert_stream(ev, s, kind_oracles()[C.cap_kind(s)]) for s in range(N4))
    assert total > N4 // 2
    return total


@functools.lru_cache(maxsize=None)
def one_submit():
    """-> ((table, pool, pre), levels, events, every stream's decimated samples)."""
    with recorder() as r:
        r.submit(C.cap_rows())
        decs = [r.decimated(s, M) for s in range(N4)]
        got = r.read_captures(pre=True)
        assert r.capture_totals == (len(got[0]), len(got[1])) and not r.capture_overflow
        lv = r.read_levels()
        ev = r.drain()
    return got, lv, ev, decs


def test_table_pool_pre_samples_and_levels_of_97_streams_equal_the_restatements():
    (runs, pool, pre), lv, ev, decs = one_submit()
    want = RR.want_tables(decs, [None] * N4)
    R.assert_tables((runs, pool), want)
    R.assert_tables((runs, pool), C.cap_restated(), "the oracle's front end")
    assert np.array_equal(pre, pre_of(decs, runs)) and pre.shape == (len(runs), 2) and pre.any()
    assert lv.tobytes() == want_levels(decs, [None] * N4).tobytes()
    assert_oracle(ev)
    # what the scene is repeated for: a step of the scan over the streams begins with an empty entry behind one with runs, and
    # both steps hold runs
    per = np.bincount(runs["stream"], minlength=N4)
    assert per[63] > 0 and per[64] == 0 and per[:64].any() and per[65:].any()


def test_one_plus_three_queued_before_the_first_read():
    _, lv1, ev1, decs = one_submit()
    sizes = (1, 3)
    parts = parity.cut(C.cap_rows(), sizes)
    with recorder(max_blocks=max(sizes)) as r:
        for p in parts:
            r.submit(p)
        last = [r.decimated(s, sizes[-1] * B) for s in range(N4)]
        got, lv, evs = [], [], []
        for _ in parts:
            got.append(r.read_captures(pre=True))
            lv.append(r.read_levels())
            evs.append(r.drain())
    for s in range(N4):  # the front end does not depend on the cut: the restatements may run on the uncut context's samples
        assert np.array_equal(last[s], decs[s][2 * B:])
    cstates, lstates, pos, prev = [None] * N4, [None] * N4, 0, None
    for k, nb in enumerate(sizes):
        part = [d[2 * pos * B:2 * (pos + nb) * B] for d in decs]
        R.assert_tables(got[k][:2], RR.want_tables(part, cstates), "submit %d" % k)
        assert np.array_equal(got[k][2], pre_of(part, got[k][0], prev, base=pos * B)), "submit %d pre" % k
        assert lv[k].tobytes() == want_levels(part, lstates).tobytes(), "submit %d levels" % k
        prev = np.stack([d.reshape(-1, 2)[-1] for d in part])
        pos += nb
    cont = got[1][0][got[1][0]["flags"] & capture.RUN_CONTINUES != 0]["stream"]
    assert (cont > 64).any() and (cont < 64).any()  # carried triggers on both sides
    assert np.concatenate(lv, axis=1).tobytes() == lv1.tobytes()
    same_events(np.concatenate(evs), ev1)
    assert_oracle(np.concatenate(evs))


@pytest.mark.parametrize("short", ["runs", "samples"])
def test_overflow_behind_stream_64_delivers_a_prefix_and_the_next_submit_is_exact(short):
    (runs, pool, _), _, ev1, _ = one_submit()
    cap = C.cap_limits(*C.cap_restated(), short)
    states = [None] * N4
    with recorder(cap=cap) as r:
        r.submit(C.cap_rows())
        want = RR.want_tables([r.decimated(s, M) for s in range(N4)], states)
        with pytest.raises(api.TfrecAmdError) as e:
            r.read_captures()
        assert e.value.code == api.E_OVERFLOW
        got = r.read_captures(allow_overflow=True, pre=True)
        assert r.capture_overflow and r.capture_totals == (len(want[0]), len(want[1])) == (len(runs), len(pool))
        wr, wp, ov = capture.prefix(want[0], want[1], *cap)
        assert ov and wr[-1]["stream"] == C.CAP_CUT - 1 and (wr["stream"] > 64).any()
        R.assert_tables(got[:2], (wr, wp), "the prefix")
        assert np.array_equal(got[2], one_submit()[0][2][:len(wr)])
        ev = r.drain()
        # the next submit -- one block, so that it fits -- captures normally, its CONTINUES flags included
        r.submit(C.cap_rows()[:, :api.BLOCK_BYTES])
        want2 = RR.want_tables([r.decimated(s, B) for s in range(N4)], states)
        got2 = r.read_captures()
        assert not r.capture_overflow
        r.drain()
    R.assert_tables(got2, want2, "the submit behind the overflow")
    assert (got2[0][got2[0]["flags"] & capture.RUN_CONTINUES != 0]["stream"] > 64).any()
    same_events(ev, ev1)  # the events do not notice


def test_a_replayed_capture_of_97_streams_gives_the_recordings_events_bit_for_bit():
    (runs, pool, pre), lv, ev, _ = one_submit()
    sizes = (2, 2)
    with R.receiver(max_blocks=max(sizes), cap=None, n=N4, levels=True, decimated=True) as r:
        r.enable_runs_input(len(runs) + len(sizes) * N4, len(pool) + 1)
        pos, glv, evs = 0, [], []
        for nb in sizes:
            t, p, q = decin.rebase(runs, pool, pre, pos * B, nb * B)
            assert decin.check(t, len(p), nb, N4) is None
            assert (t["stream"] > 64).any() and (t["stream"] < 64).any()
            r.submit_runs(t, p, q, nb)
            pos += nb
        for _ in sizes:
            glv.append(r.read_levels())
            evs.append(r.drain())
    same_events(np.concatenate(evs), ev)  # rssi_raw, offset, seq, end_sample and status included
    assert_oracle(np.concatenate(evs))
    glv = np.concatenate(glv, axis=1)
    for f in ("triggered", "n_over", "thresh", "triggered_avg"):
        assert glv[f].tolist() == lv[f].tolist(), f
    assert lv["triggered"].sum() == len(pool)
