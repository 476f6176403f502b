"""Channel-rate input on the GPU (tfrec_amd_create_decimated, tfrec_amd_enable_capture_pre, tfrec_amd_submit_runs, tfrec_gpu -R;
DESIGN.md 6n), bit for bit.

The five golden scenes tests/golden/iq_*.npz are five streams of four blocks.  Their decimated samples, fed to a channel-rate
context, give the oracle's events of the original bytes; their capture with the pre samples, replayed through sparse submits, gives
the events of the context that recorded it -- every field -- however the replay is cut.  The pre samples are compared with the
restatement tfrec_amd/decin.py on the recording context's own decimated samples, on the aimed scene (recorder_rows.scene)."""
import functools
import os
import subprocess

import numpy as np
import pytest

import parity
import recorder as R
from recorder import pre_of, raises, same_events
from recorder_rows import carrier, scene
from tfrec_amd import api, capture, decin, levels

pytestmark = pytest.mark.gpu

B = api.BLOCK_DEC
NB = 4
M = NB * B
NAMES = ("tfa_1", "tfa_2", "tfa_3", "tx22", "whb")
N = len(NAMES)
TYPES = 0x2F


@functools.lru_cache(maxsize=None)
def scenes():
    iq = np.stack([np.load(os.path.join(parity.ROOT, "tests", "golden", "iq_%s.npz" % n))["iq"][:NB * api.BLOCK_BYTES] for n in NAMES])
    iq.setflags(write=False)
    return iq


@functools.lru_cache(maxsize=None)
def oracles(types=TYPES, thresh=500):
    """-> (the oracles of the five scenes' bytes, their decimated samples int16 [N, M, 2])."""
    orcs = [parity.fresh_oracle(x, types, thresh, keep_dec=True) for x in scenes()]
    dec = np.stack([o.dec().reshape(-1, 2) for o in orcs])
    dec.setflags(write=False)
    return orcs, dec


def assert_oracle(ev, types=TYPES, thresh=500):
    n = 0
    for s, o in enumerate(oracles(types, thresh)[0]):
        n += parity.assert_stream(ev, s, o)
    assert n > 0
    return n


# ---- 1. dense
@functools.lru_cache(maxsize=None)
def dense(thresh, sizes=(NB,), serial=False):
    dec = oracles()[1]
    with api.Receiver(N, TYPES, thresh, 0, max_blocks=max(sizes), all_flushes=True, levels=True, decimated=True, serial_chains=serial) as r:
        assert r.input_bytes(3) == 3 * decin.BLOCK_BYTES and r.input_rate == (1, 4) and r.block_bytes == decin.BLOCK_BYTES
        fmt = api.C.c_int32(-1)
        assert r.L.tfrec_amd_get_input_format(r.h, api.C.byref(fmt)) == 0 and fmt.value == decin.FMT_DEC16
        parts, pos = [], 0
        for nb in sizes:
            parts.append(np.ascontiguousarray(dec[:, pos * B:(pos + nb) * B]))
            pos += nb
        for p in parts:
            r.submit(p)
        back = np.stack([r.decimated(s, sizes[-1] * B).reshape(-1, 2) for s in range(N)])
        lv, evs = [], []
        for _ in parts:
            lv.append(r.read_levels())
            evs.append(r.drain())
        th = [r.thresh(s) for s in range(N)]
    assert np.array_equal(back, dec[:, M - sizes[-1] * B:])
    return np.concatenate(evs), np.concatenate(lv, axis=1), th


@pytest.mark.parametrize("thresh", [500, 0])
def test_dense_decimated_samples_give_the_oracles_events_of_the_bytes(thresh):
    ev, lv, th = dense(thresh)
    assert_oracle(ev, TYPES, thresh)
    orcs, dec = oracles(TYPES, thresh)
    assert th == [o.thresh() for o in orcs]
    for s in range(N):
        want, _ = levels.levels(dec[s], TYPES, thresh)
        assert lv[s].tobytes() == want.tobytes()


@pytest.mark.parametrize("thresh", [500, 0])
def test_dense_four_blocks_equal_one_plus_three_queued(thresh):
    same_events(dense(thresh, (1, 3))[0], dense(thresh)[0])
    assert dense(thresh, (1, 3))[1].tobytes() == dense(thresh)[1].tobytes()


def test_dense_serial_chains_and_host_or_device_rows():
    same_events(dense(500, (NB,), True)[0], dense(500)[0])
    import torch

    dec = oracles()[1]
    with api.Receiver(N, TYPES, 500, 0, max_blocks=NB, all_flushes=True, decimated=True) as r:
        t = torch.from_numpy(np.ascontiguousarray(dec).reshape(N, -1).view(np.uint8).copy()).to("cuda:0")
        r.submit(t)
        same_events(r.drain(), dense(500)[0])


def test_dense_full_scale_values_read_back_clamped():
    x = parity.full_scale_row("s16", B, 5).view("<i2").reshape(1, B, 2).copy()
    x[0, :4] = [[-32768, -32768], [-32768, 32767], [5, -32768], [-32767, 0]]
    x[0, -1] = [-32768, 1]
    with api.Receiver(1, TYPES, 500, 0, max_blocks=1, all_flushes=True, decimated=True) as r:
        r.submit(x)
        got = r.decimated(0, B).reshape(-1, 2)
        r.drain()
    assert np.array_equal(got, decin.clamp(x[0])) and (x == -32768).sum() >= 5 and not (got == -32768).any()


# ---- 2. the recorder's pre samples
def test_pre_on_the_aimed_scene_one_submit_and_one_plus_three():
    got, _, ev, decs, _, _ = R.one_submit()
    with R.receiver() as r:
        r.enable_capture_pre()
        r.submit(scene())
        runs, pool, pre = r.read_captures(pre=True)
        assert np.array_equal(pre, r.read_capture_pre())  # reading pops nothing
        same_events(r.drain(), ev)
    R.assert_tables((runs, pool), got)  # the table and the pool do not notice
    assert np.array_equal(pre, pre_of(decs, runs)) and pre.dtype == np.int16 and pre.shape == (len(runs), 2)
    r1 = runs[runs["stream"] == 1][0]
    assert r1["start_sample"] % 64 == 63  # a run at bit 63 of a mask word: its pre is bit 62's sample
    assert np.array_equal(pre[runs["stream"] == 1][0], decs[1].reshape(-1, 2)[int(r1["start_sample"]) - 1])
    assert pre.any()
    # 1 + 3, queued: stream 6's second run starts at the submit's first sample and continues -- its pre is the first submit's last
    parts = parity.cut(scene(), (1, 3))
    with R.receiver(max_blocks=3) as r:
        r.enable_capture_pre()
        for p in parts:
            r.submit(p)
        first = r.read_captures(pre=True)
        r.drain()
        second = r.read_captures(pre=True)
        r.drain()
    d3 = [d.reshape(-1, 2) for d in decs]
    assert np.array_equal(first[2], pre_of([d[:B] for d in d3], first[0]))
    prev = np.stack([d[B - 1] for d in d3])
    assert np.array_equal(second[2], pre_of([d[B:] for d in d3], second[0], prev, base=B))
    k = int(np.flatnonzero(second[0]["stream"] == 6)[0])
    assert second[0][k]["start_sample"] == B and second[0][k]["flags"] & capture.RUN_CONTINUES
    assert np.array_equal(second[2][k], d3[6][B - 1]) and d3[6][B - 1].any()


def loud_ends():
    """One block of u8 silence with a carrier over its first and its last samples: a run at sample 0, a loud last sample."""
    x = np.full(api.BLOCK_BYTES, 128, dtype=np.uint8)
    carrier(x, 0, 2000)
    carrier(x, 4 * (B - 40), 4 * B)
    return x.reshape(1, -1)


def test_pre_at_a_fresh_streams_first_sample_and_after_a_reset():
    with api.Receiver(1, TYPES, 20, 0, max_blocks=1, all_flushes=True) as r:
        r.enable_capture(64, B)
        r.enable_capture_pre()
        got = []
        for k in range(3):
            if k == 2:
                r.reset_streams([0])
            r.submit(loud_ends())
            d = r.decimated(0, B).reshape(-1, 2)
            got.append(r.read_captures(pre=True) + (d,))
            r.drain()
    for k, (runs, pool, pre, d) in enumerate(got):
        assert runs[0]["start_sample"] == (k * B if k < 2 else 0)  # (it counts from the restart)
        assert bool(runs[0]["flags"] & capture.RUN_CONTINUES) == (k == 1)
    assert got[0][2][0].tolist() == [0, 0]  # a fresh stream: nothing precedes
    assert got[1][2][0].tolist() == got[0][3][-1].tolist() != [0, 0]  # the submit before's last sample
    assert got[2][2][0].tolist() == [0, 0]  # ... and not after a reset
    for runs, pool, pre, d in got:
        base = int(runs[0]["start_sample"])
        assert np.array_equal(pre[1:], pre_of([d], runs[1:], base=base)) and len(runs) >= 2


@pytest.mark.parametrize("short", ["runs", "samples"])
def test_pre_under_an_overflow_is_the_tables_prefix(short):
    (runs, pool), _, _, decs, _, _ = R.one_submit()
    cap = (len(runs) - 1, len(pool)) if short == "runs" else (len(runs), len(pool) - 1)
    with R.receiver(cap=cap) as r:
        r.enable_capture_pre()
        r.submit(scene())
        raises(api.E_OVERFLOW, r.read_capture_pre)
        got = r.read_captures(allow_overflow=True, pre=True)
        r.drain()
    assert len(got[0]) == len(runs) - 1 == len(got[2])
    assert np.array_equal(got[2], pre_of(decs, runs)[:len(runs) - 1])


def test_pre_memory_call_order_and_arguments():
    n, mb, max_runs = 3, 2, 48
    with api.Receiver(n, TYPES, 500, 0, max_blocks=mb) as r:
        raises(api.E_INVAL, r.enable_capture_pre)  # no recorder
        r.enable_capture(max_runs, 1024)
        without = r.memory()
        raises(api.E_INVAL, r.read_capture_pre)  # not enabled
        r.enable_capture_pre()
        m = r.memory()
        assert m["device_bytes"] - without["device_bytes"] == api.FIFO_DEPTH * max_runs * 4
        assert m["pinned_host_bytes"] == without["pinned_host_bytes"]
        raises(api.E_INVAL, r.enable_capture_pre)  # a second time
        raises(api.E_STATE, r.read_capture_pre)  # nothing undrained
        r.submit(scene()[:n, :api.BLOCK_BYTES])
        runs, pool, pre = r.read_captures(pre=True)
        assert len(runs) == 1 == len(pre)
        nr = api.C.c_uint32(0)
        buf = np.full(8, 0x55, dtype=np.uint8)
        assert r.L.tfrec_amd_read_capture_pre(r.h, buf.ctypes.data, 0, api.C.byref(nr)) == api.E_INVAL and nr.value == 1
        assert (buf == 0x55).all() and r.L.tfrec_amd_read_capture_pre(r.h, None, 1, api.C.byref(nr)) == api.E_INVAL
        r.drain()
    with api.Receiver(n, TYPES, 500, 0, max_blocks=mb) as r:  # a recorder without the call holds what it held
        r.enable_capture(max_runs, 1024)
        assert r.memory() == without
        r.submit(scene()[:n, :api.BLOCK_BYTES])
        raises(api.E_STATE, r.enable_capture_pre)  # after the first submit
        raises(api.E_INVAL, r.read_capture_pre)
        r.drain()


# ---- 3. the loop
def join(tabs):
    """[(runs, pool, pre)] of consecutive submits -> one table with its pool offsets into one pool."""
    runs, off = [], 0
    for t, p, _ in tabs:
        t = t.copy()
        t["pool_offset"] += off
        off += len(p)
        runs.append(t)
    return np.concatenate(runs), np.concatenate([p for _, p, _ in tabs]), np.concatenate([q for _, _, q in tabs])


@functools.lru_cache(maxsize=None)
def recorded(thresh=500, sizes=(NB,)):
    """The five scenes through a u8 context with the recorder -> ((runs, pool, pre) with start_sample from the streams' start,
    events, levels)."""
    with api.Receiver(N, TYPES, thresh, 0, max_blocks=max(sizes), all_flushes=True, levels=True) as r:
        r.enable_capture(4096, N * M)
        r.enable_capture_pre()
        tabs, lv, evs = [], [], []
        for p in parity.cut(scenes(), sizes):
            r.submit(p)
            tabs.append(r.read_captures(pre=True))
            lv.append(r.read_levels())
            evs.append(r.drain())
    return join(tabs), np.concatenate(evs), np.concatenate(lv, axis=1)


def replay(cap, sizes, types=TYPES, thresh=500, **kw):
    runs, pool, pre = cap
    with api.Receiver(N, types, thresh, 0, max_blocks=max(sizes), all_flushes=True, levels=True, decimated=True, **kw) as r:
        r.enable_runs_input(len(runs) + len(sizes) * N, len(pool) + 1)
        pos, lv, evs = 0, [], []
        for nb in sizes:
            t, p, q = decin.rebase(runs, pool, pre, pos * B, nb * B)
            assert decin.check(t, len(p), nb, N) is None
            r.submit_runs(t, p, q, nb)
            pos += nb
        for _ in sizes:
            lv.append(r.read_levels())
            evs.append(r.drain())
    return np.concatenate(evs), np.concatenate(lv, axis=1)


@pytest.mark.parametrize("thresh", [500, 0])
@pytest.mark.parametrize("rec,rep", [((NB,), (NB,)), ((NB,), (1, 3)), ((1, 3), (2, 2))], ids=["4-4", "4-1+3", "1+3-2+2"])
def test_a_replayed_capture_gives_the_recordings_events_bit_for_bit(thresh, rec, rep):
    cap, ev, lv = recorded(thresh, rec)
    assert 0 < len(cap[1]) < N * M  # a squelched capture: a part of the recording
    got, glv = replay(cap, rep, TYPES, thresh)
    same_events(got, ev)  # rssi_raw, offset, seq, end_sample and status included
    assert_oracle(got, TYPES, thresh)
    for f in ("triggered", "n_over", "thresh", "triggered_avg"):
        assert glv[f].tolist() == lv[f].tolist(), f
    assert lv["triggered"].sum() == len(cap[1])


def test_a_replay_with_fewer_types_and_a_higher_threshold_equals_the_oracle_with_those():
    cap, _, _ = recorded(500)
    for types, thresh in ((0x22, 700), (0x01, 500), (0x0C, 1500)):
        got, _ = replay(cap, (1, 3), types, thresh)
        assert_oracle(got, types, thresh)


def test_a_replay_on_a_serial_chains_context():
    cap, ev, _ = recorded(500)
    same_events(replay(cap, (NB,), serial_chains=True)[0], ev)


# ---- 4. submit_runs is the dense submit of the expanded rows
def crafted_table():
    """Two streams, two blocks: a run at sample 0 (its pre is the sample ahead of the submit), single samples one sample apart, a run
    over the block boundary, one that ends with the submit; stream 1 starts late.  Loud enough to trigger."""
    rng = np.random.default_rng(3)
    spans = [(0, 0, 300), (0, 301, 1), (0, 303, 1), (0, B - 100, 700), (0, 2 * B - 5, 5), (1, 4097, 64), (1, 4162, 1)]
    runs = np.zeros(len(spans), dtype=capture.RUN_DTYPE)
    runs["stream"], runs["start_sample"], runs["n_samples"] = zip(*spans)
    runs["pool_offset"] = np.concatenate([[0], np.cumsum(runs["n_samples"])[:-1]])
    pool = rng.integers(-3000, 3001, (int(runs["n_samples"].sum()), 2)).astype(np.int16)
    pool[5] = (-32768, 32767)
    pre = rng.integers(-3000, 3001, (len(runs), 2)).astype(np.int16)
    pre[0] = (120, -90)  # (quiet: as the last sample of the submit before it must not trigger there)
    return runs, pool, pre


def test_submit_runs_equals_the_dense_submit_of_the_expanded_rows():
    cap = recorded(500)[0]
    rows, override = decin.expand(*cap, NB, N)
    assert override == {}
    with api.Receiver(N, TYPES, 500, 0, max_blocks=NB, all_flushes=True, decimated=True) as r:
        r.submit(rows)
        want = [r.decimated(s, M) for s in range(N)]
        ev = r.drain()
    with api.Receiver(N, TYPES, 500, 0, max_blocks=NB, all_flushes=True, decimated=True) as r:
        r.enable_runs_input(len(cap[0]), len(cap[1]))
        r.submit_runs(*cap, NB)
        for s in range(N):
            assert np.array_equal(r.decimated(s, M), want[s])
        same_events(r.drain(), ev)
    same_events(ev, recorded(500)[1])
    # the crafted table, behind a submit that leaves a last sample: the run at sample 0 brings its own predecessor
    runs, pool, pre = crafted_table()
    rows, override = decin.expand(runs, pool, pre, 2, 2)
    assert override == {0: tuple(int(v) for v in pre[0])}
    lead = np.zeros((2, B, 2), dtype=np.int16)
    lead[0, -1] = pre[0]
    with api.Receiver(2, TYPES, 500, 0, max_blocks=2, all_flushes=True, decimated=True) as r:
        r.submit(lead)
        r.drain()
        r.submit(rows)
        want = [r.decimated(s, 2 * B) for s in range(2)]
        ev = r.drain()
    with api.Receiver(2, TYPES, 500, 0, max_blocks=2, all_flushes=True, decimated=True) as r:
        r.enable_runs_input(16, 4096)
        empty = np.zeros(0, dtype=capture.RUN_DTYPE)
        r.submit_runs(empty, np.zeros((0, 2), np.int16), np.zeros((0, 2), np.int16), 1)  # (carries (0, 0), not pre[0])
        assert not r.decimated(0, B).any()
        r.drain()
        r.submit_runs(runs, pool, pre, 2)
        for s in range(2):
            assert np.array_equal(r.decimated(s, 2 * B), want[s]) and np.array_equal(want[s].reshape(-1, 2), decin.clamp(rows[s]))
        got = r.drain()
    same_events(got, ev)
    assert len(ev) > 0


def test_submit_runs_refuses_every_rule_violation_and_nothing_changes():
    runs, pool, pre = crafted_table()
    with api.Receiver(2, TYPES, 500, 0, max_blocks=2, all_flushes=True, decimated=True) as r:
        raises(api.E_INVAL, r.submit_runs, runs, pool, pre, 2)  # not enabled
        r.enable_runs_input(len(runs), len(pool))
        raises(api.E_INVAL, r.enable_runs_input, 16, 16)
        mem = r.memory()

        def bad(field=None, index=None, value=None, pool=pool, nb=2, t=runs):
            t = t.copy()
            if field:
                t[field][index] = value
            assert nb > 2 or decin.check(t, len(pool), nb, 2, len(runs), len(pool)) is not None
            raises(api.E_INVAL, r.submit_runs, t, pool, np.resize(pre, (len(t), 2)), nb)

        bad("stream", 6, 2)
        bad("start_sample", 0, -1)
        bad("start_sample", 4, 2 * B)
        bad("n_samples", 4, 6)
        bad("n_samples", 1, 0)
        bad("start_sample", 2, 302)  # touches the run before it
        bad("stream", 0, 1)
        bad("pool_offset", 3, int(runs[3]["pool_offset"]) + 1)
        bad(pool=pool[:-1])
        bad(nb=1)  # the runs reach into a second block
        bad(nb=3)  # more than max_blocks
        bad(t=np.concatenate([runs, runs[-1:]]))  # more than max_runs (and out of order)
        assert r.memory() == mem
        r.submit_runs(runs, pool, pre, 2)  # the FIFO is empty and the state fresh: this is a first submit
        got = [r.decimated(s, 2 * B) for s in range(2)]
        ev = r.drain()
        assert len(r.drain()) == 0
    with api.Receiver(2, TYPES, 500, 0, max_blocks=2, all_flushes=True, decimated=True) as r:
        r.enable_runs_input(len(runs), len(pool))
        r.submit_runs(runs, pool, pre, 2)
        for s in range(2):
            assert np.array_equal(r.decimated(s, 2 * B), got[s])
        same_events(r.drain(), ev)
        r.map_streams([1], [0])
        raises(api.E_INVAL, r.submit_runs, runs[:5], pool[:int(runs[:5]["n_samples"].sum())], pre[:5], 2)  # mapped
    with api.Receiver(2, TYPES, 500, 0, max_blocks=2) as r:  # not a channel-rate context
        raises(api.E_INVAL, r.enable_runs_input, 16, 16)


# ---- 5. refusals and untouched behaviour
def test_what_a_channel_rate_context_refuses():
    with pytest.raises(api.TfrecAmdError) as e:
        api.Receiver(1, TYPES, 500, 0, max_blocks=1, decimated=True, input_10x=True)
    assert e.value.code == api.E_INVAL
    with api.Receiver(2, TYPES, 500, 0, max_blocks=1, decimated=True) as r:
        before = r.memory()
        raises(api.E_INVAL, r.tune_streams, [0], 1000)
        raises(api.E_INVAL, r.tune_streams_wide, [0], 1000)
        raises(api.E_INVAL, r.tune_streams_input, [0], 1000)
        raises(api.E_INVAL, r.enable_spectrum, 64, 16)
        assert r.memory() == before
        r.configure_streams([1], filter_type=1)  # accepted, without effect
        x = np.ascontiguousarray(oracles()[1][:2, :B])
        r.submit(x)
        raises(api.E_INVAL, r.stage0, 0, 16)
        got = [r.decimated(s, B) for s in range(2)]
        r.drain()
    assert np.array_equal(got[0].reshape(-1, 2), x[0]) and np.array_equal(got[1].reshape(-1, 2), x[1])
    cfg = api.Config(1, TYPES, 500, 0, 0, 1, 16, 0)
    h = api.C.c_void_p()
    assert api.load_library().tfrec_amd_create_format(api.C.byref(cfg), decin.FMT_DEC16, 1, 1, api.C.byref(h)) == api.E_INVAL


def test_two_mapped_streams_with_their_own_types_on_one_row():
    k = NAMES.index("tfa_2")
    dec = oracles()[1]
    with api.Receiver(2, TYPES, 500, 0, max_blocks=NB, all_flushes=True, decimated=True) as r:
        r.map_streams([1], [0])
        r.configure_streams([0, 1], types_mask=[0x02, 0x2D])
        assert r.rows_in_use == 1
        evs = []
        for p in (dec[k:k + 1, :B], dec[k:k + 1, B:]):  # 1 + 3: each stream carries its own last pair
            r.submit(np.ascontiguousarray(p))
            evs.append(r.drain())
        ev = np.concatenate(evs)
        assert np.array_equal(r.decimated(1, 3 * B).reshape(-1, 2), dec[k, B:])
    n = 0
    for s, types in ((0, 0x02), (1, 0x2D)):
        n += parity.assert_stream(ev, s, parity.fresh_oracle(scenes()[k], types, 500))
    assert n > 0 and (ev[ev["stream"] == 0]["status"] == 1).any()


def test_an_ordinary_context_is_what_it_was_with_and_without_the_pre_samples():
    k = NAMES.index("tfa_2")
    x = scenes()[k:k + 1]
    out = []
    for with_pre in (False, True):
        with api.Receiver(1, TYPES, 500, 0, max_blocks=NB, all_flushes=True, levels=True) as r:
            r.enable_capture(256, M)
            if with_pre:
                r.enable_capture_pre()
            r.submit(x)
            d = r.decimated(0, M)
            out.append((r.read_captures(), r.read_levels(), r.drain()))
    (cap, lv, ev), (cap2, lv2, ev2) = out
    parity.assert_stream(ev, 0, oracles()[0][k])
    assert np.array_equal(d.reshape(-1, 2), oracles()[1][k])
    runs, pool, _ = capture.captures(d, TYPES, 500)
    R.assert_tables(cap, capture.table([(runs, pool)]))
    assert lv[0].tobytes() == levels.levels(d, TYPES, 500)[0].tobytes()
    R.assert_tables(cap2, cap)
    assert lv2.tobytes() == lv.tobytes()
    same_events(ev2, ev)


# ---- 6. tfrec_gpu -S, then -R
def test_cli_record_then_replay_prints_the_same_telegrams(tmp_path):
    cli = parity.build_cli()
    k = NAMES.index("tfa_2")
    x = scenes()[k]
    f = tmp_path / "tfa2.iq"
    x.tofile(f)
    dec = oracles()[1][k]

    def run(args):
        out = subprocess.run([cli] + args, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr
        return parity.telegram_lines(out.stdout)

    base = ["-T", "2f", "-t", "500"]
    plain = run(base + ["-L", str(f)])
    assert len(plain) >= 1
    for name, rec, rep in (("cut", ["-b", "3"], ["-b", "2"]), ("slot", ["-n", "1"], ["-n", "1", "-b", "1"])):
        pre = str(tmp_path / name)
        assert run(base + rec + ["-S", pre, "-L", str(f)]) == plain
        assert run(base + rep + ["-R", pre]) == plain, name
        # the capture against the restatement, submit by submit: .idx and .cs16 are what they were, .pre is decin.pre_samples
        nb = int(rec[rec.index("-b") + 1]) if "-b" in rec else 16
        lines, pools, pres, st, prev = [], [], [], None, None
        for a in range(0, NB, nb):
            part = dec[a * B:min(a + nb, NB) * B]
            runs, pool, st = capture.captures(part, TYPES, 500, st)
            lines += [capture.idx_line(0, r) for r in runs]
            pools.append(pool)
            pres.append(decin.pre_samples(part[None], runs, prev, base=a * B))
            prev = part[None, -1]
        assert open(pre + ".idx").read().splitlines() == lines and len(lines) >= 1
        assert np.array_equal(np.fromfile(pre + ".0.cs16", dtype="<i2").reshape(-1, 2), np.concatenate(pools))
        assert np.array_equal(np.fromfile(pre + ".0.pre", dtype="<i2").reshape(-1, 2), np.concatenate(pres))
    # a stricter replay: another -T, a higher -t -- the telegrams of the recording decoded with those
    pre = str(tmp_path / "cut")
    assert run(["-T", "02", "-t", "900", "-R", pre]) == run(["-T", "02", "-t", "900", "-L", str(f)])
