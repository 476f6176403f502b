"""The IQ balancer on the GPU (tfrec_amd_create_iq, tfrec_amd_read_iq, tfrec_amd_reset_iq_rows, tfrec_gpu -Z), bit for
bit.

(t, g), d and stage 0 are pinned by the restatement (formats.to_x -> iqbal.iq_balance -> tune.mix_in_s16 / resample.resample_x16),
everything behind stage 0 by the oracle's process_s16 fed that chain's output.  The scenes are synthetic recordings of 4 units
(a unit: one block, three at 4/3) with one burst per row, a DC offset of a few u8 LSB and an IQ imbalance on each row; the ghost
scene is meter_rows.py's."""
import functools
import subprocess

import numpy as np
import pytest

import parity
from input_rows import stage0_of_x
from meter_rows import (GHOST_BLOCKS, GHOST_FREQS, GHOST_K, GHOST_RATE, IDENT, ghost_oracles, ghost_scene, guard_rows, impair,
                        receiver_oracle)
from oracle import oracle as O
from tfrec_amd import api, dcblock, formats, iqbal, resample, synth, tune

pytestmark = pytest.mark.gpu

TYPES, THRESH = 0x2F, 500
DCS = ((8, -4), (-5, 11))  # per row, in u8 LSB
IMPAIRMENTS = ((1.12, 8.0), (0.93, -5.0))  # per row: gain, degrees
SIZES = (1, 2, 1)  # the submits, in units


@functools.lru_cache(maxsize=None)
def scene(fmt, p, q, n_blocks, offset=True, n_rows=2):
    """[rows, bytes] (read-only): row r is a recording at 1536000 p / q in the format with a burst of protocol r in its middle, the
    imbalance IMPAIRMENTS[r] and -- offset -- the DC offset DCS[r] (which, left in, keeps every trigger window open: the rows of a
    context without the blocker have none)."""
    n = n_blocks * 32768 * p
    rows = []
    for r in range(n_rows):
        bursts = [dict(proto=r, start=(n // 2) // q * q, payload_seed=31 + 7 * r, f0_hz=0, amp=50)]
        u = np.ascontiguousarray(synth.gen_scene(70 + r, n_blocks, bursts, dc_iq=DCS[r] if offset else (0, 0), rate_mult=p).reshape(-1, 2)[::q]).reshape(-1)
        x = impair(tune.s16_of_u8(u), *IMPAIRMENTS[r]).astype(np.int32)
        if fmt in ("u8", "s8"):
            x = np.clip((x + 32) & ~63, -8192, 8128)
        else:
            x = np.clip(x + np.random.default_rng(9 + r).integers(-32, 32, x.shape), -8192, 8191)
        rows.append(formats.encode(fmt, x.astype(np.int16)))
    rows = np.ascontiguousarray(np.stack(rows))
    rows.setflags(write=False)
    return rows


def balanced(rows, fmt, k_dc, k_iq, sizes, p=1, q=1, reset_before=None):
    """Per row the restatement over the submits: (x'' of the whole row, [d of submit i], [tg of submit i]).  reset_before: {submit:
    rows whose balancer state is cleared ahead of it}."""
    out = []
    bps = formats.bytes_per_sample(fmt)
    for r, row in enumerate(rows):
        pos, st, xs, ds, tgs = 0, None, [], [], []
        for i, nb in enumerate(sizes):
            n = dcblock.input_samples(nb, p, q) * bps
            if reset_before and r in reset_before.get(i, ()):
                st = (st[0], None)
            x, d, tg, st = iqbal.iq_balance(row[pos:pos + n], fmt, k_dc, k_iq, st)
            xs.append(x)
            ds.append(d)
            tgs.append(tg)
            pos += n
        assert pos == len(row)
        out.append((np.concatenate(xs), ds, tgs))
    return out


def oracle_of(y0, **kw):
    o = O.Oracle(TYPES, THRESH, 0, **kw)
    o.process_s16(y0)
    return o


def run_iq(rows, sizes, p, q, fmt, k_dc, k_iq, *, n_streams=None, dc_rows=None, host=False, before=None, stage0=True, decimated=False, **kw):
    """A balancer receiver over the rows cut into `sizes` blocks, one submit in flight -> (events per submit, stage 0 per submit and
    stream, d per submit and row (None without the blocker), tg per submit and row, decimated samples per submit and stream)."""
    parts = parity.cut_input(rows, sizes, fmt, p, q)
    n = len(rows) if n_streams is None else n_streams
    kw.setdefault("all_flushes", True)
    evs, y0, ds, tgs, dec = [], [], [], [], []
    with api.Receiver(n, TYPES, THRESH, 0, max_blocks=max(sizes), input_format=fmt, input_rate=(p, q), dc_windows=k_dc or None, iq_windows=k_iq,
                      dc_rows=dc_rows, **kw) as r:
        want_rows = n if dc_rows is None else dc_rows
        assert r.input_rate == (p, q) and r.input_format == fmt and r.iq() == (k_iq, want_rows)
        assert r.dc() == ((k_dc, want_rows) if k_dc else (0, 0))
        for i, part in enumerate(parts if host else parity.to_device(parts)):
            assert r.input_bytes(sizes[i]) == part.shape[1]
            if before:
                before(r, i)
            r.submit(part)
            if stage0:
                y0.append([r.stage0(s, sizes[i] * 4 * api.BLOCK_DEC) for s in range(n)])
            if decimated:
                dec.append([r.decimated(s, sizes[i] * api.BLOCK_DEC) for s in range(n)])
            tgs.append([r.read_iq(row) for row in range(r.rows_in_use)])
            if k_dc:
                ds.append([r.read_dc(row) for row in range(r.rows_in_use)])
            else:
                with pytest.raises(api.TfrecAmdError) as e:  # a context without the blocker
                    r.read_dc(0)
                assert e.value.code == api.E_INVAL
                ds.append(None)
            evs.append(r.drain())
    return evs, y0, ds, tgs, dec


def assert_estimates(ds, tgs, want, sizes):
    for s, (_, d, tg) in enumerate(want):
        for i in range(len(sizes)):
            assert tgs[i][s].dtype == np.int16 and tgs[i][s].shape == tg[i].shape and np.array_equal(tgs[i][s], tg[i]), ("tg", s, i)
            if ds[i] is not None:
                assert np.array_equal(ds[i][s], d[i]), ("d", s, i)


# ---- (t, g), d, stage 0, the decimated samples and the events equal the chain of restatements
# fmt, p, q, unit, k_dc, k_iq.  1/1: 64 windows per block; 25/16: 100, so the last piece of a scan is partial; 4/3: units of 3 blocks,
# 256 windows.  K = 3: the ring wraps inside every submit; 64 and 100: across submits (and inside the two-unit one); 4096: never.
CONTEXTS = [("u8", 1, 1, 1, 0, 3), ("u8", 1, 1, 1, 4, 64), ("u8", 1, 1, 1, 4, 4096), ("s8", 1, 1, 1, 4, 100), ("s8", 1, 1, 1, 0, 64),
            ("s16", 25, 16, 1, 4, 3), ("s16", 25, 16, 1, 0, 100), ("s16", 25, 16, 1, 4, 64), ("f32", 4, 3, 3, 0, 4096), ("f32", 4, 3, 3, 4, 100),
            # the blocker's ring inside the balancer's estimate kernel: it fills exactly at a submit boundary (64), inside the second
            # submit (100), never (4096)
            ("u8", 1, 1, 1, 64, 3), ("s8", 1, 1, 1, 100, 64), ("s16", 25, 16, 1, 100, 64), ("f32", 4, 3, 3, 4096, 100)]


@pytest.mark.parametrize("fmt,p,q,unit,k_dc,k_iq", CONTEXTS, ids=["%s-%d/%d-dc%d-K%d" % (c[0], c[1], c[2], c[4], c[5]) for c in CONTEXTS])
def test_the_chain_equals_the_restatements(fmt, p, q, unit, k_dc, k_iq):
    sizes = tuple(unit * u for u in SIZES)
    rows = scene(fmt, p, q, sum(sizes), k_dc > 0)
    want = balanced(rows, fmt, k_dc, k_iq, sizes, p, q)
    evs, y0, ds, tgs, dec = run_iq(rows, sizes, p, q, fmt, k_dc, k_iq, decimated=True)
    assert_estimates(ds, tgs, want, sizes)
    ev = np.concatenate(evs)
    moved = 0
    for s in range(len(rows)):
        w0 = stage0_of_x(want[s][0], p, q)
        parity.assert_stage0(y0, sizes, w0, s, fmt)
        orc = oracle_of(w0, keep_dec=True)
        assert np.array_equal(np.concatenate([dd[s] for dd in dec]), orc.dec()), s
        assert parity.assert_segment(ev, s, orc, "stream %d" % s) > 0
        moved += int((np.concatenate(want[s][2]) != IDENT).any(axis=1).sum())
    assert moved > 100  # (estimates that correct something)


@pytest.mark.parametrize("mode", ["shallow", "serial_chains", "default_mode", "bits", "host"])
def test_every_mode_works(mode, monkeypatch):
    kw, layout, flags = parity.mode_kwargs(mode, monkeypatch)
    fmt, p, q, k_dc, k_iq, sizes = "u8", 1, 1, 4, 64, (1, 2, 1)
    rows = scene(fmt, p, q, 4)
    want = balanced(rows, fmt, k_dc, k_iq, sizes)
    layouts = []
    evs, _, ds, tgs, _ = run_iq(rows, sizes, p, q, fmt, k_dc, k_iq, host=flags["host"], stage0=False, timing=True,
                                before=lambda r, i: layouts.append(r.layout()), **kw)
    assert layouts[0] == layout
    assert_estimates(ds, tgs, want, sizes)
    ev = np.concatenate(evs)
    for s in range(len(rows)):
        orc = oracle_of(want[s][0], log_bits=flags["bits"])
        assert parity.assert_stream(ev, s, orc, default_mode=flags["default_mode"]) > 0
        if flags["bits"]:
            assert parity.assert_bits(ev, s, orc, "stream %d" % s) > 100


# ---- the guards
def test_guard_rows_pass_through_unchanged():
    """One submit of five S16 rows at 1/1: silence, Q = I, Q = I / 2 + noise, Q = 2 Q0 -- each refused by its guard -- and a row that
    is corrected."""
    named = guard_rows(64)
    names = list(named)
    rows = np.stack([formats.encode("s16", named[k]) for k in names])
    want = balanced(rows, "s16", 0, 64, (1,))
    evs, y0, ds, tgs, _ = run_iq(rows, (1,), 1, 1, "s16", 0, 64)
    assert_estimates(ds, tgs, want, (1,))
    for s, name in enumerate(names):
        parity.assert_stage0(y0, (1,), want[s][0], s, name)
        if name == "fine":
            assert (tgs[0][s] != IDENT).any(axis=1).all() and not np.array_equal(y0[0][s], named[name])
        else:
            assert (tgs[0][s] == IDENT).all() and np.array_equal(y0[0][s], named[name]), name
        parity.assert_segment(evs[0], s, oracle_of(want[s][0]), name)


# ---- the ghost scene
def test_no_mirror_receiver_decodes_behind_the_balancer():
    """Eight receivers on ONE row (max_rows = 1): an input-rate tune to every burst and to every mirror.  Their events are the
    oracle's behind the restatement: every burst is decoded, no mirror receiver decodes -- where the oracle of the raw row decodes
    every burst twice (test_iqbal_cpu.py)."""
    p, q = GHOST_RATE
    raw, _ = ghost_scene()
    tunes = [sgn * f for f in GHOST_FREQS for sgn in (1, -1)]
    sizes = (2, 2, 2)
    assert sum(sizes) == GHOST_BLOCKS

    def before(r, k):
        if k == 0:
            assert r.iq() == (GHOST_K, 1) and r.dc() == (0, 0)
            r.map_streams(list(range(8)), [0] * 8)
            r.tune_streams_input(list(range(8)), tunes)
            assert r.rows_in_use == 1

    evs, _ = parity.run_input(raw.reshape(1, -1), sizes, p, q, "s16", types=TYPES, thresh=THRESH, before=before, n_streams=8, stage0=False,
                              all_flushes=True, iq_windows=GHOST_K, dc_rows=1)
    ev = np.concatenate(evs)
    oracles = ghost_oracles(True)
    for s, orc in enumerate(oracles):
        parity.assert_segment(ev, s, orc, "receiver at %d Hz" % tunes[s])
        assert parity.decoded(orc) == ([s // 2] if s % 2 == 0 else [])
    told = ev[ev["status"] == 1]
    assert sorted(zip(told["stream"].tolist(), told["slot"].tolist())) == [(2 * j, j) for j in range(len(GHOST_FREQS))]


# ---- state and queueing
def test_reset_iq_rows_on_one_of_two_rows():
    fmt, k_dc, k_iq, sizes = "u8", 4, 100, (1, 1, 1)
    rows = scene(fmt, 1, 1, 4)[:, :3 * api.BLOCK_BYTES]
    want = balanced(rows, fmt, k_dc, k_iq, sizes, reset_before={1: (1,)})
    carried = balanced(rows, fmt, k_dc, k_iq, sizes)
    evs, y0, ds, tgs, _ = run_iq(rows, sizes, 1, 1, fmt, k_dc, k_iq,
                                 before=lambda r, i: (r.reset_iq_rows([1, 1]), r.reset_iq_rows([])) if i == 1 else None)  # a duplicate; n == 0
    assert_estimates(ds, tgs, want, sizes)  # (d is the carried one: the blocker's state is not the balancer's)
    ev = np.concatenate(evs)
    for s in range(2):
        parity.assert_stage0(y0, sizes, want[s][0], s)
        # the streams were not restarted: one oracle over the whole row
        assert parity.assert_segment(ev, s, oracle_of(want[s][0]), "stream %d" % s) > 0
    assert np.array_equal(want[0][2][1], carried[0][2][1]) and not np.array_equal(want[1][2][1], carried[1][2][1])
    assert all(np.array_equal(want[1][1][i], carried[1][1][i]) for i in range(3))


def test_a_stream_reset_leaves_the_estimates_unchanged():
    fmt, p, q, k_dc, k_iq, sizes = "s16", 25, 16, 4, 100, (1, 2)
    rows = scene(fmt, p, q, 4)[:, :dcblock.input_samples(3, p, q) * 4]
    want = balanced(rows, fmt, k_dc, k_iq, sizes, p, q)
    evs, y0, ds, tgs, _ = run_iq(rows, sizes, p, q, fmt, k_dc, k_iq, before=lambda r, i: r.reset_streams([0]) if i == 1 else None)
    assert_estimates(ds, tgs, want, sizes)
    cut = 2 * dcblock.input_samples(1, p, q)
    # stream 0 restarts on the corrected samples behind the cut, from a history of x = 0; stream 1 runs on
    x0 = want[0][0]
    first, second = stage0_of_x(x0[:cut], p, q), stage0_of_x(x0[cut:], p, q)
    assert np.array_equal(y0[0][0], first) and np.array_equal(y0[1][0], second)
    parity.assert_segment(evs[0], 0, oracle_of(first), "stream 0 before the reset")
    parity.assert_segment(evs[1], 0, oracle_of(second), "stream 0 after the reset")
    parity.assert_stage0(y0, sizes, stage0_of_x(want[1][0], p, q), 1)
    assert parity.assert_segment(np.concatenate(evs), 1, oracle_of(stage0_of_x(want[1][0], p, q)), "stream 1") > 0


def test_two_submits_queued_before_the_first_read():
    fmt, k_dc, k_iq, sizes = "u8", 4, 3, (1, 2)
    rows = scene(fmt, 1, 1, 4)[:, :3 * api.BLOCK_BYTES]
    want = balanced(rows, fmt, k_dc, k_iq, sizes)
    parts = parity.to_device(parity.cut_input(rows, sizes, fmt))
    with api.Receiver(2, TYPES, THRESH, 0, max_blocks=2, all_flushes=True, dc_windows=k_dc, iq_windows=k_iq) as r:
        for part in parts:
            r.submit(part)
        evs = []
        for i in range(2):
            for s in range(2):
                assert np.array_equal(r.read_iq(s), want[s][2][i]), (i, s)
                assert np.array_equal(r.read_dc(s), want[s][1][i]), (i, s)
                assert np.array_equal(r.read_iq(s), want[s][2][i])  # reading pops nothing
            evs.append(r.drain())
        with pytest.raises(api.TfrecAmdError) as e:
            r.read_iq(0)
        assert e.value.code == api.E_STATE
    for s in range(2):
        assert parity.assert_segment(np.concatenate(evs), s, oracle_of(want[s][0]), "stream %d" % s) > 0


def test_submit_host_equals_submit_device():
    fmt, p, q, k_dc, k_iq, sizes = "f32", 4, 3, 4, 64, (3,)
    unit = dcblock.input_samples(3, p, q) * 8
    rows = scene(fmt, p, q, 12)[:, 2 * unit:3 * unit]  # (the unit with the bursts)
    a = run_iq(rows, sizes, p, q, fmt, k_dc, k_iq)
    b = run_iq(rows, sizes, p, q, fmt, k_dc, k_iq, host=True)
    assert len(a[0][0]) > 0 and parity.sort_events(a[0][0]).tobytes() == parity.sort_events(b[0][0]).tobytes()
    for s in range(2):
        assert np.array_equal(a[1][0][s], b[1][0][s]) and np.array_equal(a[2][0][s], b[2][0][s]) and np.array_equal(a[3][0][s], b[3][0][s])
    assert (a[3][0][0] != IDENT).any()


# ---- the rest
def test_more_rows_than_max_rows_are_refused_and_nothing_is_queued():
    import torch

    for k_dc in (0, 4):
        rows = scene("u8", 1, 1, 4, k_dc > 0)[:, :api.BLOCK_BYTES]
        d_rows = torch.from_numpy(np.ascontiguousarray(rows)).to("cuda:0")
        with api.Receiver(2, TYPES, THRESH, 0, max_blocks=1, all_flushes=True, dc_windows=k_dc or None, iq_windows=64, dc_rows=1) as r:
            for part in (d_rows, np.ascontiguousarray(rows)):  # two rows in use, one allowed
                with pytest.raises(api.TfrecAmdError) as e:
                    r.submit(part)
                assert e.value.code == api.E_INVAL
            with pytest.raises(api.TfrecAmdError) as e:
                r.read_iq(0)  # nothing was queued
            assert e.value.code == api.E_STATE and len(r.drain()) == 0
            r.map_streams([1], [0])
            assert r.submit(d_rows[:1]) == 1
            want, = balanced(rows[:1], "u8", k_dc, 64, (1,))
            assert np.array_equal(r.read_iq(0), want[2][0])  # the row's first window ever: the refused submits left no state
            ev = r.drain()
            for s in range(2):
                parity.assert_segment(ev, s, oracle_of(want[0]), "stream %d" % s)


def test_memory_counts_everything_the_balancer_holds():
    n, nb, k_dc, k, rows = 4, 3, 100, 70, 3
    for p, q, fmt in ((1, 1, "u8"), (25, 16, "f32")):
        with api.Receiver(n, TYPES, THRESH, 0, max_blocks=nb, input_format="s16", input_rate=(p, q)) as r:
            base = r.memory()
        with api.Receiver(n, TYPES, THRESH, 0, max_blocks=nb, input_format=fmt, input_rate=(p, q), dc_windows=k_dc, dc_rows=rows) as r:
            dc = r.memory()
        with api.Receiver(n, TYPES, THRESH, 0, max_blocks=nb, input_format=fmt, input_rate=(p, q), dc_windows=k_dc, iq_windows=k, dc_rows=rows) as r:
            both = r.memory()
        with api.Receiver(n, TYPES, THRESH, 0, max_blocks=nb, input_format=fmt, input_rate=(p, q), iq_windows=k, dc_rows=rows) as r:
            alone = r.memory()
        n_max = nb * 32768 * p // q
        nw = n_max // 512
        assert n_max % 512 == 0
        per_set = rows * nw * 4  # the table of (t, g)
        per_ctx = rows * nw * (32 + 24) + rows * k * 24 + rows * 8  # a submit's sums and moments, the ring, the counts
        assert both["device_bytes"] - dc["device_bytes"] == api.FIFO_DEPTH * per_set + per_ctx, (p, q)
        assert alone["device_bytes"] - base["device_bytes"] == api.FIFO_DEPTH * (per_set + rows * n_max * 4) + per_ctx, (p, q)  # + its rows
        assert both["pinned_host_bytes"] == alone["pinned_host_bytes"] == base["pinned_host_bytes"]


def test_older_contexts_beside_a_balancer_give_what_they_gave():
    """A tfrec_amd_create_dc and a tfrec_amd_create_format context, made and run while a balancer context lives: their events are
    the restatements' -- the DC blocker's and the plain format's."""
    fmt, sizes = "u8", (1, 2)
    rows = scene(fmt, 1, 1, 4, False)[:, :3 * api.BLOCK_BYTES]  # (no offset: the plain format context decodes too)
    parts = parity.to_device(parity.cut_input(rows, sizes, fmt))
    with api.Receiver(2, TYPES, THRESH, 0, max_blocks=2, all_flushes=True, input_format=fmt, dc_windows=4, iq_windows=64) as r:
        r.submit(parts[0])
        with api.Receiver(2, TYPES, THRESH, 0, max_blocks=2, all_flushes=True, input_format=fmt, dc_windows=64) as rd, \
                api.Receiver(2, TYPES, THRESH, 0, max_blocks=2, all_flushes=True, input_format="s8") as rf:
            assert rd.iq() == (0, 0) and rf.iq() == (0, 0) and rd.dc() == (64, 2)
            ed, ef = [], []
            for part in parts:
                rd.submit(part)
                rf.submit(part ^ 0x80)  # (the same samples as s8)
                for call in (lambda: rd.read_iq(0), lambda: rf.read_iq(0), lambda: rd.reset_iq_rows([0]), lambda: rf.reset_iq_rows([])):
                    with pytest.raises(api.TfrecAmdError) as e:
                        call()
                    assert e.value.code == api.E_INVAL
                ed.append(rd.drain())
                ef.append(rf.drain())
        r.drain()
    ed, ef = np.concatenate(ed), np.concatenate(ef)
    for s in range(2):
        pos, st, xs = 0, None, []
        for nb in sizes:
            x, _, st = dcblock.dc_block(rows[s][pos:pos + nb * api.BLOCK_BYTES], fmt, 64, st)
            xs.append(x)
            pos += nb * api.BLOCK_BYTES
        assert parity.assert_segment(ed, s, oracle_of(np.concatenate(xs)), "dc stream %d" % s) > 0
        assert parity.assert_segment(ef, s, oracle_of(formats.to_x(fmt, rows[s])), "format stream %d" % s) > 0


def test_refusals_on_a_device():
    L = api.load_library()
    C = api.C
    for kw in (dict(iq_windows=0), dict(iq_windows=4097), dict(iq_windows=64, dc_windows=4097), dict(iq_windows=64, dc_windows=-1),
               dict(iq_windows=64, dc_rows=0), dict(iq_windows=64, dc_rows=3), dict(iq_windows=64, input_rate=(1, 2)),
               dict(iq_windows=64, input_10x=True)):
        with pytest.raises(api.TfrecAmdError) as e:
            api.Receiver(2, TYPES, THRESH, 0, max_blocks=1, **kw)
        assert e.value.code == api.E_INVAL, kw
    rows = scene("u8", 1, 1, 4, False)[:, :api.BLOCK_BYTES]
    with api.Receiver(2, TYPES, THRESH, 0, max_blocks=1, all_flushes=True, iq_windows=64, dc_windows=0) as r:
        assert r.iq() == (64, 2) and r.dc() == (0, 0)
        nw = C.c_int(7)
        assert L.tfrec_amd_read_iq(r.h, 0, None, 0, C.byref(nw)) == api.E_STATE and nw.value == 0  # nothing undrained
        for bad in ([2], [-1], [0, 5]):
            with pytest.raises(api.TfrecAmdError) as e:
                r.reset_iq_rows(bad)
            assert e.value.code == api.E_INVAL
        with pytest.raises(api.TfrecAmdError) as e:
            r.reset_dc_rows([0])  # no blocker on this context
        assert e.value.code == api.E_INVAL
        assert L.tfrec_amd_reset_iq_rows(r.h, None, 1) == api.E_INVAL and L.tfrec_amd_reset_iq_rows(r.h, None, -1) == api.E_INVAL
        r.submit(np.ascontiguousarray(rows))
        want = balanced(rows, "u8", 0, 64, (1,))  # (the refused [0, 5] marked nothing: row 0's estimate is a first submit's)
        tg = np.full((64, 2), 77, dtype=np.int16)
        assert L.tfrec_amd_read_iq(r.h, 0, tg.ctypes.data, 63, C.byref(nw)) == api.E_INVAL and nw.value == 64 and (tg == 77).all()
        assert L.tfrec_amd_read_iq(r.h, 0, None, 64, C.byref(nw)) == api.E_INVAL and nw.value == 64
        assert L.tfrec_amd_read_iq(r.h, 0, tg.ctypes.data, 64, None) == api.E_INVAL
        for bad in (2, -1):
            with pytest.raises(api.TfrecAmdError) as e:
                r.read_iq(bad)
            assert e.value.code == api.E_INVAL
        assert L.tfrec_amd_read_iq(r.h, 1, tg.ctypes.data, 64, C.byref(nw)) == api.E_OK and np.array_equal(tg, want[1][2][0])
        assert np.array_equal(r.read_iq(0), want[0][2][0])
        ev = r.drain()
        parity.assert_segment(ev, 0, oracle_of(want[0][0]), "stream 0")


# ---- tfrec_gpu -Z
def cli_oracle(x, hz):
    """tfrec_gpu's receiver at hz from the centre on the input-rate samples x: the tune behind the resampler within +-767 kHz, the
    input-rate tune beyond."""
    if abs(hz) >= 768000:
        return receiver_oracle(x, hz)
    p, q = GHOST_RATE
    o = O.Oracle(TYPES, THRESH, 0)
    o.process_s16(tune.mix_s16(resample.resample_x16(x, p, q), hz, 0))
    return o


def test_cli_prints_no_ghost_with_Z(tmp_path):
    """tfrec_gpu -Z -F s16 -r 2400000 on the ghost scene, given eight times with a receiver at every burst and every mirror: the four
    bursts' telegrams, as the oracle prints them behind the restatement, and nothing else; without -Z the ghosts are there too.
    -D: an iq line per submit with the restatement's last estimate."""
    cli = parity.build_cli()
    raw, _ = ghost_scene()
    f = tmp_path / "ghost.cs16"
    raw.tofile(f)
    c = 868250
    tunes = [sgn * hz for hz in GHOST_FREQS for sgn in (1, -1)]
    base = ["-F", "s16", "-r", "2400000", "-c", str(c), "-T", "%x" % TYPES, "-t", str(THRESH), "-b", "2"]
    args = []
    for hz in tunes:
        args += ["-p", "f=%d" % (c + hz // 1000), "-L", str(f)]
    y = iqbal.iq_balance(raw, "s16", 0, GHOST_K)[0]
    want = []
    for s, hz in enumerate(tunes):
        lines = parity.telegram_lines(cli_oracle(y, hz).text())
        assert len(lines) == (1 if s % 2 == 0 else 0), hz
        want += lines
    out = subprocess.run([cli, "-Z"] + base + args, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    assert parity.telegram_lines(out.stdout) == want and len(want) == len(GHOST_FREQS)
    out = subprocess.run([cli] + base + args, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    assert len(parity.telegram_lines(out.stdout)) > len(want)  # the ghosts
    out = subprocess.run([cli, "-Z", "64", "-D"] + base + ["-L", str(f)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    tg = iqbal.iq_balance(raw, "s16", 0, 64)[2]
    per = dcblock.input_samples(2, *GHOST_RATE) // 512
    assert [ln for ln in out.stdout.splitlines() if ln.startswith("iq ")] == \
        ["iq %s t=%d g=%d" % (f, tg[(i + 1) * per - 1, 0], tg[(i + 1) * per - 1, 1]) for i in range(GHOST_BLOCKS // 2)]


def test_cli_queue_mode_starts_a_new_estimate_with_a_new_file(tmp_path):
    """tfrec_gpu -n 1: two files go through one stream, one after the other.  At K = 4096 -- longer than both -- the second file's
    estimates are those of that file alone only if the slot's row was reset with its stream."""
    cli = parity.build_cli()
    _, x = ghost_scene()
    files, want = [], []
    per = dcblock.input_samples(2, *GHOST_RATE) // 512
    for name, z in (("a", x), ("b", impair(x, 0.9, -6.0))):
        f = tmp_path / ("%s.cs16" % name)
        raw = formats.encode("s16", z)
        raw.tofile(f)
        _, d, tg, _ = iqbal.iq_balance(raw, "s16", 4096, 4096)
        files += ["-L", str(f)]
        for i in range(GHOST_BLOCKS // 2):
            w = (i + 1) * per - 1
            want += ["dc %s I=%d Q=%d" % (f, d[w, 0], d[w, 1]), "iq %s t=%d g=%d" % (f, tg[w, 0], tg[w, 1])]
    out = subprocess.run([cli, "-z", "4096", "-Z", "4096", "-D", "-n", "1", "-b", "2", "-F", "s16", "-r", "2400000", "-T", "%x" % TYPES, "-t",
                          str(THRESH)] + files, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    assert [ln for ln in out.stdout.splitlines() if ln.startswith(("dc ", "iq "))] == want
    assert want[5].split(" ", 2)[2] != want[11].split(" ", 2)[2]  # (the two files' last estimates differ)
