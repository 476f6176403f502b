"""The whole-kHz rates of the resampling stage on the GPU (Q | 1536), bit for bit: the staged kernels at the new
denominators whose table still fits (125/96, 625/384, 129/128) and resample_stream_kernel where it does not (3125/384, 735/512,
1537/1536, 15359/1536), in every format, untuned and with mixed tunes in one launch -- among them the tunes whose increment
needs a 128-bit numerator --, across a reset and on a shared row; the decode behind the stage end to end; the DC blocker and the
refusals under the block rule unit(Q) = Q / gcd(Q, 64).

input_rows.py holds the rates, rows and scenes; test_khz_rates_cpu.py asserts what each is there for.  Every sweep run is full-scale data
over submits of (unit, 2 unit, unit) blocks -- (24, 24) at Q = 1536 -- on a context of the largest: stage 0 is read back after each
submit and compared per stream and submit with the restatement (tfrec_amd/resample.py, tune.py, formats.py) by np.array_equal."""
import numpy as np
import pytest

import parity
from input_rows import (KHZ_SCENE_RATES, KHZ_SWEEP, KHZ_SWEEP_BY_RATE, KHZ_SWEEP_IDS, THRESH, TYPES, format_stage0, khz_scene, khz_sweep_rows,
                        khz_sweep_stage0, khz_sweep_tunes, oracle_of, rate_scene)
from tfrec_amd import api, dcblock, formats, resample, tune

pytestmark = pytest.mark.gpu

RATES = [r[:2] for r in KHZ_SWEEP]


def stage0_run(fmt, rows, sizes, p, q, before=None, n_streams=None):
    """A u8 rate receiver (the older constructor) or a format receiver over the rows -> stage 0 per submit and stream."""
    return parity.run_input(rows, sizes, p, q, None if fmt == "u8" else fmt, types=TYPES, thresh=THRESH, before=before,
                            n_streams=n_streams, all_flushes=True, max_events=1 << 16)[1]


def sweep(fmt, p, q, tuned):
    _, _, n, sizes, fmts, _ = KHZ_SWEEP_BY_RATE[p, q]
    assert fmt in fmts  # (15359/1536 runs u8 and s16 only)
    hz = khz_sweep_tunes(p, q, fmt)

    def before(r, k):
        if tuned and k == 0:
            r.tune_streams_input(list(range(n)), hz)
            assert [r.stream_tune_input(s) for s in range(n)] == list(hz)

    y0 = stage0_run(fmt, khz_sweep_rows(fmt, p, q), sizes, p, q, before=before)
    want = khz_sweep_stage0(fmt, p, q, tuned)
    label = "%d/%d %s%s" % (p, q, fmt, " tuned" if tuned else "")
    for s in range(n):
        parity.assert_stage0(y0, sizes, want[s], s, label, 1024)
    if tuned:  # the tunes act: a tuned stream is not the untuned restatement
        s = [i for i in range(n) if hz[i]][0]
        assert not np.array_equal(want[s], khz_sweep_stage0(fmt, p, q, False)[s])


@pytest.mark.parametrize("p,q", RATES, ids=KHZ_SWEEP_IDS)
def test_u8_untuned(p, q):
    """resample_kernel where the table is staged, resample_stream_kernel<U8> where it is not."""
    sweep("u8", p, q, False)


@pytest.mark.parametrize("p,q", RATES, ids=KHZ_SWEEP_IDS)
def test_u8_mixed_tunes_in_one_launch(p, q):
    """Stream 0 tuned, stream 1 untuned, stream 2 tuned negative (15359/1536: +7000001 Hz and an untuned stream)."""
    sweep("u8", p, q, True)


FORMAT_CASES = [(fmt, r[0], r[1]) for r in KHZ_SWEEP for fmt in r[4][1:]]


@pytest.mark.parametrize("fmt,p,q", FORMAT_CASES, ids=["%s-%d/%d" % c for c in FORMAT_CASES])
def test_formats_untuned(fmt, p, q):
    sweep(fmt, p, q, False)


@pytest.mark.parametrize("p,q", RATES, ids=KHZ_SWEEP_IDS)
def test_one_format_with_mixed_tunes(p, q):
    """The format cycles down the table (15359/1536: s16 with an untuned stream and -699051 Hz)."""
    sweep(KHZ_SWEEP_BY_RATE[p, q][5], p, q, True)


# ---- beside the sweep
@pytest.mark.parametrize("fmt,p,q", [("u8", 1537, 1536), ("s16", 3125, 384)])
def test_reset_before_the_second_submit(fmt, p, q):
    """reset_streams([1]) before the second submit: from there stream 1 is the restatement of the remaining input from zero
    history and phase 0; stream 0 carries on."""
    sizes = KHZ_SWEEP_BY_RATE[p, q][3]
    rows = khz_sweep_rows(fmt, p, q)[:2]
    y0 = stage0_run(fmt, rows, sizes, p, q, before=lambda r, k: r.reset_streams([1]) if k == 1 else None)

    def restated(row):
        return resample.resample_s16(row, p, q) if fmt == "u8" else format_stage0(fmt, row, p, q)

    cut = formats.bytes_per_sample(fmt) * resample.input_samples(sizes[0], p, q)
    whole = khz_sweep_stage0(fmt, p, q, False)
    label = "%d/%d %s" % (p, q, fmt)
    parity.assert_stage0(y0, sizes, whole[0], 0, label + " beside a reset", 1024)
    n0 = 2 * sizes[0] * 4 * api.BLOCK_DEC
    assert np.array_equal(y0[0][1], whole[1][:n0])
    parity.assert_stage0(y0, sizes, restated(rows[1][cut:]), 1, label + " after the reset", 1024, first=1)
    assert not np.array_equal(y0[1][1][:16], whole[1][n0:][:16])  # the history is silence, not the carried stream's


def test_shared_row_with_three_input_tunes():
    """3125/384, f32: three streams read row 0 with three input tunes, and the submits carry that one row."""
    p, q, fmt = 3125, 384, "f32"
    sizes, hz = KHZ_SWEEP_BY_RATE[p, q][3], (6249999, 1234, -123457)
    row = khz_sweep_rows(fmt, p, q)[:1].copy()

    def before(r, k):
        if k == 0:
            r.map_streams([0, 1, 2], [0, 0, 0])
            r.tune_streams_input([0, 1, 2], hz)
            assert r.rows_in_use == 1

    y0 = stage0_run(fmt, row, sizes, p, q, before=before, n_streams=3)
    x = formats.to_x(fmt, row[0])
    for s in range(3):
        want = resample.resample_x16(tune.mix_in_s16(x, hz[s], p, q), p, q)
        parity.assert_stage0(y0, sizes, want, s, "3125/384 f32 shared row", 512)


@pytest.mark.parametrize("p,q", KHZ_SCENE_RATES)
def test_events_equal_the_oracle_behind_the_restatement(p, q):
    """End to end at 2.0 and 12.5 MS/s: every stream's events are the oracle's on the restatement's stage 0, every flush
    reported, with a decoded telegram in every stream."""
    iq = khz_scene(p, q)
    evs, _ = parity.run_input(iq, (6, 6), p, q, types=TYPES, thresh=THRESH, stage0=False, all_flushes=True)
    ev = np.concatenate(evs)
    for s in range(len(iq)):
        orc = oracle_of(iq[s], p, q)
        assert parity.assert_segment(ev, s, orc, "%d/%d stream %d" % (p, q, s)) > 0
        assert len(parity.decoded(orc)) >= 1, s


def test_dc_blocker_at_2500000():
    """tfrec_amd_create_dc at 625/384, s8, K = 64, submits of (6, 6): d per window and stage 0 are the restatement's
    (dcblock.dc_block ahead of resample_x16); a submit of 3 blocks -- whole samples, not a multiple of the unit -- is refused
    and queues nothing."""
    p, q, fmt, k, sizes = 625, 384, "s8", 64, (6, 6)
    rows = khz_sweep_rows(fmt, p, q)[:2, :formats.bytes_per_sample(fmt) * resample.input_samples(12, p, q)]
    parts = parity.cut_input(rows.copy(), sizes, fmt, p, q)
    with api.Receiver(2, TYPES, THRESH, 0, max_blocks=6, input_format=fmt, input_rate=(p, q), dc_windows=k, all_flushes=True) as r:
        assert r.dc() == (k, 2)
        with pytest.raises(api.TfrecAmdError) as e:
            r.submit(parts[0], n_blocks=3)
        assert e.value.code == api.E_INVAL
        got_d, y0 = [], []
        for i, part in enumerate(parity.to_device(parts)):
            assert r.input_bytes(sizes[i]) == part.shape[1]
            r.submit(part)
            y0.append([r.stage0(s, sizes[i] * 4 * api.BLOCK_DEC) for s in range(2)])
            got_d.append([r.read_dc(row) for row in range(2)])
            r.drain()
    for s in range(2):
        st, xs = None, []
        for i, part in enumerate(parts):
            x, d, st = dcblock.dc_block(part[s], fmt, k, st)
            assert len(d) == dcblock.input_samples(sizes[i], p, q) // 512
            assert got_d[i][s].shape == d.shape and np.array_equal(got_d[i][s], d), (s, i)
            xs.append(x)
        parity.assert_stage0(y0, sizes, resample.resample_x16(np.concatenate(xs), p, q), s, "625/384 s8 behind the DC blocker", 1024)


def test_refusals_leave_the_context_usable():
    """625/384: 1, 3 and 4 blocks are no multiple of 6 (3 would be a whole number of samples); nothing is queued or marked, and
    a submit of 6 then decodes as on a fresh context."""
    p, q = 625, 384
    iq = rate_scene(p, q, n_blocks=6)
    with api.Receiver(2, TYPES, THRESH, 0, max_blocks=6, all_flushes=True, input_rate=(p, q)) as r:
        for nb in (1, 3, 4):
            with pytest.raises(api.TfrecAmdError) as e:
                r.input_bytes(nb)
            assert e.value.code == api.E_INVAL
            with pytest.raises(api.TfrecAmdError) as e:
                r.submit(iq, n_blocks=nb)
            assert e.value.code == api.E_INVAL
        assert r.input_bytes(6) == iq.shape[1] == 2 * 6 * 32768 * p // q
        assert r.submit(iq) == 6
        ev = r.drain()
        for s in range(2):
            assert parity.assert_segment(ev, s, oracle_of(iq[s], p, q), "stream %d" % s) > 0
