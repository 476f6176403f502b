"""The resampling kernels on the GPU across the rate range, bit for bit: resample_kernel, resample_fmt_kernel<U8> (the tuned u8 kernel) and
resample_fmt_kernel<S8 | S16 | F32> at the rates of input_rows.RATE_SWEEP (the edges of T, Q, the LDS and the
whole-tile / half-tile decision; test_rate_sweep_cpu.py asserts what each rate is there for and that the expectations are consistent in
themselves), and ingest_kernel's row lookup.

Every run is three streams of different full-scale data over submits of (unit, 2 unit, unit) blocks on a context of 2 units:
both history buffers are used and the first is reused, the phase carries twice, and a submit is smaller than the context's
buffers.  Stage 0 is read back after each submit and compared per stream and submit with the restatement
(tfrec_amd/resample.py, tune.py, formats.py); every comparison is np.array_equal."""
import numpy as np
import pytest

import parity
from input_rows import (RATE_SWEEP, RATE_SWEEP_FORMAT, RATE_SWEEP_IDS, RATE_SWEEP_STREAMS, THRESH, TYPES, format_stage0, rate_sweep_rows,
                        rate_sweep_sizes, rate_sweep_stage0, rate_sweep_tunes, tile_of)
from tfrec_amd import api, formats, resample, tune

pytestmark = pytest.mark.gpu

RATES = [r[:2] for r in RATE_SWEEP]


def stage0_run(fmt, rows, sizes, p, q, before=None, n_streams=None):
    """A u8 rate receiver (the older constructor) or a format receiver over the rows -> stage 0 per submit and stream.
    max_blocks is the largest submit."""
    return parity.run_input(rows, sizes, p, q, None if fmt == "u8" else fmt, types=TYPES, thresh=THRESH, before=before,
                            n_streams=n_streams, all_flushes=True, max_events=1 << 16)[1]


def tune_first(p, q):
    hz = rate_sweep_tunes(p, q)

    def before(r, k):
        if k == 0:
            r.tune_streams_input(list(range(RATE_SWEEP_STREAMS)), hz)
            assert [r.stream_tune_input(s) for s in range(RATE_SWEEP_STREAMS)] == list(hz)

    return before


def sweep(fmt, p, q, tuned):
    sizes = rate_sweep_sizes(q)
    y0 = stage0_run(fmt, rate_sweep_rows(fmt, p, q), sizes, p, q, before=tune_first(p, q) if tuned else None)
    want = rate_sweep_stage0(fmt, p, q, tuned)
    label = "%d/%d %s%s" % (p, q, fmt, " tuned" if tuned else "")
    tile = 1024 if fmt == "u8" and not tuned else tile_of(p, q, resample.n_taps(p, q))
    for s in range(RATE_SWEEP_STREAMS):
        parity.assert_stage0(y0, sizes, want[s], s, label, tile)


@pytest.mark.parametrize("p,q", RATES, ids=RATE_SWEEP_IDS)
def test_u8_untuned(p, q):
    """(a) resample_kernel: the kernel tfrec_gpu -r uses by default."""
    sweep("u8", p, q, False)


@pytest.mark.parametrize("p,q", RATES, ids=RATE_SWEEP_IDS)
def test_u8_mixed_tunes_in_one_launch(p, q):
    """(b) resample_fmt_kernel<U8>, the tuned u8 kernel: stream 0 tuned 1234 Hz inside the limit, stream 1 untuned, stream 2 tuned to -123457 Hz."""
    sweep("u8", p, q, True)


@pytest.mark.parametrize("p,q", RATES, ids=RATE_SWEEP_IDS)
@pytest.mark.parametrize("fmt", ["s8", "s16", "f32"])
def test_formats_untuned(fmt, p, q):
    """(c) resample_fmt_kernel<FMT> launched without the cosine table."""
    sweep(fmt, p, q, False)


@pytest.mark.parametrize("p,q", RATES, ids=RATE_SWEEP_IDS)
def test_one_format_with_mixed_tunes(p, q):
    """(d) resample_fmt_kernel<FMT> with the tunes of (b); the format cycles s8, s16, f32 down the table."""
    sweep(RATE_SWEEP_FORMAT[p, q], p, q, True)


# ---- beside the sweep
@pytest.mark.parametrize("fmt", ["s8", "s16", "f32"])
def test_base_rate_format_context_reads_mapped_rows(fmt):
    """ingest_kernel's `chan` path: on a 1/1 format context streams 0, 1, 2 read rows 1, 1, 0, and stage 0 of a stream is
    to_x of its row; a map back to the identity before the second submit takes effect."""
    sizes, rows_of = (1, 1), ([1, 1, 0], [0, 1, 2])
    n = resample.input_samples(sum(sizes), 1, 1)
    rows = np.concatenate([parity.full_scale_row(fmt, n, 11 + s) for s in range(3)])

    def before(r, k):
        r.map_streams([0, 1, 2], rows_of[k])
        assert [r.stream_input(s) for s in range(3)] == rows_of[k] and r.rows_in_use == (2, 3)[k]

    y0 = stage0_run(fmt, rows, sizes, 1, 1, before=before)
    half = rows.shape[1] // 2
    for k in range(2):
        for s in range(3):
            want = format_stage0(fmt, rows[rows_of[k][s], k * half:(k + 1) * half], 1, 1)
            assert np.array_equal(y0[k][s], want), "%s submit %d stream %d: %s" % (fmt, k, s, parity.first_difference(y0[k][s], want, 2048))
    assert not np.array_equal(y0[0][0], y0[0][2]) and not np.array_equal(y0[1][0], y0[1][1])


def test_shared_row_at_a_half_tile_rate():
    """39/4, f32: three streams read row 0 with three input tunes, and the submits carry that one row."""
    p, q, fmt = 39, 4, "f32"
    sizes, hz = rate_sweep_sizes(q), rate_sweep_tunes(p, q)
    row = rate_sweep_rows(fmt, p, q)[:1].copy()

    def before(r, k):
        if k == 0:
            r.map_streams([0, 1, 2], [0, 0, 0])
            r.tune_streams_input([0, 1, 2], hz)
            assert r.rows_in_use == 1

    y0 = stage0_run(fmt, row, sizes, p, q, before=before, n_streams=3)
    x = formats.to_x(fmt, row[0])
    for s in range(3):
        want = rate_sweep_stage0(fmt, p, q, True)[0] if s == 0 else resample.resample_x16(tune.mix_in_s16(x, hz[s], p, q), p, q)
        parity.assert_stage0(y0, sizes, want, s, "39/4 f32 shared row", 512)


@pytest.mark.parametrize("fmt,p,q", [("u8", 65, 64), ("s16", 39, 4)])
def test_reset_at_an_edge_rate(fmt, p, q):
    """reset_streams([1]) before the second submit: from there stream 1 is the restatement of the remaining input from zero
    history and phase 0; stream 0 carries on."""
    sizes = rate_sweep_sizes(q)
    if fmt == "u8":
        rows = parity.loud_and_quiet(p, q, sizes, 2, 1000 * p + q)
    else:
        rows = np.concatenate([parity.full_scale_row(fmt, resample.input_samples(sum(sizes), p, q), 31 + s) for s in range(2)])
    y0 = stage0_run(fmt, rows, sizes, p, q, before=lambda r, k: r.reset_streams([1]) if k == 1 else None)

    def restated(row):
        return resample.resample_s16(row, p, q) if fmt == "u8" else format_stage0(fmt, row, p, q)

    tile = 1024 if fmt == "u8" else tile_of(p, q, resample.n_taps(p, q))
    cut = formats.bytes_per_sample(fmt) * resample.input_samples(sizes[0], p, q)
    parity.assert_stage0(y0, sizes, restated(rows[0]), 0, "%d/%d %s beside a reset" % (p, q, fmt), tile)
    whole = restated(rows[1])
    n0 = 2 * sizes[0] * 4 * api.BLOCK_DEC
    assert np.array_equal(y0[0][1], whole[:n0])
    parity.assert_stage0(y0, sizes, restated(rows[1][cut:]), 1, "%d/%d %s after the reset" % (p, q, fmt), tile, first=1)
    assert not np.array_equal(y0[1][1][:16], whole[n0:][:16])  # the history is silence, not the carried stream's
