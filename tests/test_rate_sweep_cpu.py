"""The resampling stage across its whole rate range, without a GPU: the library's tap table against the restatement
tfrec_amd/resample.py at EVERY accepted rate P/Q (gcd 1, Q <= 64, 1 < P/Q < 10: 11 339 rates), the properties the kernels rely
on at every one of them, and what the rates, rows and expectations of the GPU sweep (input_rows.py's RATE_SWEEP) are there for.

Everything is bit-exact; nothing here has a tolerance."""
import math

import numpy as np
import pytest

from input_rows import (LDS_LIMIT, RATE_SWEEP, RATE_SWEEP_FORMAT, RATE_SWEEP_IDS, rate_sweep_rows, rate_sweep_sizes, rate_sweep_stage0,
                        rate_sweep_tunes, raw_chunks, tile_of, tuned_lds)
from tfrec_amd import api, formats, resample, tune


def all_rates():
    return [(p, q) for q in range(1, resample.Q_MAX + 1) for p in range(q + 1, 10 * q) if math.gcd(p, q) == 1]


def plain_lds(p, q, t):
    """Bytes of LDS of resample_kernel (input_rows.tuned_lds: of a tuned launch): the table and the raw image (4 dwords per chunk),
    always a whole tile."""
    return (((q * t + 3) & ~3) + 4 * raw_chunks(p, q, t, 1024)) * 4


# ---- every rate
def test_every_rate_library_taps_equal_the_restatement():
    """All 11 339 rates in one loop (about half a minute, most of it the restatement's scalar definition): the C library's table
    and resample.taps either both refuse or are the same int32 table; exactly 399/41 is refused (v = 110.50000000091906 at
    phase 12, 9.19e-10 from a rounding tie: inside the 1e-9 guard on both sides, whose sums differ in their last bits); and
    every accepted table has what the kernels assume of it."""
    refused, n, worst = set(), 0, (0, None)
    for p, q in all_rates():
        try:
            got = api.resample_taps(p, q)
        except api.TfrecAmdError as e:
            assert e.code == api.E_INVAL, (p, q)
            got = None
        try:
            want = resample.taps(p, q)
        except resample.RateError:
            want = None
        n += 1
        assert (got is None) == (want is None), "%d/%d: one side refuses, the library %s" % (p, q, "refuses" if got is None else "accepts")
        if want is None:
            refused.add((p, q))
            continue
        t = resample.n_taps(p, q)
        assert got.dtype == np.int32 and want.dtype == np.int32 and got.shape == want.shape == (q, t), (p, q)
        assert np.array_equal(got, want), "%d/%d: first differing (phase, tap) %s" % (p, q, np.argwhere(got != want)[0].tolist())
        assert 8 <= t <= 60 and t % 2 == 0, (p, q)
        h = want.astype(np.int64)
        assert (h.sum(axis=1) == 65536).all(), (p, q)  # unity DC gain, every phase
        assert np.abs(h).max() < 1 << 17, (p, q)  # h / 1024 and h / 65536 are exact in fp32
        a = int(np.abs(h).sum(axis=1).max())
        assert (a * 8192) >> 16 < 32768, (p, q, a)  # the int16 store cannot wrap for u8, s8, s16 or f32 input
        assert (a * 11585) >> 16 < 32768, (p, q, a)  # ... nor behind the input-rate tune (tfrec_amd_tune_streams_input's guard)
        worst = max(worst, (a, (p, q)))
    assert n == 11339
    assert refused == {(399, 41)}
    assert worst == (108112, (65, 64))  # csrc/resample.h: "108112 at 65/64 is the largest sum |h| of any accepted rate"


# ---- the sweep's rates
def test_sweep_rates_are_what_they_are_there_for():
    """Non-vacuity of test_rate_sweep_gpu.py: each rate has the T, the Q, the block unit and the side of the whole-tile /
    half-tile decision it is listed with, computed from the geometry csrc/resample.h documents."""
    for p, q, t, unit, tile, fmt in RATE_SWEEP:
        assert math.gcd(p, q) == 1 and q <= 64 and q < p < 10 * q
        assert resample.n_taps(p, q) == t and resample.permitted_blocks(q) == unit, (p, q)
        assert tile_of(p, q, t) == tile, (p, q, tuned_lds(p, q, t, 1024))
        assert tuned_lds(p, q, t, tile) <= LDS_LIMIT and plain_lds(p, q, t) <= LDS_LIMIT
    by_rate = {r[:2]: r for r in RATE_SWEEP}
    assert len(by_rate) == len(RATE_SWEEP) == 15
    # the edges of T and Q
    assert min(all_rates(), key=lambda r: r[0] / r[1]) == (65, 64) and resample.abs_sum_max(65, 64) == 108112
    assert [by_rate[r][2] for r in ((65, 64), (3, 2), (127, 64))] == [8, 10, 12] and 2 * 127 < 2 * 2 * 64
    assert [by_rate[r][2] for r in ((2, 1), (4, 1), (9, 1))] == [12, 24, 54]
    assert by_rate[19, 2][2] == 58 and by_rate[39, 4][2] == by_rate[639, 64][2] == 60
    assert max(all_rates(), key=lambda r: r[0] / r[1]) == (639, 64)
    assert sorted({r[3] for r in RATE_SWEEP}) == [1, 3, 5]
    # the whole-tile / half-tile threshold, from both sides
    lds = {r: tuned_lds(r[0], r[1], resample.n_taps(*r), 1024) for r in all_rates()}
    half = sorted((v, r) for r, v in lds.items() if v > LDS_LIMIT)
    assert len(lds) == 11339 and len(half) == 2567
    assert lds[461, 64] == LDS_LIMIT == max(v for v in lds.values() if v <= LDS_LIMIT)
    assert lds[39, 4] == 49344 and lds[267, 32] == 49248 and lds[463, 64] == 49280 and lds[639, 64] == max(lds.values())
    # (below 49248 lie only steps of 16 and 32 bytes over the limit: 267/32 and 463/64 are the first of their Q)
    assert min(v for v, r in half if r[1] == 32) == 49248 and min(v for v, r in half if r[1] == 64) == 49280
    assert max(plain_lds(r[0], r[1], resample.n_taps(*r)) for r in all_rates()) == plain_lds(639, 64, 60) == 35936
    assert max(tuned_lds(r[0], r[1], resample.n_taps(*r), 512) for _, r in half) <= LDS_LIMIT
    # every format of case (d) meets a whole-tile and a half-tile rate
    assert {(r[5], r[4]) for r in RATE_SWEEP} == {(f, n) for f in ("s8", "s16", "f32") for n in (512, 1024)}
    assert [r[5] for r in RATE_SWEEP] == ["s8", "s16", "f32"] * 5


@pytest.mark.parametrize("p,q", [r[:2] for r in RATE_SWEEP], ids=RATE_SWEEP_IDS)
def test_cutting_the_sweep_rows_reproduces_the_stream(p, q):
    """What the GPU sweep expects is consistent in itself: the sweep's u8 row cut into its (unit, 2 unit, unit) submits, each
    from the T - 1 raw samples before it, is the uncut stream; and so is the (d)-format row behind tune.mix_in_s16 with the phase
    carried (the history is rotated with its own sample numbers) and resample_x16.  An untuned stream of a tuned launch is the
    untuned restatement."""
    t = resample.n_taps(p, q)
    sizes = rate_sweep_sizes(q)
    u8 = rate_sweep_rows("u8", p, q)[0]
    parts, pos = [], 0
    for nb in sizes:
        n = 2 * resample.input_samples(nb, p, q)
        parts.append(resample.resample_s16(u8[pos:pos + n], p, q, hist=u8[pos - 2 * (t - 1):pos] if pos else None))
        assert len(parts[-1]) == 2 * nb * 32768
        pos += n
    assert pos == len(u8) and np.array_equal(np.concatenate(parts), rate_sweep_stage0("u8", p, q, False)[0])
    assert np.array_equal(rate_sweep_stage0("u8", p, q, True)[1], rate_sweep_stage0("u8", p, q, False)[1])
    assert not np.array_equal(rate_sweep_stage0("u8", p, q, True)[0], rate_sweep_stage0("u8", p, q, False)[0])

    fmt = RATE_SWEEP_FORMAT[p, q]
    hz = rate_sweep_tunes(p, q)[0]
    assert 2 * (hz + 1234) * q < 1536000 * p <= 2 * (hz + 1235) * q  # 1234 Hz inside the limit
    x = formats.to_x(fmt, rate_sweep_rows(fmt, p, q)[0])
    assert x.min() == -8192 and x.max() == (8128 if fmt == "s8" else 8191)
    parts, pos = [], 0  # (pos counts int16 values: two per complex sample)
    for nb in sizes:
        n = 2 * resample.input_samples(nb, p, q)
        lead = 2 * (t - 1) if pos else 0
        m = tune.mix_in_s16(x[pos - lead:pos + n], hz, p, q, (pos - lead) // 2)
        parts.append(resample.resample_x16(m[lead:], p, q, hist=m[:lead] if lead else None))
        pos += n
    assert pos == len(x) and np.array_equal(np.concatenate(parts), rate_sweep_stage0(fmt, p, q, True)[0])
    assert np.array_equal(rate_sweep_stage0(fmt, p, q, True)[1], rate_sweep_stage0(fmt, p, q, False)[1])
