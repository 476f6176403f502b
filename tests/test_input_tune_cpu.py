"""The input-rate tune (tfrec_amd_tune_streams_input, tfrec_gpu -r with -f) without a GPU: the restatement
tfrec_amd/tune.py (inc_in, mix_in_s16) and tfrec_amd/resample.py (resample_x16) against the definition, the overflow guard,
the presence of the interface, tfrec_gpu's argument handling, and the scenes the GPU tests decode.

Everything is bit-exact; nothing here has a tolerance."""
import os
import re

import numpy as np
import pytest

import parity
from input_rows import WIDE_SCENES, input_oracle, wide_row
from tfrec_amd import api, resample, tune

# ---- inc_in
CORNERS = (0, 1, -1, 1000, -1000, 250000, -250000, 767999, -767999)


def test_inc_in_is_the_one_definition_for_every_rate():
    for f in CORNERS:
        assert tune.inc_in(f, 1, 1) == tune.inc(f)
    for f in CORNERS + (768000, -768000, 5000000, -5000000, 7679999, -7679999):
        assert tune.inc_in(f, 10, 1) == tune.inc10(f)
    assert tune.inc_in(1, 10, 1) == 280 and tune.inc_in(7679999, 10, 1) == 2 ** 31 - 280
    # written out once more, in big integers, for rates of their own
    for p, q in ((4, 3), (25, 16), (25, 12), (7, 5), (639, 64)):
        for f in (1, -1, 123456, -654321, (1536000 * p - 1) // (2 * q), -((1536000 * p - 1) // (2 * q))):
            num, den = f * 2 ** 33 * q + 1536000 * p, 2 * 1536000 * p
            assert tune.inc_in(f, p, q) == (num // den) % 2 ** 32
            assert abs(num) < 2 ** 63


@pytest.mark.parametrize("p,q", [(4, 3), (25, 16), (25, 12), (7, 5)])
def test_the_limit_is_half_the_input_rate_in_integers(p, q):
    """|tune_hz| < fs_in / 2, tested as 2 |tune_hz| Q < 1536000 P."""
    top = (1536000 * p + 2 * q - 1) // (2 * q) - 1  # the largest permitted |tune_hz|
    assert 2 * top * q < 1536000 * p <= 2 * (top + 1) * q
    for f in (top, -top):
        assert 0 < tune.inc_in(f, p, q) < 2 ** 32
    for f in (top + 1, -top - 1, 10 ** 7):
        with pytest.raises(ValueError):
            tune.inc_in(f, p, q)
    assert {(4, 3): 1023999, (25, 16): 1199999, (25, 12): 1599999, (7, 5): 1075199}[p, q] == top


@pytest.mark.parametrize("p,q,hz,n0", [(25, 16, 900000, 0), (4, 3, -1023999, 2 ** 32 - 37), (25, 12, 1300000, 2 ** 32 - 3),
                                       (7, 5, 1, 2 ** 31 + 5), (639, 64, -7000000, 12345678901)])
def test_mix_in_s16_equals_a_scalar_loop(p, q, hz, n0):
    rng = np.random.default_rng(p + q)
    x = tune.s16_of_u8(rng.integers(0, 256, 2 * 300, dtype=np.uint8))
    x[:4] = (-8192, -8192, 8128, -8192)  # the rails' corners
    got = tune.mix_in_s16(x, hz, p, q, n0)
    step = ((hz * 2 ** 33 * q + 1536000 * p) // (2 * 1536000 * p)) % 2 ** 32
    c, s = tune.table()
    for n in range(300):
        k = (((n0 + n) * step) % 2 ** 32) >> 20
        i, qq = int(x[2 * n]), int(x[2 * n + 1])
        ck, sk = int(c[k]), int(s[k])
        want = (max(-32768, min(32767, (i * ck + qq * sk + 2 ** 14) >> 15)), max(-32768, min(32767, (qq * ck - i * sk + 2 ** 14) >> 15)))
        assert (int(got[2 * n]), int(got[2 * n + 1])) == want, n
    assert np.abs(got.astype(np.int64)).max() <= 11585  # the mixer's output of u8 input
    assert np.array_equal(tune.mix_in_s16(x, 0, p, q, n0), x)


@pytest.mark.parametrize("p,q", [(4, 3), (25, 16), (25, 12), (75, 64), (639, 64)])
def test_resample_x16_equals_resample_s16_on_widened_input(p, q):
    rng = np.random.default_rng(3 * p + q)
    nb = resample.permitted_blocks(q)
    iq = rng.integers(0, 256, 2 * resample.input_samples(nb, p, q), dtype=np.uint8)[:2 * 6000]
    assert np.array_equal(resample.resample_x16(tune.s16_of_u8(iq), p, q), resample.resample_s16(iq, p, q))
    t = resample.n_taps(p, q)
    cut = 2 * 2000
    a = resample.resample_x16(tune.s16_of_u8(iq[cut:]), p, q, hist=tune.s16_of_u8(iq[cut - 2 * (t - 1):cut]))
    b = resample.resample_s16(iq[cut:], p, q, hist=iq[cut - 2 * (t - 1):cut])
    assert np.array_equal(a, b)


def accepted_rates():
    out = []
    for q in range(1, resample.Q_MAX + 1):
        for p in range(q + 1, 10 * q):
            if np.gcd(p, q) == 1:
                out.append((p, q))
    return out


def test_no_accepted_rate_trips_the_overflow_guard():
    """|y0| <= max_phi sum |h| * 11585 >> 16 must stay below 32768: over every accepted rate with the library's tables (which
    test_resample_cpu.py pins to the restatement), and with the restatement's own at the worst case, the common and the
    largest rates."""
    worst, n = (0, None), 0
    for p, q in accepted_rates():
        try:
            h = api.resample_taps(p, q)
        except api.TfrecAmdError:
            continue  # (a refused rate has no context to tune)
        n += 1
        a = int(np.abs(h.astype(np.int64)).sum(axis=1).max())
        assert (a * 11585) >> 16 < 32768, (p, q, a)
        worst = max(worst, (a, (p, q)))
    assert n == 11338 and worst == (108112, (65, 64))
    assert (108112 * 11585) >> 16 == 19111
    for p, q in ((65, 64), (4, 3), (25, 16), (25, 12), (639, 64), (19, 2)):
        a = resample.abs_sum_max(p, q)
        assert a == int(np.abs(api.resample_taps(p, q).astype(np.int64)).sum(axis=1).max()) and (a * 11585) >> 16 < 32768


# ---- the interface
def test_header_library_and_binding_have_the_calls():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "tfrec_amd.h")) as f:
        h = f.read()
    assert re.search(r"int tfrec_amd_tune_streams_input\(tfrec_amd_ctx \*ctx, const int32_t \*streams, const int32_t \*tune_hz, int n\);", h)
    assert re.search(r"int tfrec_amd_get_stream_tune_input\(tfrec_amd_ctx \*ctx, int stream, int32_t \*tune_hz\);", h)
    assert "tfrec_amd_tune_streams_input" in api.EXPORTS and "tfrec_amd_get_stream_tune_input" in api.EXPORTS
    L = api.load_library()
    assert L.tfrec_amd_tune_streams_input and L.tfrec_amd_get_stream_tune_input
    assert callable(api.Receiver.tune_streams_input) and callable(api.Receiver.stream_tune_input)
    assert L.tfrec_amd_tune_streams_input(None, None, None, 0) == api.E_INVAL
    assert L.tfrec_amd_get_stream_tune_input(None, 0, None) == api.E_INVAL


# ---- tfrec_gpu -r with -f: what is decided before a device is opened
@pytest.fixture(scope="module")
def cli():
    return parity.build_cli()


def test_cli_accepts_tunes_up_to_half_the_rate(cli, tmp_path):
    missing = str(tmp_path / "missing.iq")
    # beyond 767 kHz, below half the rate: accepted, the run ends at the missing file
    for rate, khz in (("2400000", 900), ("2400000", -1199), ("2048000", 1023), ("3200000", -1599), ("2400000", 767)):
        out = parity.run_cli(["-r", rate, "-c", "868250", "-f", str(868250 + khz), "-L", missing])
        assert out.returncode == 2 and "missing.iq" in out.stderr, (rate, khz, out.stderr)
        out = parity.run_cli(["-r", rate, "-c", "868250", "-p", "f=%d" % (868250 + khz), "-L", missing])
        assert out.returncode == 2 and "missing.iq" in out.stderr, (rate, khz, out.stderr)
    # at half the rate and beyond: refused, and the text names the rate
    for rate, khz in (("2400000", 1200), ("2400000", -1200), ("2048000", 1024), ("3200000", 1600), ("2400000", 5000)):
        out = parity.run_cli(["-r", rate, "-c", "868250", "-p", "f=%d" % (868250 + khz), "-L", missing])
        assert out.returncode == 1 and rate in out.stderr and "missing.iq" not in out.stderr, (rate, khz, out.stderr)
    # without -r the limit is what it was
    out = parity.run_cli(["-c", "868250", "-f", "869150", "-L", missing])
    assert out.returncode == 1 and "767 kHz" in out.stderr
    out = parity.run_cli(["-r", "2400000", "-x", "-f", "869150", "-L", missing])
    assert out.returncode == 1 and "exclude" in out.stderr


# ---- the scenes
@pytest.mark.parametrize("p,q", sorted(WIDE_SCENES))
def test_every_burst_decodes_for_exactly_the_receiver_tuned_to_it(p, q):
    """Non-vacuity of test_input_tune_gpu.py, through the restatement and the oracle alone."""
    x = wide_row(p, q)[0]
    freqs = WIDE_SCENES[p, q]
    assert freqs[0] == 0 and any(0 < abs(f) < 768000 for f in freqs) and any(abs(f) > 768000 for f in freqs)
    for j, f in enumerate(freqs):
        assert parity.decoded(input_oracle(x, p, q, f)) == [j], (j, f)
        if abs(f) < 768000:  # within the narrow tune's reach both tunes decode it
            assert parity.decoded(input_oracle(x, p, q, 0, f)) == [j], (j, f)
        else:
            # the tune behind the resampler does not reach it: neither as near as that tune gets, nor at the frequency the
            # burst would alias to at 1.536 MS/s -- the resampler's low-pass has removed it
            edge = 767999 if f > 0 else -767999
            alias = f - 1536000 if f > 0 else f + 1536000
            assert abs(alias) < 768000
            for hz in (edge, alias):
                assert j not in parity.decoded(input_oracle(x, p, q, 0, hz)), (j, f, hz)
