"""The whole-kHz rates of the resampling stage (Q <= 64 or Q | 1536) without a GPU: the library's tap tables against
the restatement tfrec_amd/resample.py at the new denominators, the figures the kernels' bounds rest on over all 12 960 new rates,
the rates that stay refused, the block rule unit(Q) = Q / gcd(Q, 64), the input-rate tune's increment where its numerator leaves
64 bits, tfrec_gpu -r's argument handling, and what the rates, rows and scenes of the GPU tests (input_rows.py's KHZ_SWEEP and
khz_scene) are there for.

Everything is bit-exact; nothing here has a tolerance."""
import math
from concurrent.futures import ThreadPoolExecutor
from fractions import Fraction

import numpy as np
import pytest

import parity
from input_rows import KHZ_SCENE_RATES, KHZ_SWEEP, KHZ_SWEEP_BY_RATE, khz_scene, khz_sweep_rows, khz_sweep_stage0, khz_sweep_tunes, oracle_of
from tfrec_amd import api, resample, tune

NEW_Q = (96, 128, 192, 256, 384, 512, 768, 1536)  # the divisors of 1536 above 64
# 2.0, 2.5, 5, 10, 12.5 and 2.205 MS/s; the smallest rate of Q = 128, 768 and 1536; the largest rate of all
NAMED = [(125, 96), (625, 384), (625, 192), (625, 96), (3125, 384), (735, 512), (129, 128), (769, 768), (1537, 1536), (15359, 1536)]
UNITS = {96: 3, 128: 2, 192: 3, 256: 4, 384: 6, 512: 8, 768: 12, 1536: 24}


def new_rates():
    return [(p, q) for q in NEW_Q for p in range(q + 1, 10 * q) if math.gcd(p, q) == 1]


def library_taps(p, q):
    """The library's table in one call (api.resample_taps asks for T first: twice the work), or None where it refuses."""
    L = api.load_library()
    t = resample.n_taps(p, q)
    out = np.empty((q, t), dtype=np.int32)
    got = api.C.c_int(0)
    rc = L.tfrec_amd_resample_taps(p, q, out.ctypes.data, out.size, api.C.byref(got))
    if rc != api.E_OK:
        assert rc == api.E_INVAL, (p, q, rc)
        return None
    assert got.value == t, (p, q)
    return out


# ---- the tables
def test_the_new_denominators_are_the_whole_khz_rates():
    assert [q for q in range(65, 1537) if 1536 % q == 0] == list(NEW_Q) and resample.Q_MAX == 64 and resample.Q_DIV == 1536
    assert len(new_rates()) == 12960
    for hz in range(1537000, 15360000, 1000):
        p, q = resample.reduce_rate(hz)
        assert 1536 % q == 0 and q < p < 10 * q, hz
        assert resample.n_taps(p, q) <= 60
    assert [resample.reduce_rate(hz) for hz in (2000000, 2500000, 5000000, 10000000, 12500000, 2205000)] == NAMED[:6]


def test_library_taps_equal_the_restatement_at_the_named_rates_and_a_sample():
    rng = np.random.default_rng(1536)
    rates = new_rates()
    sample = [rates[i] for i in rng.choice(len(rates), 150, replace=False)]
    for p, q in NAMED + sample:
        want = resample.taps(p, q)
        got = api.resample_taps(p, q)
        assert got.dtype == np.int32 and got.shape == want.shape == (q, resample.n_taps(p, q)), (p, q)
        assert np.array_equal(got, want), "%d/%d: first differing (phase, tap) %s" % (p, q, np.argwhere(got != want)[0].tolist())
        assert (want.astype(np.int64).sum(axis=1) == 65536).all(), (p, q)


def test_every_new_rate_is_accepted_and_within_the_bounds():
    """The library alone over all 12 960 (the restatement's scalar definition takes ten minutes of CPU for them; its figures, from
    the run DESIGN.md 6f records, are the expectations here): none refused, the largest sum |h| 108260 at exactly 769/768 and
    1537/1536, the largest |h| 65497 -- so h / 65536 is exact in fp32 and neither int16 guard comes near."""
    def figures(rate):
        h = library_taps(*rate)
        assert h is not None, rate
        a = np.abs(h.astype(np.int64))
        return int(a.sum(axis=1).max()), int(a.max())

    rates = new_rates()
    with ThreadPoolExecutor(8) as ex:  # (the library call releases the GIL; its error text is per thread)
        fig = list(ex.map(figures, rates))
    worst = max(f[0] for f in fig)
    assert worst == 108260 and {r for r, f in zip(rates, fig) if f[0] == worst} == {(769, 768), (1537, 1536)}
    assert max(f[1] for f in fig) == 65497 < 1 << 17
    assert (worst * 8192) >> 16 == 13532 and (worst * 11585) >> 16 == 19137


@pytest.mark.parametrize("p,q", [(97, 80), (1025, 1024), (3073, 3072), (125, 192), (961, 96), (250, 192)])
def test_still_refused(p, q):
    """Bad denominators, one beyond 1536, a rate below 1 and one above 10, and a pair not in lowest terms."""
    with pytest.raises(resample.RateError):
        resample.taps(p, q)
    with pytest.raises(api.TfrecAmdError) as e:
        api.resample_taps(p, q)
    assert e.value.code == api.E_INVAL


# ---- the block rule
def test_permitted_blocks_is_q_over_gcd_q_64():
    for q in range(1, 65):
        odd = q
        while odd % 2 == 0:
            odd //= 2
        assert resample.permitted_blocks(q) == odd, q
    assert {q: resample.permitted_blocks(q) for q in NEW_Q} == UNITS
    for p, q in NAMED:
        unit = resample.permitted_blocks(q)
        n = resample.input_samples(unit, p, q)
        assert n % 512 == 0 and n * q == unit * 32768 * p, (p, q)
        assert unit > 1
        with pytest.raises(resample.RateError):
            resample.input_samples(unit + 1, p, q)
    with pytest.raises(resample.RateError):  # 33024 samples: whole, but 64.5 windows of 512
        resample.input_samples(1, 129, 128)
    assert 32768 * 129 % 128 == 0 and 32768 * 129 // 128 % 512 == 256


# ---- the input-rate tune where tune_hz * 2^33 * Q leaves 63 bits
@pytest.mark.parametrize("p,q,hz", [(15359, 1536, 699051), (15359, 1536, 7000001), (15359, 1536, 7679499), (3125, 384, 6249999)])
def test_inc_in_against_big_integers(p, q, hz):
    for v in (hz, -hz):
        want = math.floor(Fraction(v * q, 1536000 * p) * 2 ** 32 + Fraction(1, 2)) % 2 ** 32  # round(v / fs_in * 2^32), halves up
        assert tune.inc_in(v, p, q) == want
    assert abs(hz) * 2 ** 33 * q >= 2 ** 63  # (the case is here because an int64 numerator would have wrapped)
    with pytest.raises(ValueError):
        tune.inc_in((1536000 * p + 2 * q - 1) // (2 * q), p, q)


# ---- tfrec_gpu -r: what is decided before a device is opened
@pytest.fixture(scope="module")
def cli():
    return parity.build_cli()


def test_cli_takes_the_whole_khz_rates(cli, tmp_path):
    missing = str(tmp_path / "missing.iq")
    for hz in ("2000000", "2500000", "10000000", "12500000", "1537000"):
        out = parity.run_cli(["-r", hz, "-L", missing])
        assert out.returncode == 2 and "missing.iq" in out.stderr and "does not take" not in out.stderr, (hz, out.stderr)
    out = parity.run_cli(["-r", "2500000", "-b", "4", "-L", missing])  # 625/384: multiples of 6
    assert out.returncode == 2 and "-b 4 rounded up to 6" in out.stderr
    out = parity.run_cli(["-r", "1548000", "-b", "1", "-L", missing])  # 129/128: multiples of 2, not of the odd part
    assert out.returncode == 2 and "-b 1 rounded up to 2" in out.stderr
    out = parity.run_cli(["-r", "1537500", "-L", missing])  # 1025/1024
    assert out.returncode == 1 and "does not take" in out.stderr


# ---- what the GPU tests run (test_khz_rates_gpu.py)
STAGED_MAX = 3840  # csrc/tfrec_dev.h: kRsTableMax


def test_sweep_rates_are_what_they_are_there_for():
    for p, q, n, sizes, fmts, tuned_fmt in KHZ_SWEEP:
        unit = resample.permitted_blocks(q)
        assert sizes == ((unit, 2 * unit, unit) if q != 1536 else (24, 24)) and all(nb % unit == 0 for nb in sizes)
        assert tuned_fmt in fmts and fmts[0] == "u8" and n == (2 if p == 15359 else 3)
        for fmt in ("u8", tuned_fmt):
            for hz in khz_sweep_tunes(p, q, fmt):
                tune.inc_in(hz, p, q)  # (inside half the input rate)
    t = {r[:2]: resample.n_taps(*r[:2]) for r in KHZ_SWEEP}
    assert [t[r[:2]] for r in KHZ_SWEEP] == [8, 10, 8, 50, 10, 8, 60]
    table = {r: r[1] * t[r] for r in t}
    assert table[125, 96] == 768 and table[625, 384] == STAGED_MAX == 64 * 60 and table[129, 128] == 1024
    assert table[3125, 384] == 19200 and table[735, 512] == 5120 and table[1537, 1536] == 12288 and table[15359, 1536] == 92160
    assert all(q * resample.n_taps(p, q) <= STAGED_MAX for p, q in NAMED[:4])  # 2.0, 2.5, 5 and 10 MS/s run the staged kernels
    assert max(r[0] for r in new_rates()) == 15359 and resample.permitted_blocks(128) == 2
    # the tunes that are there for the 128-bit numerator need it
    assert 7000001 * 2 ** 33 * 1536 >= 2 ** 63 and 699051 * 2 ** 33 * 1536 >= 2 ** 63 > 699050 * 2 ** 33 * 1536
    assert 6249999 * 2 ** 33 * 384 >= 2 ** 63


@pytest.mark.parametrize("p,q", [(129, 128), (3125, 384)])
def test_cutting_at_the_unit_reproduces_the_stream(p, q):
    """What the GPU sweep expects is consistent in itself: the u8 row cut into its submits, each from the T - 1 raw samples before
    it, is the uncut stream."""
    t = resample.n_taps(p, q)
    u8 = khz_sweep_rows("u8", p, q)[0]
    parts, pos = [], 0
    for nb in KHZ_SWEEP_BY_RATE[p, q][3]:
        n = 2 * resample.input_samples(nb, p, q)
        parts.append(resample.resample_s16(u8[pos:pos + n], p, q, hist=u8[pos - 2 * (t - 1):pos] if pos else None))
        pos += n
    assert pos == len(u8) and np.array_equal(np.concatenate(parts), khz_sweep_stage0("u8", p, q, False)[0])


@pytest.mark.parametrize("p,q", KHZ_SCENE_RATES)
def test_gpu_scenes_decode_every_protocol(p, q):
    """Non-vacuity of the end-to-end GPU test: the oracle alone, fed the restatement's stage 0 of the scene, yields a status-1
    telegram of every protocol at each rate, and at least one in every stream."""
    iq = khz_scene(p, q)
    seen = set()
    for s in range(len(iq)):
        ok = {e[0] for e in oracle_of(iq[s], p, q).events_full() if e[7] == 1}
        assert ok, s
        seen |= ok
    assert seen == {0, 1, 2, 3, 4}
