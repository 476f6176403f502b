"""The resampling stage without a GPU: the library's tap tables against the restatement tfrec_amd/resample.py,
the properties of the definition, the scenes the GPU tests decode, and tfrec_gpu -r's argument handling.

Everything is bit-exact; nothing here has a tolerance."""
import numpy as np
import pytest

import parity
from input_rows import SCENE_RATES, oracle_of, rate_scene
from tfrec_amd import api, resample

RATES = [(4, 3), (25, 16), (5, 4), (5, 3), (15, 8), (25, 12), (2, 1), (4, 1), (75, 64)]


# ---- tap tables
@pytest.mark.parametrize("p,q", RATES)
def test_library_taps_equal_the_restatement(p, q):
    h = resample.taps(p, q)
    t = 2 * -(-3 * p // q)  # 2 ceil(3 r)
    assert h.shape == (q, t) and t % 2 == 0 and t <= 60
    got = api.resample_taps(p, q)
    assert got.dtype == np.int32 and got.shape == h.shape and np.array_equal(got, h)
    assert (h.sum(axis=1) == 65536).all()  # unity DC gain, every phase
    # the int16 store cannot wrap for u8 input, and h / 1024 is exact in fp32
    assert (int(np.abs(h).sum(axis=1).max()) * 8192) >> 16 < 32768 and np.abs(h).max() < 1 << 17


def test_taps_per_phase_of_the_common_rates():
    assert resample.n_taps(4, 3) == 8 and resample.n_taps(25, 16) == 10
    assert resample.reduce_rate(2048000) == (4, 3) and resample.reduce_rate(2400000) == (25, 16)
    assert resample.reduce_rate(1920000) == (5, 4) and resample.reduce_rate(3200000) == (25, 12)


@pytest.mark.parametrize("p,q", RATES)
def test_taps_are_even_in_the_tap_offset(p, q):
    """The window and the sinc are even in d = n - T/2 + 1 - phi/Q.  Phase 0 has d = n - T/2 + 1: taps n and T - 2 - n mirror
    each other (d = T/2, the last tap, has no partner).  A phase phi > 0 has the negated offsets of phase Q - phi, tap n
    against tap T - 1 - n there: d(phi, n) = -d(Q - phi, T - 1 - n).  (With T - 2 - n for every phase the offsets of phi > 0
    would differ by one sample: the tables are not equal there, and need not be.)  The residual correction goes to ONE tap:
    at phi = Q/2 the two centre taps (d = -1/2, +1/2) have the same v, the lower one takes the residual, and the pair may
    differ by exactly that residual; everywhere else the largest tap is unique and mirrors onto the largest tap."""
    h = resample.taps(p, q).astype(np.int64)
    t = h.shape[1]
    assert all(h[0, n] == h[0, t - 2 - n] for n in range(t - 1))
    for phi in range(1, q):
        a, b = h[phi], h[q - phi][::-1]
        if 2 * phi != q:
            assert np.array_equal(a, b), phi
        else:
            diff = np.nonzero(a != b)[0].tolist()
            assert diff in ([], [t // 2 - 1, t // 2]), phi
            assert abs(a[t // 2 - 1] - a[t // 2]) <= t // 2  # the residual: at most half a unit of rounding per tap


@pytest.mark.parametrize("p,q", [(1, 1), (10, 1), (3, 4), (130, 128), (8, 6), (0, 3), (4, 0), (-4, 3), (4, -3), (640, 64),
                                 (65, 65)])
def test_refused_rates(p, q):
    with pytest.raises(resample.RateError):
        resample.taps(p, q)
    with pytest.raises(api.TfrecAmdError) as e:
        api.resample_taps(p, q)
    assert e.value.code == api.E_INVAL


def test_taps_call_argument_errors():
    L = api.load_library()
    buf = np.zeros(3 * 8, dtype=np.int32)
    t = api.C.c_int(0)
    assert L.tfrec_amd_resample_taps(4, 3, buf.ctypes.data, 23, api.C.byref(t)) == api.E_INVAL  # cap too small
    assert not buf.any()
    assert L.tfrec_amd_resample_taps(4, 3, None, 5, None) == api.E_INVAL
    assert L.tfrec_amd_resample_taps(4, 3, None, 0, None) == api.E_OK
    assert L.tfrec_amd_resample_taps(4, 3, buf.ctypes.data, 24, None) == api.E_OK and buf.reshape(3, 8).sum(axis=1).tolist() == [65536] * 3


# ---- the restatement's properties
@pytest.mark.parametrize("p,q", [(4, 3), (25, 16), (75, 64), (4, 1)])
def test_constant_input_has_unity_gain_minus_the_floors(p, q):
    t = resample.n_taps(p, q)
    for c in (100, -128, 127, 0, -1):
        x = np.full(2 * 4000, c + 128, dtype=np.uint8)
        y = resample.resample_s16(x, p, q).astype(np.int64)
        first = -(-t * q // p)  # outputs from here on have i0 >= T: every tap sees the constant
        assert len(y) // 2 > first + 100
        steady = y[2 * first:]
        assert steady.max() <= c * 64 and steady.min() >= c * 64 - t, (c, steady.min(), steady.max())


@pytest.mark.parametrize("p,q,sizes", [(4, 3, (3, 6, 3)), (25, 16, (1, 2, 4, 5)), (5, 3, (3, 3)), (75, 64, (1, 1))])
def test_cutting_at_permitted_boundaries_reproduces_the_stream(p, q, sizes):
    nb = sum(sizes)
    rng = np.random.default_rng(7 * p + q)
    x = rng.integers(0, 256, 2 * resample.input_samples(nb, p, q), dtype=np.uint8)
    whole = resample.resample_s16(x, p, q)
    assert len(whole) == 2 * nb * 32768
    t = resample.n_taps(p, q)
    unit = resample.permitted_blocks(q)
    parts, pos = [], 0
    for k in sizes:
        assert k % unit == 0
        n = 2 * resample.input_samples(k, p, q)
        parts.append(resample.resample_s16(x[pos:pos + n], p, q, hist=x[pos - 2 * (t - 1):pos] if pos else None))
        pos += n
    assert np.array_equal(np.concatenate(parts), whole)
    if unit > 1:  # a block count that is no multiple of Q's odd part is no whole number of samples
        with pytest.raises(resample.RateError):
            resample.input_samples(unit + 1, p, q)


@pytest.mark.parametrize("p,q", SCENE_RATES)
def test_gpu_scenes_decode_every_protocol(p, q):
    """Non-vacuity of test_resample_gpu.py: the oracle alone, fed the restatement's stage 0 of the scene, yields a status-1
    telegram of every protocol of the mask at each rate (and at least four protocols in every stream)."""
    iq = rate_scene(p, q)
    seen = set()
    for s in range(len(iq)):
        o = oracle_of(iq[s], p, q)
        ok = {e[0] for e in o.events_full() if e[7] == 1}
        assert len(ok) >= 4, (s, ok)
        seen |= ok
    assert seen == {0, 1, 2, 3, 4}


# ---- tfrec_gpu -r: what is decided before a device is opened
@pytest.fixture(scope="module")
def cli():
    return parity.build_cli()


def test_cli_rate_argument_errors(cli, tmp_path):
    missing = str(tmp_path / "missing.iq")
    for bad in ("abc", "0", "-5", "2048000x", ""):
        out = parity.run_cli(["-r", bad, "-L", missing])
        assert out.returncode == 1 and "bad -r" in out.stderr, bad
    out = parity.run_cli(["-r", "2048000", "-x", "-L", missing])
    assert out.returncode == 1 and "exclude" in out.stderr
    # refused by the library's rules: below 1.536 MS/s, at 15.36 MS/s, a denominator above 64
    for hz in ("1000000", "15360000", "1536001", "20000000"):
        out = parity.run_cli(["-r", hz, "-L", missing])
        assert out.returncode == 1 and "does not take" in out.stderr, hz
    # 1536000 itself is the default input: no resampler, the file is looked for
    out = parity.run_cli(["-r", "1536000", "-L", missing])
    assert out.returncode == 2 and "missing.iq" in out.stderr


def test_cli_rounds_the_block_count_up(cli, tmp_path):
    missing = str(tmp_path / "missing.iq")
    # 2.048 MS/s = 4/3: multiples of 3 blocks; the run then ends at the missing file, before any device is opened
    out = parity.run_cli(["-r", "2048000", "-b", "16", "-L", missing])
    assert out.returncode == 2 and "-b 16 rounded up to 18" in out.stderr and "missing.iq" in out.stderr
    out = parity.run_cli(["-r", "2048000", "-b", "18", "-L", missing])
    assert out.returncode == 2 and "rounded" not in out.stderr
    # 2.4 MS/s = 25/16: Q is a power of two, any block count
    out = parity.run_cli(["-r", "2400000", "-b", "7", "-L", missing])
    assert out.returncode == 2 and "rounded" not in out.stderr
    # 3.2 MS/s = 25/12: multiples of 3 again
    out = parity.run_cli(["-r", "3200000", "-b", "1", "-L", missing])
    assert out.returncode == 2 and "-b 1 rounded up to 3" in out.stderr
