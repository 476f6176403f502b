"""The IQ balancer without a GPU (tfrec_amd_create_iq, tfrec_gpu -Z): the restatement tfrec_amd/iqbal.py against a
per-sample form of the definition, the raw-sum identities, every guard, the roundings and the square root at their edges, its
behaviour under cutting, the ghost telegrams of an impaired recording behind the oracle, the exports and what tfrec_gpu decides
before it opens a device.

Everything but the FFT of the tone test is an exact integer; nothing here has a tolerance."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import parity
from meter_rows import GHOST_FREQS, IDENT, THRESH, TYPES, ghost_oracles, guard_rows, impair
from tfrec_amd import api, dcblock, formats, iqbal

L = iqbal.L


def noisy_row(fmt, n, seed, dc=(300, -170), gain=1.1, deg=5.0, rails=True):
    """[bytes] of n complex samples in the format: impaired noise around a DC offset (in x), with stretches at both rails."""
    rng = np.random.default_rng(seed)
    x = rng.integers(-2500, 2500, (n, 2))
    x[n // 3:n // 3 + 700] = rng.integers(-8192, 8192, (700, 2))
    x = impair(np.clip(x, -8192, 8191).astype(np.int16).reshape(-1), gain, deg).reshape(-1, 2).astype(np.int64) + np.asarray(dc)
    if rails:  # (both rails alike: that window's estimate is refused, and every sum it is part of)
        x[n // 2:n // 2 + 40] = 8191
        x[n // 2 + 40:n // 2 + 80] = -8192
    x = np.clip(x, -8192, 8191)
    if fmt in ("u8", "s8"):
        x &= ~63
    return formats.encode(fmt, x.astype(np.int16).reshape(-1))


# ---- the vectorised form equals the per-sample one
@pytest.mark.parametrize("fmt", ["u8", "s8", "s16", "f32"])
def test_iq_balance_equals_the_per_sample_form(fmt):
    n_win, cut = 10, 4
    raw = noisy_row(fmt, n_win * L, 5)
    bps = formats.bytes_per_sample(fmt)
    seen = set()
    for k_dc in (0, 4, 64):
        for k_iq in (1, 3, 64, 100, 4096):
            got = iqbal.iq_balance(raw, fmt, k_dc, k_iq)
            want = iqbal.iq_balance_bruteforce(raw, fmt, k_dc, k_iq)
            for g, w in zip(got[:3], want[:3]):
                assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (fmt, k_dc, k_iq)
            assert got[3][1][1] == n_win and len(got[3][1][0]) == min(n_win, k_iq)
            # ... and carried over a cut, both forms from the vectorised form's state and from their own
            a = iqbal.iq_balance(raw[:cut * L * bps], fmt, k_dc, k_iq)
            b = iqbal.iq_balance(raw[cut * L * bps:], fmt, k_dc, k_iq, a[3])
            aa = iqbal.iq_balance_bruteforce(raw[:cut * L * bps], fmt, k_dc, k_iq)
            bb = iqbal.iq_balance_bruteforce(raw[cut * L * bps:], fmt, k_dc, k_iq, aa[3])
            for i in range(3):
                assert np.array_equal(np.concatenate([a[i], b[i]]), want[i]) and np.array_equal(np.concatenate([aa[i], bb[i]]), want[i])
            seen.update(map(tuple, want[2].tolist()))
            if k_dc == 0:
                assert not want[1].any()
    assert len(seen) > 5 and IDENT in seen  # (estimates that move; the window of the rails' stretch is refused)


RATES = [(1, 1, 1), (4, 3, 3), (25, 16, 1)]  # p, q, the blocks of a unit


@pytest.mark.parametrize("p,q,unit", RATES, ids=["%d/%d" % r[:2] for r in RATES])
def test_results_do_not_depend_on_the_cut(p, q, unit):
    n = dcblock.input_samples(4 * unit, p, q)
    raw = noisy_row("s16", n, 11 + p)
    for k_dc, k_iq in ((0, 3), (4, 64), (64, 100), (64, 4096), (4, 1)):
        whole = iqbal.iq_balance(raw, "s16", k_dc, k_iq)
        for sizes in ((1, 3), (2, 2), (1, 1, 1, 1)):
            pos, st, parts = 0, None, []
            for nb in sizes:
                m = dcblock.input_samples(nb * unit, p, q) * 4
                parts.append(iqbal.iq_balance(raw[pos:pos + m], "s16", k_dc, k_iq, st))
                st = parts[-1][3]
                pos += m
            assert pos == len(raw)
            for i in range(3):
                assert np.array_equal(np.concatenate([pt[i] for pt in parts]), whole[i]), (k_dc, k_iq, sizes, i)
            assert st[1][1] == whole[3][1][1] == n // L and np.array_equal(st[1][0], whole[3][1][0])


def test_a_reset_between_submits_starts_the_row_again():
    raw = noisy_row("s16", 8 * L, 2, rails=False)
    a = iqbal.iq_balance(raw[:4 * L * 4], "s16", 4, 64)
    b = iqbal.iq_balance(raw[4 * L * 4:], "s16", 4, 64, (a[3][0], None))  # the balancer's state alone
    fresh = iqbal.estimate(iqbal.moments(formats.to_x("s16", raw[4 * L * 4:]), b[1]), 64)[0]
    assert np.array_equal(b[2], fresh)
    assert not np.array_equal(b[2], iqbal.iq_balance(raw[4 * L * 4:], "s16", 4, 64, a[3])[2])


# ---- the moments follow from five raw sums
def test_raw_sum_identities_hold_where_the_clamp_acts():
    """A row that jumps from -8192 to 8191 under a long DC average: x - d leaves the rails (the apply clamps it), the moments are
    those of the unclamped difference."""
    n_win = 8
    x = np.full((n_win * L, 2), -8192, dtype=np.int16)
    x[5 * L + 100:] = 8191
    x[:, 1] = -x[:, 1] - 1
    x[::7, 0] += 500
    x = x.reshape(-1)
    d, _ = dcblock.estimate(dcblock.window_sums(x), 64)
    u = x.reshape(-1, L, 2).astype(np.int64) - d.reshape(-1, 1, 2).astype(np.int64)
    assert u.max() > 8191 and u.min() < -8192 and np.abs(u).max() <= 16383
    direct = np.stack([(u[:, :, 0] ** 2).sum(axis=1), (u[:, :, 1] ** 2).sum(axis=1), (u[:, :, 0] * u[:, :, 1]).sum(axis=1)], axis=1)
    assert np.array_equal(iqbal.moments(x, d), direct)
    assert direct.max() < 1 << 37 and direct[:, 2].min() < 0
    s5 = iqbal.raw_sums(x)
    assert np.array_equal(s5[:, :2], dcblock.window_sums(x)) and np.array_equal(iqbal.moments_of_sums(s5, np.zeros_like(d)), s5[:, [2, 3, 4]])
    xp = dcblock.apply(x, d)
    assert not np.array_equal(xp.astype(np.int64), u.reshape(-1))  # (the clamp acted)


# ---- the guards
def unguarded(sa, sb, sc):
    """(a, D, t, g) of the definition before the guards, in Python integers (t, g None where they do not exist)."""
    s = max(0, max(sa, sb).bit_length() - 31)
    a, b, c = sa >> s, sb >> s, sc >> s
    dd = a * b - c * c
    if a == 0 or dd <= 0:
        return a, dd, None, None
    r = math.isqrt(dd)
    return a, dd, (c * 32768 + a) // (2 * a), (a * 32768 + r) // (2 * r)


def test_each_guard_is_tripped_by_its_row():
    rows = guard_rows()
    for name, x in rows.items():
        m = iqbal.moments(x, np.zeros((4, 2), dtype=np.int16))
        tg, _ = iqbal.estimate(m, 4)
        a, dd, t, g = unguarded(*m.sum(axis=0).tolist())
        if name == "silence":
            assert a == 0
        elif name == "correlated":
            assert a > 0 and dd == 0
        elif name == "t":
            assert dd > 0 and abs(t) > 4096 and abs(t - 8192) < 200
        elif name == "g":
            assert dd > 0 and abs(t) <= 4096 and g < 12288
        if name == "fine":
            assert dd > 0 and tuple(tg[-1]) == (t, g) != IDENT
        else:
            assert (tg == IDENT).all(), name
            assert np.array_equal(iqbal.apply(x, tg), x)  # the identity passes the row through
    assert iqbal.tg_of(1 << 20, 1 << 18, 0) == IDENT and unguarded(1 << 20, 1 << 18, 0)[3] == 32768  # g too large
    assert iqbal.tg_of(1 << 20, 1 << 20, -(1 << 19)) == IDENT and unguarded(1 << 20, 1 << 20, -(1 << 19))[2] == -8192
    # the guards' edges are inside
    assert iqbal.tg_of(4 << 20, 4 << 20, 1 << 20)[0] == 4096 and iqbal.tg_of(4 << 20, 4 << 20, -(1 << 20))[0] == -4096
    assert iqbal.tg_of(16 << 20, 9 << 20, 0) == IDENT and iqbal.tg_of(9 << 20, 16 << 20, 0) == (0, 12288)
    assert unguarded(16 << 20, 9 << 20, 0)[3] == 21845 and iqbal.tg_of(25 << 20, 16 << 20, 0) == (0, 20480)


def test_t_floors_a_negative_numerator():
    """SC < 0 and 2 a does not divide c 32768 + a: floor, where C's division would truncate towards zero."""
    for sa, sc in ((1000, -3), (1000, -1), (999, -7), (1 << 30, -123457)):
        num, den = sc * 32768 + sa, 2 * sa
        assert num < 0 and num % den != 0
        t, g = iqbal.tg_of(sa, sa, sc)
        assert t == -((-num + den - 1) // den) == int(math.trunc(num / den)) - 1 and g != 0
    assert iqbal.tg_of(1000, 1000, -3) == (-49, 16400)


def test_the_shift_acts_on_full_scale_rows_at_4096_windows():
    full = (512 * 16383 * 16383, 512 * 16383 * 16382, -512 * 16383 * 16383 // 9)  # (|u| <= 16383)
    m = np.tile(np.array(full, dtype=np.int64), (4100, 1))
    m[::3, 2] += 12345  # (so that the shifted c differs from a multiple)
    tg, st = iqbal.estimate(m, 4096)
    sa, sb, sc = (int(v) for v in m[4:4100].sum(axis=0))
    assert sa.bit_length() == 49 and len(st[0]) == 4096 and st[1] == 4100
    s = sa.bit_length() - 31
    a, b, c = sa >> s, sb >> s, -((-sc + (1 << s) - 1) >> s)  # floor of a negative: written as a ceiling of the magnitude
    r = math.isqrt(a * b - c * c)
    assert a < 1 << 31 and (-sc) % (1 << s) != 0
    assert tuple(tg[-1]) == (-((-(c * 32768 + a) + 2 * a - 1) // (2 * a)), (a * 32768 + r) // (2 * r)) != IDENT
    # ... and on one window of a real full-scale row
    x = np.empty((L, 2), dtype=np.int16)
    x[:, 0] = np.where(np.arange(L) % 2, 8191, -8192)
    x[:, 1] = np.where(np.arange(L) % 4 < 2, 8191, -8192)
    raw = formats.encode("s16", x.reshape(-1))
    got, want = iqbal.iq_balance(raw, "s16", 0, 4096), iqbal.iq_balance_bruteforce(raw, "s16", 0, 4096)
    assert int(iqbal.moments(x.reshape(-1), np.zeros((1, 2)))[0, 0]).bit_length() > 31
    assert np.array_equal(got[2], want[2]) and np.array_equal(got[0], want[0])


def test_isqrt_is_the_exact_floor_around_every_perfect_square():
    rng = np.random.default_rng(1)
    ks = {0, 1, 2, 3, (1 << 31) - 1, (1 << 31) - 2, 94906265, 94906266, 94906267, 3037000499 % (1 << 31)}  # (94906266^2 ~ 2^53)
    for j in range(1, 31):
        ks.update((1 << j, (1 << j) - 1, (1 << j) + 1))
    ks.update(int(v) for v in rng.integers(1, 1 << 31, 400))
    ks.update(int(v) for v in rng.integers(1 << 30, 1 << 31, 400))
    for k in sorted(ks):
        for d in (k * k - 1, k * k, k * k + 1):
            if 0 <= d < 1 << 62:
                assert iqbal.isqrt(d) == math.isqrt(d), d
    assert iqbal.isqrt((1 << 62) - 1) == (1 << 31) - 1


# ---- tones
def tone(n, cycles_per_window, amp=4000):
    ph = 2 * np.pi * cycles_per_window * np.arange(n) / L
    return np.stack([np.rint(amp * np.cos(ph)), np.rint(amp * np.sin(ph))], axis=1).astype(np.int16).reshape(-1)


def test_a_balanced_tone_ends_at_exactly_the_identity():
    x = tone(80 * L, 37)
    for k in (1, 64):
        tg = iqbal.iq_balance(formats.encode("s16", x), "s16", 0, k)[2]
        assert tuple(tg[-1]) == IDENT and (tg[k:] == IDENT).all()


@pytest.mark.parametrize("gain,deg", [(1.12, 8.0), (1.06, 3.0), (0.9, -6.0)])
def test_the_image_of_an_impaired_tone_falls(gain, deg):
    n, cyc, k = 80 * L, 37, 64
    x = impair(tone(n, cyc), gain, deg)
    y = iqbal.iq_balance(formats.encode("s16", x), "s16", 0, k)[0]

    def image_dbc(v):  # the last window: a whole number of cycles, no leakage
        z = v.reshape(-1, 2)[-L:].astype(np.float64)
        f = np.abs(np.fft.fft(z[:, 0] + 1j * z[:, 1]))
        return 20 * np.log10(max(f[L - cyc], 1e-9) / f[cyc])

    before, after = image_dbc(x), image_dbc(y)
    print("image at %.2f / %g deg: %.1f dBc before, %.1f dBc behind the balancer" % (gain, deg, before, after))
    assert after < before


# ---- the ghost telegrams
def test_every_image_decodes_as_a_ghost_and_none_behind_the_balancer():
    raw_t = [parity.decoded(o) for o in ghost_oracles(False)]
    bal_t = [parity.decoded(o) for o in ghost_oracles(True)]
    for j in range(len(GHOST_FREQS)):
        assert raw_t[2 * j] == [j] and bal_t[2 * j] == [j], j          # the burst, raw and balanced
        assert raw_t[2 * j + 1] == [j], "no ghost of burst %d" % j      # its mirror: the same protocol again
        assert bal_t[2 * j + 1] == [], "burst %d's ghost survives" % j  # ... and nothing behind the balancer


# ---- the library and the binding
NAMES = ("tfrec_amd_create_iq", "tfrec_amd_get_iq", "tfrec_amd_read_iq", "tfrec_amd_reset_iq_rows")


def test_the_library_exports_the_four_symbols():
    Lb = api.load_library()
    for n in NAMES:
        assert n in api.EXPORTS and getattr(Lb, n) is not None
    hdr = open(os.path.join(parity.ROOT, "include", "tfrec_amd.h")).read()
    for n in NAMES[1:]:  # struct-free signatures: integers and pointers to integers only
        decl = hdr[hdr.index("int %s(" % n):]
        decl = decl[:decl.index(";")]
        assert "struct" not in decl and decl.count("tfrec_amd_") == 2, decl
    for n in ("iq", "read_iq", "reset_iq_rows"):
        assert callable(getattr(api.Receiver, n))
    h = C.c_void_p()
    k, rows, nw = C.c_int32(7), C.c_int32(7), C.c_int(7)
    cfg = api.Config(2, 0x2F, 500, 0, 0, 1, 4096, 0)
    assert Lb.tfrec_amd_create_iq(None, 0, 1, 1, 0, 64, 1, C.byref(h)) == api.E_INVAL
    assert Lb.tfrec_amd_create_iq(C.byref(cfg), 0, 1, 1, 0, 64, 1, None) == api.E_INVAL
    assert Lb.tfrec_amd_get_iq(None, C.byref(k), C.byref(rows)) == api.E_INVAL
    assert Lb.tfrec_amd_read_iq(None, 0, None, 0, C.byref(nw)) == api.E_INVAL
    assert Lb.tfrec_amd_reset_iq_rows(None, None, 0) == api.E_INVAL
    # argument errors that need no device: checked before one is looked for
    for fmt, p, q, kd, ki, rr in ((4, 1, 1, 0, 64, 1), (-1, 1, 1, 0, 64, 1), (0, 1, 1, -1, 64, 1), (0, 1, 1, 4097, 64, 1), (0, 1, 1, 0, 0, 1),
                                  (0, 1, 1, 4, 4097, 1), (0, 1, 1, 0, 64, 0), (0, 1, 1, 0, 64, 3), (0, 1, 2, 0, 64, 1), (2, 100, 1, 4, 64, 1)):
        assert Lb.tfrec_amd_create_iq(C.byref(cfg), fmt, p, q, kd, ki, rr, C.byref(h)) == api.E_INVAL and not h, (fmt, p, q, kd, ki, rr)
    cfg.flags = api.F_INPUT_10X
    assert Lb.tfrec_amd_create_iq(C.byref(cfg), 0, 1, 1, 0, 64, 1, C.byref(h)) == api.E_INVAL and not h
    assert b"10:1" in Lb.tfrec_amd_last_error()
    for kw in (dict(iq_windows=2 ** 31), dict(iq_windows=64, input_format="x16"), dict(iq_windows=64, decimated=True)):
        with pytest.raises(api.TfrecAmdError) as e:
            api.Receiver(2, TYPES, THRESH, 0, max_blocks=1, **kw)
        assert e.value.code == api.E_INVAL, kw


def test_k_outside_its_range_is_refused():
    for k in (0, -1, 4097):
        with pytest.raises(ValueError):
            iqbal.estimate(np.zeros((1, 3), dtype=np.int64), k)
        with pytest.raises(ValueError):
            iqbal.iq_balance_bruteforce(np.zeros(4 * L, dtype=np.uint8), "s16", 0, k)


# ---- tfrec_gpu -Z: what is decided before a device is opened
@pytest.fixture(scope="module")
def cli():
    return parity.build_cli()


def test_cli_usage_errors(cli, tmp_path):
    f = str(tmp_path / "missing.iq")
    for extra in (["-x"], ["-X", f]):
        out = parity.run_cli(["-Z", "-L", f] + extra)
        assert out.returncode == 1 and "-Z removes the IQ imbalance" in out.stderr, extra
    out = parity.run_cli(["-Z", "-R", str(tmp_path / "cap")])
    assert out.returncode == 2 and "-Z" in out.stderr
    for bad in ("0", "4097", "64x", "9999999999"):
        for args in (["-Z", bad], ["-Z" + bad]):
            out = parity.run_cli(args + ["-L", f])
            assert out.returncode == 1 and "bad -Z" in out.stderr, args
    for args in (["-Z"], ["-Z", "1"], ["-Z4096"], ["-Z", "-z"], ["-z", "64", "-Z", "100"], ["-Z", "-r", "2048000", "-F", "s16"],
                 ["-Z", "64", "-c", "868250", "-f", "868300"], ["-Z", "-p", "t=300"], ["-Z", "-s", "50"], ["-Z", "-S", str(tmp_path / "cap")],
                 ["-Z", "-P", "256"], ["-Z", "-A"], ["-Z", "-n", "1"], ["-D", "-Z", "2048"]):
        out = parity.run_cli(args + ["-L", f])  # accepted: the file is looked for
        assert out.returncode == 2 and "missing.iq" in out.stderr, args
    out = parity.run_cli(["-h"])
    assert out.returncode == 0 and "-Z [n]" in out.stderr and "-z [n]" in out.stderr
