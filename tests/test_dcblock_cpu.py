"""The DC blocker without a GPU (tfrec_amd_create_dc, tfrec_gpu -z): the restatement tfrec_amd/dcblock.py against a
per-sample form of the definition, its rounding and clamping at their edges, its behaviour under cutting, the acceptance table of
the golden scenes behind the oracle, the exports and what tfrec_gpu decides before it opens a device.

Everything is an exact integer; nothing here has a tolerance."""
import ctypes as C
import os

import numpy as np
import pytest

import parity
from meter_rows import golden_scene, offset_scene
from oracle import oracle as O
from tfrec_amd import api, dcblock, formats

L = dcblock.L
SCENES = ("tfa_1", "tfa_2", "tfa_3", "tx22", "whb")


def noisy_rows(fmt, n, seed, dc=(300, -170)):
    """[bytes] of n complex samples in the format: noise around a DC offset (in x), with stretches at both rails."""
    rng = np.random.default_rng(seed)
    x = rng.integers(-900, 900, (n, 2)) + np.asarray(dc)
    x[n // 3:n // 3 + 700] = rng.integers(-8192, 8192, (700, 2))
    x[n // 2:n // 2 + 40] = 8191
    x[n // 2 + 40:n // 2 + 80] = -8192
    x = np.clip(x, -8192, 8191)
    if fmt in ("u8", "s8"):
        x &= ~63
    return formats.encode(fmt, x.astype(np.int16).reshape(-1))


# ---- the vectorised form equals the per-sample one
@pytest.mark.parametrize("fmt", ["u8", "s8", "s16", "f32"])
def test_dc_block_equals_the_per_sample_form(fmt):
    raw = noisy_rows(fmt, 12 * L, 3)
    bps = formats.bytes_per_sample(fmt)
    for k in (1, 4, 64, 4096):
        got = dcblock.dc_block(raw, fmt, k)
        want = dcblock.dc_block_bruteforce(raw, fmt, k)
        for g, w in zip(got[:2], want[:2]):
            assert g.dtype == w.dtype and np.array_equal(g, w), (fmt, k)
        assert np.array_equal(got[2][0], want[2][0]) and got[2][1] == want[2][1] == 12
        # ... and carried over a cut at window 5, a state of fewer than K and of K windows
        a = dcblock.dc_block(raw[:5 * L * bps], fmt, k)
        b = dcblock.dc_block(raw[5 * L * bps:], fmt, k, a[2])
        bb = dcblock.dc_block_bruteforce(raw[5 * L * bps:], fmt, k, a[2])
        assert np.array_equal(np.concatenate([a[0], b[0]]), want[0]) and np.array_equal(np.concatenate([a[1], b[1]]), want[1])
        assert np.array_equal(b[0], bb[0]) and np.array_equal(b[1], bb[1]) and np.array_equal(b[2][0], bb[2][0])
    assert np.abs(want[1]).max() > 100  # (K = 4096: the running mean sees the offset)


def test_f32_edge_values_go_through_to_x():
    v = np.zeros(2 * L, dtype="<f4")
    v[:8] = [np.nan, np.inf, -np.inf, 2.0, -2.0, 0.5 / 8192, 1.5 / 8192, -0.5 / 8192]
    x, d, _ = dcblock.dc_block(v.view(np.uint8), "f32", 1)
    xin = formats.to_x("f32", v.view(np.uint8))
    assert np.array_equal(d, dcblock.estimate(dcblock.window_sums(xin), 1)[0]) and np.array_equal(x, dcblock.apply(xin, d))


# ---- the estimate's rounding: floor, not truncation, and ties half up
def floor_div(num, den):
    q = abs(num) // den
    return q if num >= 0 else -q - (1 if abs(num) % den else 0)


def test_estimate_floors_negative_numerators_and_rounds_ties_up():
    cases = []
    for a in (-1, -255, -256, -257, -511, -512, -513, -767, -768, -769, -1023, -1025, 255, 256, 257, 767, 768, 769, -(1 << 22), (1 << 22) - 512):
        cases.append(a)
    s = np.array([[a, -a if abs(a) < 1 << 21 else 0] for a in cases], dtype=np.int64)  # (a window's sum lies within [-2^22, 8191 * 512])
    d, _ = dcblock.estimate(s, 1)  # K = 1: A = S[w], c = 1
    for (a, b), (di, dq) in zip(s.tolist(), d.tolist()):
        assert di == floor_div(2 * a + 512, 1024) and dq == floor_div(2 * b + 512, 1024), a
    byname = dict(zip(cases, d[:, 0].tolist()))
    # ties at exactly half: a mean of -0.5 is 0, of -1.5 is -1, of 0.5 is 1, of 1.5 is 2 (half up, not half away from zero)
    assert (byname[-256], byname[-768], byname[256], byname[768]) == (0, -1, 1, 2)
    # where floor and C's truncation differ: a negative numerator that 1024 does not divide
    assert byname[-257] == -1 and int((2 * -257 + 512) / 1024) == 0
    assert byname[-769] == -2 and int((2 * -769 + 512) / 1024) == -1
    assert byname[-(1 << 22)] == -8192 and byname[(1 << 22) - 512] == 8191  # the range's ends
    # c > 1: two windows, K = 2: A = S[0] + S[1], 1024 c = 2048; a tie at c = 2 (A = -512: mean -0.5) and a negative remainder
    for a0, a1 in ((-300, -212), (-300, -213), (-1, 0), (-1023, -1), (700, -1212)):
        d, _ = dcblock.estimate(np.array([[a0, 0], [a1, 0]], dtype=np.int64), 2)
        assert d[1, 0] == floor_div(2 * (a0 + a1) + 1024, 2048) and d[0, 0] == floor_div(2 * a0 + 512, 1024)
    assert dcblock.estimate(np.array([[-300, 0], [-212, 0]]), 2)[0][1, 0] == 0


def test_apply_clamps_at_both_edges():
    x = np.zeros((2 * L, 2), dtype=np.int16)
    x[:L, 0], x[:L, 1] = 8191, -8192
    x[L:, 0], x[L:, 1] = -8192, 8191
    x[5], x[L + 5] = (8191, 8191), (-8192, -8192)
    d = np.array([[-3, 7], [9, -2]], dtype=np.int16)
    y = dcblock.apply(x.reshape(-1), d).reshape(-1, 2)
    assert y[0].tolist() == [8191, -8192] and y[5].tolist() == [8191, 8184]  # 8191 + 3 and -8192 - 7 clamp
    assert y[L].tolist() == [-8192, 8191] and y[L + 5].tolist() == [-8192, -8190]
    # a full-scale constant row is its own offset: x' = 0 but for nothing
    raw = formats.encode("s16", np.full(2 * 3 * L, -8192, dtype=np.int16))
    y, d, _ = dcblock.dc_block(raw, "s16", 4)
    assert (d == -8192).all() and not y.any()
    raw = formats.encode("s16", np.full(2 * 3 * L, 8191, dtype=np.int16))
    y, d, _ = dcblock.dc_block(raw, "s16", 4)
    assert (d == 8191).all() and not y.any()


def test_k_outside_its_range_is_refused():
    for k in (0, -1, 4097):
        with pytest.raises(ValueError):
            dcblock.estimate(np.zeros((1, 2)), k)


# ---- cutting
def run_cut(raw, fmt, k, sizes, p=1, q=1, reset_before=()):
    """dc_block over submits of sizes[i] blocks at the rate, the state carried; a DC reset ahead of the listed submits."""
    bps = formats.bytes_per_sample(fmt)
    pos, st, xs, ds = 0, None, [], []
    for i, nb in enumerate(sizes):
        n = dcblock.input_samples(nb, p, q) * bps
        if i in reset_before:
            st = None
        x, d, st = dcblock.dc_block(raw[pos:pos + n], fmt, k, st)
        xs.append(x)
        ds.append(d)
        pos += n
    assert pos == len(raw)
    return np.concatenate(xs), np.concatenate(ds), st


@pytest.mark.parametrize("k", [4, 63, 64, 100, 4096])
def test_results_do_not_depend_on_the_cut(k):
    """4 blocks against 1 + 3 and 2 + 2: K below, at and above one block's 64 windows."""
    raw = noisy_rows("s16", 4 * 32768, 11)
    whole = run_cut(raw, "s16", k, (4,))
    for sizes in ((1, 3), (2, 2), (1, 1, 1, 1)):
        got = run_cut(raw, "s16", k, sizes)
        assert np.array_equal(got[0], whole[0]) and np.array_equal(got[1], whole[1]), sizes
        assert np.array_equal(got[2][0], whole[2][0]) and got[2][1] == whole[2][1] == 256


def test_a_dc_reset_between_submits_starts_the_row_again():
    raw = noisy_rows("u8", 4 * 32768, 12)
    got = run_cut(raw, "u8", 100, (2, 2), reset_before=(1,))
    first, second = dcblock.dc_block(raw[:len(raw) // 2], "u8", 100), dcblock.dc_block(raw[len(raw) // 2:], "u8", 100)
    assert np.array_equal(got[0], np.concatenate([first[0], second[0]])) and np.array_equal(got[1], np.concatenate([first[1], second[1]]))
    assert got[2][1] == 128
    assert not np.array_equal(got[1], run_cut(raw, "u8", 100, (2, 2))[1])


@pytest.mark.parametrize("p,q,sizes", [(4, 3, (3,)), (4, 3, (3, 3)), (25, 16, (1, 2)), (25, 16, (3,))])
def test_rate_submits_are_whole_windows(p, q, sizes):
    n = dcblock.input_samples(sum(sizes), p, q)
    assert all(dcblock.input_samples(nb, p, q) % L == 0 for nb in sizes)
    raw = noisy_rows("s16", n, 13)
    whole = dcblock.dc_block(raw, "s16", 70)
    got = run_cut(raw, "s16", 70, sizes, p, q)
    assert np.array_equal(got[0], whole[0]) and np.array_equal(got[1], whole[1])


def test_every_permitted_submit_of_every_q_is_whole_windows():
    """Q = 2^a o, o odd, 2^a <= 64: n_blocks is a multiple of o and 32768 / 2^a >= 512."""
    for q in range(1, 65):
        o = q
        while o % 2 == 0:
            o //= 2
        p = q + 1  # (any P coprime to Q: the argument does not depend on it)
        assert dcblock.input_samples(o, p, q) % L == 0 and (32768 // (q // o)) % L == 0


# ---- the acceptance table: the golden scenes with a DC offset, behind the oracle
@pytest.mark.parametrize("name", SCENES)
def test_offset_scenes_decode_behind_the_blocker_and_not_without(name):
    iq, clean = golden_scene(name)
    assert len(clean.splitlines()) >= 1
    off = offset_scene(name)
    o = O.Oracle(0x2F, 500)
    o.process(off)
    assert o.text() == ""  # pwr = |I| + |Q| stays above 500: no window ever closes
    for k in (64, 2048):
        x, d, _ = dcblock.dc_block(off, "u8", k)
        o = O.Oracle(0x2F, 500)
        o.process_s16(x)
        assert o.text() == clean, (name, k)
        x0, d0, _ = dcblock.dc_block(iq, "u8", k)  # ... and a scene without an offset is not harmed
        o = O.Oracle(0x2F, 500)
        o.process_s16(x0)
        assert o.text() == clean, (name, k, "no offset")


# ---- the library and the binding
def test_the_library_exports_the_four_symbols():
    names = ("tfrec_amd_create_dc", "tfrec_amd_get_dc", "tfrec_amd_read_dc", "tfrec_amd_reset_dc_rows")
    Lb = api.load_library()
    for n in names:
        assert n in api.EXPORTS and getattr(Lb, n) is not None
    hdr = open(os.path.join(parity.ROOT, "include", "tfrec_amd.h")).read()
    # struct-free signatures: integers and pointers to integers only
    for n in names[1:]:
        decl = hdr[hdr.index("int %s(" % n):]
        decl = decl[:decl.index(";")]
        assert "struct" not in decl and decl.count("tfrec_amd_") == 2, decl  # (the name and the context)
    h = C.c_void_p()
    k, rows, nw = C.c_int32(7), C.c_int32(7), C.c_int(7)
    assert Lb.tfrec_amd_create_dc(None, 0, 1, 1, 64, 1, C.byref(h)) == api.E_INVAL
    assert Lb.tfrec_amd_create_dc(C.byref(api.Config(1, 0x2F, 500, 0, 0, 1, 4096, 0)), 0, 1, 1, 64, 1, None) == api.E_INVAL
    assert Lb.tfrec_amd_get_dc(None, C.byref(k), C.byref(rows)) == api.E_INVAL
    assert Lb.tfrec_amd_read_dc(None, 0, None, 0, C.byref(nw)) == api.E_INVAL
    assert Lb.tfrec_amd_reset_dc_rows(None, None, 0) == api.E_INVAL
    # argument errors that need no device: checked before one is looked for
    cfg = api.Config(2, 0x2F, 500, 0, 0, 1, 4096, 0)
    for fmt, p, q, kk, rr in ((4, 1, 1, 64, 1), (-1, 1, 1, 64, 1), (0, 1, 1, 0, 1), (0, 1, 1, 4097, 1), (0, 1, 1, 64, 0), (0, 1, 1, 64, 3),
                              (0, 1, 2, 64, 1), (2, 100, 1, 64, 1)):
        assert Lb.tfrec_amd_create_dc(C.byref(cfg), fmt, p, q, kk, rr, C.byref(h)) == api.E_INVAL and not h, (fmt, p, q, kk, rr)
    cfg.flags = api.F_INPUT_10X
    assert Lb.tfrec_amd_create_dc(C.byref(cfg), 0, 1, 1, 64, 1, C.byref(h)) == api.E_INVAL and not h
    assert b"10:1" in Lb.tfrec_amd_last_error()


# ---- tfrec_gpu -z: what is decided before a device is opened
@pytest.fixture(scope="module")
def cli():
    return parity.build_cli()


def test_cli_usage_errors(cli, tmp_path):
    f = str(tmp_path / "missing.iq")
    for extra in (["-x"], ["-X", f]):
        out = parity.run_cli(["-z", "-L", f] + extra)
        assert out.returncode == 1 and "-z removes the DC offset" in out.stderr, extra
    for bad in ("0", "4097", "64x", "9999999999"):
        for args in (["-z", bad], ["-z" + bad]):
            out = parity.run_cli(args + ["-L", f])
            assert out.returncode == 1 and "bad -z" in out.stderr, args
    for args in (["-z"], ["-z", "1"], ["-z4096"], ["-z", "-r", "2048000", "-F", "s16"], ["-z", "64", "-c", "868250", "-f", "868300"],
                 ["-z", "-p", "t=300"], ["-z", "-s", "50"], ["-z", "-S", str(tmp_path / "cap")], ["-z", "-P", "256"], ["-z", "-A"],
                 ["-z", "-n", "1"], ["-D", "-z", "2048"]):
        out = parity.run_cli(args + ["-L", f])  # accepted: the file is looked for
        assert out.returncode == 2 and "missing.iq" in out.stderr, args
    out = parity.run_cli(["-h"])
    assert out.returncode == 0 and "-z [n]" in out.stderr
