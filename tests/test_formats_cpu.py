"""Sample formats (tfrec_amd_create_format, tfrec_gpu -F) without a GPU: the restatement tfrec_amd/formats.py against
the definition's table at every boundary, the encoders, the argument errors the library and tfrec_gpu give before a device is
opened, tfrec_gpu's block-size arithmetic, and the scenes the GPU tests decode.

Everything is bit-exact; nothing here has a tolerance."""
import numpy as np
import pytest

import parity
from input_rows import KINDS, SCENE_STREAMS, THRESH, TYPES, scene, scene_oracle, scene_u8
from tfrec_amd import api, formats


def f32_bytes(values):
    return np.asarray(values, dtype="<f4").view(np.uint8)


# ---- to_x at every boundary
def test_bytes_per_sample_and_aliases():
    assert [formats.bytes_per_sample(f) for f in ("u8", "s8", "s16", "f32")] == [2, 2, 4, 8]
    assert [formats.bytes_per_sample(f) for f in (0, 1, 2, 3)] == [2, 2, 4, 8]
    assert [formats.FORMATS[a] for a in ("cu8", "cs8", "cs16", "cf32")] == [0, 1, 2, 3]
    with pytest.raises((KeyError, ValueError)):
        formats.bytes_per_sample("s24")
    with pytest.raises(ValueError):
        formats.to_x(4, np.zeros(8, dtype=np.uint8))


def test_u8_and_s8_over_all_bytes():
    b = np.arange(256, dtype=np.uint8)
    u = formats.to_x("u8", b)
    assert u.dtype == np.int16 and u.tolist() == [(v - 128) << 6 for v in range(256)]
    assert u.min() == -8192 and u.max() == 8128
    assert np.array_equal(formats.to_x("s8", b ^ 0x80), u)  # S8 of b ^ 0x80 is U8 of b
    assert formats.to_x("s8", np.array([0x80, 0xFF, 0, 1, 0x7F], dtype=np.uint8)).tolist() == [-8192, -64, 0, 64, 8128]


def test_s16_shift_floors():
    v = np.array([-32768, -32767, -5, -4, -3, -1, 0, 1, 3, 4, 32767], dtype="<i2")
    assert formats.to_x("s16", v.view(np.uint8)).tolist() == [-8192, -8192, -2, -1, -1, -1, 0, 0, 0, 1, 8191]
    every = np.arange(-32768, 32768, dtype=np.int32)
    got = formats.to_x("s16", every.astype("<i2").view(np.uint8)).astype(np.int32)
    assert np.array_equal(got, np.floor_divide(every, 4)) and got.min() == -8192 and got.max() == 8191


def test_f32_full_scale_clamps_and_nan():
    one = np.float32(0.99993896)  # 8191.5 / 8192 rounded to fp32: v is a tie or next to one, and rounds into the clamp
    assert formats.to_x("f32", f32_bytes([one, -one])).tolist() == [8191, -8192]
    assert formats.to_x("f32", f32_bytes([8191 / 8192, -8191 / 8192])).tolist() == [8191, -8191]
    assert formats.to_x("f32", f32_bytes([1.0, -1.0, 2.0, -2.0])).tolist() == [8191, -8192, 8191, -8192]
    assert formats.to_x("f32", f32_bytes([np.inf, -np.inf, np.nan, -np.nan])).tolist() == [8191, -8192, 0, 0]
    big = np.finfo(np.float32).max  # f * 8192 overflows fp32: clamps like inf
    assert formats.to_x("f32", f32_bytes([big, -big, 1e35, -1e35])).tolist() == [8191, -8192, 8191, -8192]
    assert formats.to_x("f32", f32_bytes([0.0, -0.0])).tolist() == [0, 0]


def test_f32_ties_go_to_even():
    k = np.array([0, 1, 2, 3, 100, 101, 8189, 8190, -1, -2, -3, -4, -101, -8191, -8192], dtype=np.int64)
    f = ((k + 0.5) / 8192.0).astype(np.float32)  # exact in fp32: (2 k + 1) * 2^-14
    assert np.array_equal(f.astype(np.float64) * 8192.0, k + 0.5)
    want = [0, 2, 2, 4, 100, 102, 8190, 8190, 0, -2, -2, -4, -100, -8190, -8192]
    assert formats.to_x("f32", f.view(np.uint8)).tolist() == want
    assert all(w % 2 == 0 for w in want)
    assert formats.to_x("f32", f32_bytes([8190.5 / 8192, 8191.5 / 8192, -8192.5 / 8192])).tolist() == [8190, 8191, -8192]


def test_f32_just_below_a_half_and_denormals():
    half = np.float32(0.5 / 8192.0)
    below = np.nextafter(half, np.float32(0.0))  # the largest float below 0.5 / 8192
    above = np.nextafter(half, np.float32(1.0))
    assert formats.to_x("f32", f32_bytes([below, half, above, -below, -half, -above])).tolist() == [0, 0, 1, 0, 0, -1]
    tiny = np.float32(1e-45)  # the smallest denormal
    den = np.nextafter(np.finfo(np.float32).tiny, np.float32(0.0))  # the largest one
    assert tiny > 0 and den < np.finfo(np.float32).tiny
    assert formats.to_x("f32", f32_bytes([tiny, -tiny, den, -den])).tolist() == [0, 0, 0, 0]


def test_encode_round_trips_through_to_x():
    x = np.arange(-8192, 8192, dtype=np.int16)
    for fmt in ("s16", "f32"):
        raw = formats.encode(fmt, x)
        assert raw.dtype == np.uint8 and len(raw) == len(x) * formats.bytes_per_sample(fmt) // 2
        assert np.array_equal(formats.to_x(fmt, raw), x)
    assert np.array_equal(formats.encode("s16", x).view("<i2").astype(np.int32), x.astype(np.int32) << 2)
    assert np.array_equal(formats.encode("f32", x).view("<f4").astype(np.float64) * 8192.0, x.astype(np.float64))
    x64 = np.arange(-8192, 8192, 64, dtype=np.int16)
    for fmt in ("u8", "s8"):
        assert np.array_equal(formats.to_x(fmt, formats.encode(fmt, x64)), x64)
    assert np.array_equal(formats.encode("s8", x64), formats.encode("u8", x64) ^ 0x80)
    with pytest.raises(AssertionError):
        formats.encode("s8", np.array([65], dtype=np.int16))


def test_the_fine_scenes_reach_x():
    """The finer scenes do what they are for: the dropped bits of s16d move x (the shift floors), the content below u8's
    resolution of s16 reaches x, and f32 rounds where s16 floors."""
    p, q = 4, 3
    x = formats.to_x("u8", scene_u8(p, q)[0]).astype(np.int32)
    d = formats.to_x("s16", scene("s16d", p, q)[0]).astype(np.int32)
    assert set(np.unique(d - x).tolist()) == {-1, 0}
    e = formats.to_x("s16", scene("s16", p, q)[0]).astype(np.int32)
    assert set(np.unique(e - x).tolist()) == set(range(-32, 32))
    f = formats.to_x("f32", scene("f32", p, q)[0]).astype(np.int32)
    assert set(np.unique(f - e).tolist()) == {0, 1}
    assert np.array_equal(formats.to_x("s8", scene("s8", p, q)[0]), x)


@pytest.mark.parametrize("p,q", [(4, 3), (1, 1)])
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_gpu_scenes_decode(kind, p, q):
    """Non-vacuity of test_formats_gpu.py: the oracle alone, fed the restatement's stage 0 of the scene, decodes at least 8
    telegrams per scene."""
    n = sum(1 for s in range(len(SCENE_STREAMS)) for e in scene_oracle(kind, p, q, s).events_full() if e[7] == 1)
    assert n >= 8, n


# ---- tfrec_amd_create_format: what is refused before a device is opened
def test_create_format_argument_errors():
    L = api.load_library()
    cfg = api.Config(2, TYPES, THRESH, 0, 0, 4, 4096, api.F_ALL_FLUSHES)
    h = api.C.c_void_p()
    assert L.tfrec_amd_create_format(None, 2, 4, 3, api.C.byref(h)) == api.E_INVAL
    assert L.tfrec_amd_create_format(api.C.byref(cfg), 2, 4, 3, None) == api.E_INVAL
    for fmt in (-1, 4, 7, 1 << 20):  # an unknown format
        assert L.tfrec_amd_create_format(api.C.byref(cfg), fmt, 4, 3, api.C.byref(h)) == api.E_INVAL and not h
        assert L.tfrec_amd_create_format(api.C.byref(cfg), fmt, 1, 1, api.C.byref(h)) == api.E_INVAL and not h
    for fmt in (1, 2, 3):
        for p, q in ((3, 4), (10, 1), (130, 128), (0, 1), (1, 0), (2, 2)):  # neither 1/1 nor a rate tfrec_amd_create_rate takes
            assert L.tfrec_amd_create_format(api.C.byref(cfg), fmt, p, q, api.C.byref(h)) == api.E_INVAL and not h
    assert L.tfrec_amd_create_format(api.C.byref(cfg), 0, 3, 4, api.C.byref(h)) == api.E_INVAL and not h
    cfg.flags = api.F_ALL_FLUSHES | api.F_INPUT_10X  # the 15.36 MS/s input is u8
    for fmt in (1, 2, 3):
        for p, q in ((1, 1), (4, 3), (10, 1)):
            assert L.tfrec_amd_create_format(api.C.byref(cfg), fmt, p, q, api.C.byref(h)) == api.E_INVAL and not h
    assert L.tfrec_amd_get_input_format(None, None) == api.E_INVAL
    with pytest.raises(api.TfrecAmdError) as e:
        api.Receiver(1, input_format="s24")
    assert e.value.code == api.E_INVAL
    assert "tfrec_amd_create_format" in api.EXPORTS and "tfrec_amd_get_input_format" in api.EXPORTS


# ---- tfrec_gpu -F: what is decided before a device is opened
@pytest.fixture(scope="module")
def cli():
    return parity.build_cli()


def test_cli_format_argument_errors(cli, tmp_path):
    missing = str(tmp_path / "missing.iq")
    for bad in ("s24", "", "S16", "u16", "f64"):
        out = parity.run_cli(["-F", bad, "-L", missing])
        assert out.returncode == 1 and "bad -F" in out.stderr, bad
    for fmt in ("s16", "cs8", "f32"):
        out = parity.run_cli(["-F", fmt, "-x", "-L", missing])
        assert out.returncode == 1 and "exclude" in out.stderr, fmt
    out = parity.run_cli(["-F", "u8", "-x", "-L", missing])  # u8 is no format of its own: the file is looked for
    assert out.returncode == 2 and "missing.iq" in out.stderr
    for fmt in ("u8", "cu8", "s8", "cs8", "s16", "cs16", "f32", "cf32"):
        out = parity.run_cli(["-F", fmt, "-r", "2048000", "-b", "4", "-L", missing])
        assert out.returncode == 2 and "missing.iq" in out.stderr and "rounded up to 6" in out.stderr, fmt
    out = parity.run_cli(["-F", "s16", "-r", "1000000", "-L", missing])
    assert out.returncode == 1 and "does not take" in out.stderr


@pytest.mark.parametrize("args,piece,unit", [
    (["-F", "s16", "-r", "2048000"], 65536 * 4 * 2, 3),   # 4/3: pieces of 3 blocks, 4 bytes per complex sample
    (["-F", "cf32", "-r", "2048000"], 65536 * 4 * 4, 3),
    (["-F", "s8", "-r", "2400000"], 102400, 1),            # 25/16: 65536 * 25 / 16 bytes per block
    (["-F", "cs16", "-r", "2400000"], 204800, 1),
    (["-F", "f32"], 65536 * 4, 1),                         # without -r: 1.536 MS/s
    (["-F", "s16", "-r", "1536000"], 65536 * 2, 1),
])
def test_cli_block_size_arithmetic(cli, tmp_path, args, piece, unit):
    """A file of two pieces and a bit is cut into 2 * unit blocks of 65536 * P / Q * bytes per sample / 2 bytes each (-D reports
    the cut before a device is opened; the run itself then needs one)."""
    f = tmp_path / "two_and_a_bit.iq"
    with open(f, "wb") as fd:
        fd.truncate(2 * piece + piece // 2)
    out = parity.run_cli(args + ["-D", "-b", str(unit), "-L", str(f)])
    assert "%s: %d blocks, %d bytes per %d\n" % (f, 2 * unit, piece, unit) in out.stderr, out.stderr
    assert out.returncode in (0, 2)
