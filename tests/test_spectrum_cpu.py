"""The per-input power spectrum without a GPU (tfrec_amd_enable_spectrum, tfrec_gpu -P): the restatement against a
brute-force evaluation of the definition, the window, the exactness bound recomputed from the tables, where tones land, and what
tfrec_gpu decides before it opens a device.
"""
import re

import numpy as np
import pytest

import parity
from tfrec_amd import formats, spectrum, tune


def brute(x, n_bins, g):
    """The definition in Python ints, one term at a time."""
    c, s = (t.tolist() for t in tune.table())
    step = 4096 // n_bins
    w = [(32767 - c[(n * step) % 4096]) >> 1 for n in range(n_bins)]
    x = [int(v) for v in x]
    frames = (len(x) // 2) // n_bins
    p = []
    for f in range(frames):
        xi = [(x[2 * (f * n_bins + n)] * w[n] + (1 << 14)) >> 15 for n in range(n_bins)]
        xq = [(x[2 * (f * n_bins + n) + 1] * w[n] + (1 << 14)) >> 15 for n in range(n_bins)]
        row = []
        for k in range(n_bins):
            re_, im_ = 0, 0
            for n in range(n_bins):
                t = (k * n * step) % 4096
                re_ += xi[n] * c[t] + xq[n] * s[t]
                im_ += xq[n] * c[t] - xi[n] * s[t]
            yr, yi = (re_ + (1 << 14)) >> 15, (im_ + (1 << 14)) >> 15
            row.append(yr * yr + yi * yi)
        p.append(row)
    recs = [p[r:r + g] for r in range(0, frames, g)]
    return ([[sum(col) for col in zip(*r)] for r in recs], [[max(col) for col in zip(*r)] for r in recs], [len(r) for r in recs])


def test_restatement_equals_the_brute_force_definition():
    rng = np.random.default_rng(5)
    x = rng.integers(-8192, 8192, 2 * (5 * 64 + 17)).astype(np.int16)  # 5 frames and a tail that is not analysed
    x[:8] = [-8192, 8191, 8191, -8192, -8192, -8192, 8191, 8191]
    s, p, nf = spectrum.spectrum(x, 64, 2)
    ws, wp, wn = brute(x, 64, 2)
    assert s.dtype == np.uint64 and p.dtype == np.uint64 and nf.dtype == np.uint32
    assert s.tolist() == ws and p.tolist() == wp and nf.tolist() == wn == [2, 2, 1]
    # the raw rows go through formats.to_x
    raw = formats.encode("s16", x)
    for a, b in zip(spectrum.spectrum(raw, 64, 2, fmt="s16"), (s, p, nf)):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("n_bins", spectrum.BINS)
def test_window(n_bins):
    w = spectrum.window(n_bins)
    assert len(w) == n_bins and w[0] == 0 and w[n_bins // 2] == 32767 and w.min() == 0 and w.max() == 32767
    assert np.array_equal(w[1:], w[1:][::-1])  # periodic Hann: w[n] = w[N - n]


def test_the_exactness_bound_from_the_tables():
    """A term is at most 8192 (|C[t]| + |S[t]|); at N = 1024 the sum over n of that bound stays below 2^39 for every bin,
    p below 2^49 and a record of 16384 frames below 2^63."""
    c, s = (t.astype(np.int64) for t in tune.table())
    assert int((np.abs(c) + np.abs(s)).max()) * 8192 < 1 << 29
    n_bins = 1024
    w = spectrum.window(n_bins)
    xw_max = (8192 * w + (1 << 14)) >> 15  # |xw| for |x| <= 8192
    assert xw_max.max() <= 8192
    ct, st = spectrum.twiddles(n_bins)
    x_max = int(((np.abs(ct) + np.abs(st)) * xw_max[:, None]).sum(axis=0).max())
    assert x_max < 1 << 39
    y_max = (x_max + (1 << 14)) >> 15
    p_max = 2 * y_max * y_max
    assert p_max < 1 << 49 and spectrum.G_MAX * p_max < 1 << 63
    assert n_bins * (8192 * 46341) < 1 << 53  # every partial sum of every grouping: exact in fp64 too


def tone_bytes(fmt, f_hz, fs, n, amp):
    ph = 2.0 * np.pi * f_hz / fs * np.arange(n)
    if fmt == "u8":
        v = np.stack([np.rint(128 + amp * np.cos(ph)), np.rint(128 + amp * np.sin(ph))], axis=1)
        return np.clip(v, 0, 255).astype(np.uint8).reshape(-1)
    v = np.stack([np.rint(256 * amp * np.cos(ph)), np.rint(256 * amp * np.sin(ph))], axis=1)
    return np.clip(v, -32768, 32767).astype("<i2").reshape(-1).view(np.uint8)


@pytest.mark.parametrize("fmt", ["u8", "s16"])
@pytest.mark.parametrize("f_hz", [300000, -300000, 37500])
def test_a_tone_lands_in_its_bin(fmt, f_hz):
    fs, n_bins = 2400000, 256
    raw = tone_bytes(fmt, f_hz, fs, 4 * n_bins, 100)
    s, p, nf = spectrum.spectrum(raw, n_bins, 4, fmt=fmt)
    assert nf.tolist() == [4]
    k = round(abs(f_hz) * n_bins / fs)
    want = k if f_hz > 0 else n_bins - k
    assert int(np.argmax(s[0])) == want and int(np.argmax(p[0])) == want
    # the margin over every bin more than 2 away (the Hann window's main lobe is 4 bins wide; beyond it lie its side lobes, the
    # mirror bin and the quantisation noise), taken from the restatement's own output on this input: the peak's sum over the
    # largest far sum, rounded down -- the peak exceeds every far bin by that factor, in the sums and in the peak hold alike
    d = np.abs((np.arange(n_bins) - want + n_bins // 2) % n_bins - n_bins // 2)
    far = d > 2
    assert far.sum() == n_bins - 5 and far[(n_bins - want) % n_bins]
    factor = int(s[0][want]) // max(1, int(s[0][far].max()))
    print("tone %+d Hz, %s: bin %d, factor %d" % (f_hz, fmt, want, factor))
    assert factor > 1
    assert all(int(s[0][want]) >= factor * int(v) for v in s[0][far])
    assert all(int(p[0][want]) > int(v) for v in p[0][far])


def test_dc_and_nyquist_inputs():
    n_bins = 128
    # all bytes 0: x = -8192 on both rails, a tone at 0 Hz -- the Hann window leaves bins 0, 1 and N - 1
    s, p, nf = spectrum.spectrum(np.zeros(2 * 3 * n_bins, dtype=np.uint8), n_bins, 3, fmt="u8")
    assert nf.tolist() == [3] and int(np.argmax(s[0])) == 0
    assert (s[0][2:n_bins - 1] * 1000 < s[0][0]).all() and s[0][1] == s[0][n_bins - 1] and s[0][1] > 0
    assert (s[0] == 3 * p[0]).all()  # every frame is the same
    # samples alternating 0 and 255 (both rails of a sample alike): the tone at fs / 2, bin N / 2, beside the DC that -8192 / +8128 leaves
    x = np.repeat(np.tile(np.array([0, 255], dtype=np.uint8), 3 * n_bins // 2), 2)
    s, p, nf = spectrum.spectrum(x, n_bins, 3, fmt="u8")
    assert int(np.argmax(s[0])) == n_bins // 2 and s[0][n_bins // 2] > 1000 * s[0][n_bins // 4]


def test_the_short_last_record_and_the_arguments():
    rng = np.random.default_rng(6)
    x = rng.integers(0, 256, 2 * 7 * 64, dtype=np.uint8)
    s, p, nf = spectrum.spectrum(x, 64, 3, fmt="u8")
    assert s.shape == p.shape == (3, 64) and nf.tolist() == [3, 3, 1]
    assert np.array_equal(s[2], p[2])  # one frame: its sum is its peak
    fp = spectrum.frame_power(formats.to_x("u8", x), 64)
    assert np.array_equal(s[1], fp[3:6].sum(axis=0, dtype=np.uint64)) and np.array_equal(p[1], fp[3:6].max(axis=0))
    # records of whole frames do not depend on the cut: 7 frames as 6 + 1 with G = 3
    a = spectrum.spectrum(x[:2 * 6 * 64], 64, 3, fmt="u8")
    b = spectrum.spectrum(x[2 * 6 * 64:], 64, 3, fmt="u8")
    for whole, first, second in zip((s, p, nf), a, b):
        assert np.array_equal(whole, np.concatenate([first, second]))
    for bad in (0, 32, 100, 2048):
        with pytest.raises(ValueError):
            spectrum.spectrum(x, bad, 1, fmt="u8")
    for bad in (0, -1, 16385):
        with pytest.raises(ValueError):
            spectrum.spectrum(x, 64, bad, fmt="u8")


# ---- tfrec_gpu -P: what is decided before a device is opened
@pytest.fixture(scope="module")
def cli():
    return parity.build_cli()


def test_cli_spectrum_usage_errors(cli, tmp_path):
    f = str(tmp_path / "missing.iq")
    for extra in (["-s", "50"], ["-n", "2"], ["-p", "t=100"], ["-L", f], ["-d", "0,1"], ["-X", f]):
        out = parity.run_cli(["-P", "256", "-L", f] + extra)
        assert out.returncode == 1 and "-P takes the spectrum of one -L file" in out.stderr, extra
    for bad in ("0", "100", "2048", "32", "x", "", "256,", "256,0", "256,16385", "256,x", "256;4", "-64"):
        out = parity.run_cli(["-P", bad, "-L", f])
        assert out.returncode == 1 and "bad -P" in out.stderr, bad
    for args in (["-P", "64"], ["-P", "1024,16384", "-x"], ["-P", "256,1", "-r", "2400000", "-F", "s16"], ["-P", "512", "-c", "433920"]):
        out = parity.run_cli(args + ["-L", f])  # accepted: the file is looked for
        assert out.returncode == 2 and "missing.iq" in out.stderr, args
    out = parity.run_cli(["-P", "256"])
    assert out.returncode == 1 and "need -L" in out.stderr


@pytest.mark.parametrize("args,fs_in,n_bins,g", [
    (["-r", "2400000", "-c", "868250", "-P", "256"], 2400000, 256, 200),
    (["-c", "868250", "-P", "64,7"], 1536000, 64, 7),
    (["-x", "-c", "868250", "-P", "1024"], 15360000, 1024, 320),
    (["-r", "2048000", "-c", "433920", "-P", "512"], 2048000, 512, 85),
])
def test_cli_spectrum_bin_list(cli, tmp_path, args, fs_in, n_bins, g):
    """The bins in ascending frequency, c + (k < N/2 ? k : k - N) fs_in / N, and the default record: the frames one block's input
    holds (32768 P / Q samples) -- listed before a device is opened (the run itself then needs one)."""
    f = tmp_path / "empty.iq"
    f.write_bytes(b"")
    out = parity.run_cli(args + ["-L", str(f)])
    assert out.returncode in (0, 2)
    c = int(args[args.index("-c") + 1])
    assert "spec: %d bins, %d frames per record, input rate %d S/s" % (n_bins, g, fs_in) in out.stderr
    got = re.findall(r"^spec bin (\S+) kHz$", out.stderr, re.M)
    khz = spectrum.bin_khz(c, fs_in, n_bins)
    want = ["%.3f" % khz[(i + n_bins // 2) % n_bins] for i in range(n_bins)]
    assert got == want and [float(v) for v in got] == sorted(float(v) for v in got)
    assert got[n_bins // 2] == "%.3f" % c and got[0] == "%.3f" % (c - fs_in / 2000.0)
    if fs_in == 2400000:
        assert got[1] == "867059.375" and got[-1] == "869440.625"
