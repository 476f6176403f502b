"""The per-input power spectrum on the GPU (tfrec_amd_enable_spectrum, tfrec_amd_read_spectrum, tfrec_gpu -P), bit
for bit: every record is compared with the restatement tfrec_amd/spectrum.py run on the very bytes submitted.  The transform is
an exact integer DFT, so there is no tolerance anywhere."""
import subprocess

import numpy as np
import pytest

import parity
from meter_rows import assert_spectrum, golden, scan_file, tone, u8_rows, want_u8
from tfrec_amd import api, resample, spectrum

pytestmark = pytest.mark.gpu

TYPES = 0x2F
BB = api.BLOCK_BYTES


@pytest.mark.parametrize("n_bins,g,n_blocks", [(64, 7, 2), (256, 7, 2), (1024, 5, 1)])
def test_base_context_equals_the_restatement(n_bins, g, n_blocks):
    rows = u8_rows()[:, :n_blocks * BB]
    frames = rows.shape[1] // 2 // n_bins
    assert frames % g != 0  # the last record is short
    with api.Receiver(3, TYPES, 500, 0, max_blocks=2) as r:
        r.enable_spectrum(n_bins, g)
        r.submit(parity.to_device([np.ascontiguousarray(rows)])[0])
        got = [r.read_spectrum(row) for row in range(3)]
        r.drain()
    for row, w in enumerate(want_u8(n_bins, g, n_blocks)):
        assert got[row][2].sum() == frames and got[row][2][-1] == frames % g
        assert_spectrum(got[row], w, "N %d row %d" % (n_bins, row))
    # what the crafted rows are for: the tone in row 0, DC in row 1, fs / 2 in row 2
    s0, s1, s2 = (got[k][0].sum(axis=0) for k in range(3))
    assert int(np.argmax(s0[1:])) + 1 == round(0.1337 * n_bins) and int(np.argmax(s1)) == 0 and int(np.argmax(s2)) == n_bins // 2


def run_one(rows, n_blocks, n_bins, g, **kw):
    with api.Receiver(len(rows), TYPES, 500, 0, max_blocks=n_blocks, **kw) as r:
        assert r.input_bytes(n_blocks) == rows.shape[1]
        r.enable_spectrum(n_bins, g)
        r.submit(parity.to_device([np.ascontiguousarray(rows)])[0])
        got = [r.read_spectrum(k) for k in range(len(rows))]
        r.drain()
    return got


def test_an_s16_context_at_25_16_with_the_extreme_values():
    n = resample.input_samples(1, 25, 16)
    assert n == 51200
    row = parity.full_scale_row("s16", n, 3).copy()
    v = row.view("<i2")
    v[0, :6] = [32767, -32768, -32768, 32767, 32767, 32767]
    v[0, 2 * 255:2 * 255 + 4] = [-32768, -32768, 32767, -32768]  # across the boundary between frames 0 and 1
    v[0, -2:] = [-32768, 32767]
    got = run_one(row, 1, 256, 3, input_rate=(25, 16), input_format="s16")
    assert got[0][2].tolist() == [3] * 66 + [2]
    assert_spectrum(got[0], spectrum.spectrum(row[0], 256, 3, fmt="s16"), "s16 25/16")


def test_an_f32_context_at_4_3_with_values_no_sample_should_hold():
    n = resample.input_samples(3, 4, 3)
    assert n == 131072
    row = parity.full_scale_row("f32", n, 4).copy()
    v = row.view("<f4")
    rng = np.random.default_rng(8)
    for val in (np.nan, np.inf, -np.inf, 3.0e38, -3.0e38, 1.0e30, 0.99993896484375, -1.0, 0.5 / 8192, 1.5 / 8192, -0.0):
        v[0, rng.integers(0, 2 * n, 40)] = val
    got = run_one(row, 3, 512, 5, input_rate=(4, 3), input_format="f32")
    assert got[0][2].tolist() == [5] * 51 + [1]
    assert_spectrum(got[0], spectrum.spectrum(row[0], 512, 5, fmt="f32"), "f32 4/3")


def test_a_10x_context():
    rng = np.random.default_rng(12)
    n = 327680
    row = np.clip(rng.integers(96, 160, 2 * n) + np.rint(tone(n, -0.31, 90.0)), 0, 255).astype(np.uint8).reshape(1, -1)
    got = run_one(row, 1, 128, 100, input_10x=True)
    assert got[0][2].tolist() == [100] * 25 + [60]
    assert_spectrum(got[0], spectrum.spectrum(row[0], 128, 100, fmt="u8"), "10x")
    assert int(np.argmax(got[0][0].sum(axis=0))) == 128 - round(0.31 * 128)


def test_events_levels_and_captures_do_not_depend_on_it():
    x = parity.to_device([np.ascontiguousarray(golden())])[0]
    n_bins, g, nb = 256, 50, 3
    out = []
    for spec in (False, True):
        with api.Receiver(1, TYPES, 500, 0, max_blocks=nb, levels=True, all_flushes=True) as r:
            r.enable_capture(1024, nb * api.BLOCK_DEC)
            before = r.memory()
            if spec:
                r.enable_spectrum(n_bins, g)
                after = r.memory()
                records = -(-(nb * BB // 2 // n_bins) // g)
                assert after["device_bytes"] - before["device_bytes"] == api.FIFO_DEPTH * 1 * records * (n_bins * 16 + 4)
                assert after["pinned_host_bytes"] == before["pinned_host_bytes"]
            r.submit(x)
            if spec:
                assert_spectrum(r.read_spectrum(0), spectrum.spectrum(golden()[0], n_bins, g, fmt="u8"), "golden")
            lv = r.read_levels()
            runs, samples = r.read_captures()
            out.append((parity.sort_events(r.drain()), lv, runs, samples))
    (ev0, lv0, runs0, smp0), (ev1, lv1, runs1, smp1) = out
    assert len(ev0) > 0 and (ev0["status"] == 1).any() and len(runs0) > 0
    assert ev0.tobytes() == ev1.tobytes() and lv0.tobytes() == lv1.tobytes()
    assert runs0.tobytes() == runs1.tobytes() and smp0.tobytes() == smp1.tobytes()
    # ... and a plain context without levels and capture decodes the same with and without it
    plain = []
    for spec in (False, True):
        with api.Receiver(1, TYPES, 500, 0, max_blocks=nb) as r:
            if spec:
                r.enable_spectrum(1024, 1)
            r.submit(x)
            plain.append(parity.sort_events(r.drain()))
    assert len(plain[0]) > 0 and plain[0].tobytes() == plain[1].tobytes()


def test_without_the_call_the_read_is_refused():
    with api.Receiver(1, TYPES, 500, 0, max_blocks=1) as r:
        for submitted in (False, True):
            if submitted:
                r.submit(parity.to_device([np.ascontiguousarray(u8_rows()[:1, :BB])])[0])
            with pytest.raises(api.TfrecAmdError) as e:
                r.read_spectrum(0)
            assert e.value.code == api.E_INVAL
        r.drain()


def test_two_queued_submits_give_their_own_records():
    rows = u8_rows()
    parts = parity.to_device(parity.cut(rows, (1, 1)))
    with api.Receiver(3, TYPES, 500, 0, max_blocks=1) as r:
        r.enable_spectrum(64, 7)
        with pytest.raises(api.TfrecAmdError) as e:
            r.read_spectrum(0)  # nothing undrained
        assert e.value.code == api.E_STATE
        for p in parts:
            r.submit(p)
        for k in range(2):
            for row in range(3):
                assert_spectrum(r.read_spectrum(row), want_u8(64, 7, 1, k)[row], "submit %d row %d" % (k, row))
            assert_spectrum(r.read_spectrum(0), want_u8(64, 7, 1, k)[0], "submit %d again" % k)  # reading pops nothing
            r.drain()
        with pytest.raises(api.TfrecAmdError) as e:
            r.read_spectrum(0)
        assert e.value.code == api.E_STATE


def test_four_blocks_equal_one_plus_three_where_the_cut_is_aligned():
    n_bins, g = 256, 128  # a block holds 128 frames: N divides n_in and G divides F in every submit
    rows = np.concatenate([u8_rows()[:1], u8_rows()[:1, ::-1]], axis=1)
    got = []
    for sizes in ((4,), (1, 3)):
        recs = []
        with api.Receiver(1, TYPES, 500, 0, max_blocks=4) as r:
            r.enable_spectrum(n_bins, g)
            for p in parity.to_device(parity.cut(rows, sizes)):
                r.submit(p)
                recs.append(r.read_spectrum(0))
                r.drain()
        got.append([np.concatenate([x[i] for x in recs]) for i in range(3)])
    assert_spectrum(got[0], spectrum.spectrum(rows[0], n_bins, g, fmt="u8"), "one submit")
    assert_spectrum(got[1], got[0], "1 + 3")
    assert got[0][2].tolist() == [128] * 4


def test_rows_follow_the_map_and_max_rows():
    rows = u8_rows()
    with api.Receiver(3, TYPES, 500, 0, max_blocks=2) as r:  # three streams on row 0: one row is provided and analysed
        r.map_streams([0, 1, 2], 0)
        r.enable_spectrum(64, 7)
        r.submit(parity.to_device([np.ascontiguousarray(rows[:1])])[0])
        assert_spectrum(r.read_spectrum(0), want_u8(64, 7)[0], "mapped row 0")
        for bad in (1, 2, -1, 3):
            with pytest.raises(api.TfrecAmdError) as e:
                r.read_spectrum(bad)
            assert e.value.code == api.E_INVAL
        r.drain()
    with api.Receiver(2, TYPES, 500, 0, max_blocks=2) as r:  # max_rows = 1 on a two-row submit
        r.enable_spectrum(64, 7, max_rows=1)
        r.submit(parity.to_device([np.ascontiguousarray(rows[1:3])])[0])
        assert_spectrum(r.read_spectrum(0), want_u8(64, 7)[1], "max_rows 1")
        with pytest.raises(api.TfrecAmdError) as e:
            r.read_spectrum(1)
        assert e.value.code == api.E_INVAL
        r.drain()


def test_submit_host_gives_the_records_of_submit_device():
    rows = np.ascontiguousarray(u8_rows())
    with api.Receiver(3, TYPES, 500, 0, max_blocks=2) as r:
        r.enable_spectrum(256, 7)
        r.submit(rows)  # a numpy array: tfrec_amd_submit_host
        r.submit(rows[:, ::-1].copy())  # the staging buffers of two sets in flight
        for row in range(3):
            assert_spectrum(r.read_spectrum(row), want_u8(256, 7)[row], "host row %d" % row)
        r.drain()
        assert_spectrum(r.read_spectrum(0), spectrum.spectrum(rows[0, ::-1], 256, 7, fmt="u8"), "second host submit")
        r.drain()


def test_call_order_and_argument_errors():
    L = api.load_library()
    assert L.tfrec_amd_enable_spectrum(None, 64, 1, 1) == api.E_INVAL
    with api.Receiver(2, TYPES, 500, 0, max_blocks=1) as r:
        for bad in ((0, 1, 1), (32, 1, 1), (96, 1, 1), (2048, 1, 1), (-64, 1, 1), (64, 0, 1), (64, -1, 1), (64, 16385, 1), (64, 1, 0),
                    (64, 1, 3), (64, 1, -1)):
            with pytest.raises(api.TfrecAmdError) as e:
                r.enable_spectrum(*bad)
            assert e.value.code == api.E_INVAL, bad
        r.enable_spectrum(64, 16384, 2)
        with pytest.raises(api.TfrecAmdError) as e:
            r.enable_spectrum(64, 16384, 2)  # a second call
        assert e.value.code == api.E_INVAL
        r.submit(parity.to_device([np.ascontiguousarray(u8_rows()[:2, :BB])])[0])
        # the arrays may be NULL only to fetch the count; too little room writes nothing but sets the count
        nr = api.C.c_int(-1)
        assert L.tfrec_amd_read_spectrum(r.h, 0, None, None, 0, None, api.C.byref(nr)) == api.E_INVAL and nr.value == 1
        assert L.tfrec_amd_read_spectrum(r.h, 0, None, None, 0, None, None) == api.E_INVAL
        s = np.full(64, 7, dtype=np.uint64)
        assert L.tfrec_amd_read_spectrum(r.h, 0, s.ctypes.data, None, 1, None, api.C.byref(nr)) == api.E_INVAL and (s == 7).all()
        got = r.read_spectrum(1)
        assert got[2].tolist() == [512]  # one record, short of G
        r.drain()
    with api.Receiver(1, TYPES, 500, 0, max_blocks=1) as r:
        r.submit(parity.to_device([np.ascontiguousarray(u8_rows()[:1, :BB])])[0])
        with pytest.raises(api.TfrecAmdError) as e:
            r.enable_spectrum(64, 1)
        assert e.value.code == api.E_STATE
        r.drain()


def test_cli_spectrum_of_the_scan_file(tmp_path):
    cli = parity.build_cli()
    x = scan_file()
    f = tmp_path / "scan.iq"
    x.tofile(f)
    c, fs, n_bins = 868250, 2048000, 256
    base = [cli, "-r", "2048000", "-c", str(c), "-T", "2f", "-t", "500", "-b", "3"]
    plain = subprocess.run(base + ["-f", str(c + 600), "-L", str(f)], capture_output=True, text=True, timeout=300)
    out = subprocess.run(base + ["-f", str(c + 600), "-P", "256", "-L", str(f)], capture_output=True, text=True, timeout=300)
    dbg = subprocess.run(base + ["-f", str(c + 600), "-P", "256", "-D", "-L", str(f)], capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0 and out.returncode == 0 and dbg.returncode == 0, plain.stderr + out.stderr + dbg.stderr
    assert len(parity.telegram_lines(plain.stdout)) >= 1
    assert parity.telegram_lines(out.stdout) == parity.telegram_lines(plain.stdout)
    # the restatement on the file: one submit of 3 blocks, G = the frames of a block's input, floor(32768 * 4 / 3 / 256) = 170
    s, p, nf = spectrum.spectrum(x, n_bins, 170, fmt="u8")
    assert nf.tolist() == [170, 170, 170, 2]
    khz = spectrum.bin_khz(c, fs, n_bins)
    order = [(i + n_bins // 2) % n_bins for i in range(n_bins)]
    total = [sum(int(v) for v in s[:, k]) for k in range(n_bins)]
    want = ["spec %.3f mean=%d peak=%d" % (khz[k], total[k] // int(nf.sum()), int(p[:, k].max())) for k in order]
    lines = out.stdout.splitlines()
    assert [ln for ln in lines if ln.startswith("spec ")] == want and lines[-n_bins:] == want  # behind the telegram output
    assert lines[:-n_bins] == plain.stdout.splitlines() and not any(ln.startswith("spec-rec ") for ln in lines)
    lines = dbg.stdout.splitlines()  # -D: every record ahead of the table
    assert lines[-n_bins:] == want
    want_rec = ["spec-rec %d %.3f sum=%d peak=%d frames=%d" % (q, khz[k], s[q, k], p[q, k], nf[q]) for q in range(len(nf)) for k in order]
    assert [ln for ln in lines if ln.startswith("spec-rec ")] == want_rec and lines[-n_bins - len(want_rec):-n_bins] == want_rec
    # the bin with the largest peak is the one the restatement names: the scene sits at +600 kHz, bin 75
    peaks = [int(ln.split()[3].split("=")[1]) for ln in want]
    best = order[int(np.argmax(peaks))]
    assert best == int(np.argmax(p.max(axis=0))) and abs(khz[best] - (c + 600)) <= 60
