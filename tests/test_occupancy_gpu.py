"""The occupancy detector on the GPU (tfrec_amd_enable_occupancy, tfrec_amd_read_occupancy, tfrec_gpu -A), bit for bit:
every struct and bitmap word is compared with the restatement tfrec_amd/occupancy.py, twice -- on the context's own spectrum records,
which isolates the detector's kernel, and on the submitted bytes through tfrec_amd/spectrum.py.  Exact integers: no tolerance."""
import subprocess

import numpy as np
import pytest

import parity
from meter_rows import assert_spectrum, golden, scan_file, tone, u8_rows, want_u8
from tfrec_amd import api, occupancy, resample, spectrum

pytestmark = pytest.mark.gpu

TYPES = 0x2F
BB = api.BLOCK_BYTES


def assert_occupancy(got, want, label=""):
    for name, g, w in zip(("records", "bitmap"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, "%s %s: %s %s, want %s %s" % (label, name, g.dtype, g.shape, w.dtype, w.shape)
        if g.tobytes() != w.tobytes():
            bad = np.argwhere(g != w)
            raise AssertionError("%s %s: %d values differ, first at %s: got %s, want %s" % (
                label, name, len(bad), tuple(bad[0]), g[tuple(bad[0])], w[tuple(bad[0])]))


def check_row(r, row, want_spec, ratio=occupancy.RATIO, rel=occupancy.REL, label=""):
    """Row `row` of the oldest undrained submit: the detector's output against the restatement on the context's own spectrum records
    and on the restatement of the spectrum -> (records, bitmap)."""
    spec = r.read_spectrum(row)
    got = r.read_occupancy(row)
    assert_occupancy(got, occupancy.occupancy(*spec, ratio, rel), label + " on the context's records")
    assert_occupancy(got, occupancy.occupancy(*want_spec, ratio, rel), label + " on the submitted bytes")
    return got


@pytest.mark.parametrize("n_bins,g,n_blocks", [(64, 7, 2), (256, 7, 2), (1024, 5, 1)])
def test_base_context_equals_the_restatement(n_bins, g, n_blocks):
    rows = u8_rows()[:, :n_blocks * BB]
    assert (rows.shape[1] // 2 // n_bins) % g != 0  # the last record is short
    with api.Receiver(3, TYPES, 500, 0, max_blocks=2) as r:
        r.enable_spectrum(n_bins, g)
        r.enable_occupancy()
        r.submit(parity.to_device([np.ascontiguousarray(rows)])[0])
        got = [check_row(r, row, w, label="N %d row %d" % (n_bins, row)) for row, w in enumerate(want_u8(n_bins, g, n_blocks))]
        r.drain()
    # what the crafted rows are for: the tone of row 0 stands out of its full-range noise (from 256 bins on: at 64 a bin is too
    # wide for it); all bytes 0 (row 1) is DC, which the Hann window spreads over bins 0, 1 and N - 1, above a floor of rounding
    # residue; row 2 is the tone at fs / 2 beside its DC
    hit = [occupancy.unpack(b, n_bins) for _, b in got]
    assert (got[0][0]["floor"] > 0).all() and (n_bins == 64 or hit[0][:, round(0.1337 * n_bins)].all())
    assert hit[1][:, 0].all() and not hit[1][:, 2:n_bins - 1].any() and (got[1][0]["n_hit"] == 3).all()
    assert hit[2][:, n_bins // 2].all()
    for recs, bits in got:
        assert (recs["n_hit"] == occupancy.unpack(bits, n_bins).sum(axis=1)).all() and recs["n_frames"][-1] < g


@pytest.mark.parametrize("ratio,rel", [(2, 1), (4096, 4096), (2, 4096), (4096, 1)])
def test_the_parameters_at_their_extremes(ratio, rel):
    n_bins, g = 256, 7
    with api.Receiver(3, TYPES, 500, 0, max_blocks=2) as r:
        r.enable_spectrum(n_bins, g)
        r.enable_occupancy(ratio, rel)
        r.submit(parity.to_device([np.ascontiguousarray(u8_rows())])[0])
        got = [check_row(r, row, w, ratio, rel, "ratio %d rel %d row %d" % (ratio, rel, row)) for row, w in enumerate(want_u8(n_bins, g))]
        r.drain()
    if (ratio, rel) == (2, 1):  # only the bin that equals the record's top (at ratio 4096 not even that one stands over the noise)
        assert (got[0][0]["n_hit"] == 1).all()
    if ratio == 4096:
        assert (got[0][0]["n_hit"] == 0).all()
    if (ratio, rel) == (2, 4096):  # the noise of row 0: a frame's peak over twice the mean nearly everywhere
        assert (got[0][0]["n_hit"] > n_bins // 2).all()


def run_one(rows, n_blocks, n_bins, g, **kw):
    with api.Receiver(len(rows), TYPES, 500, 0, max_blocks=n_blocks, **kw) as r:
        assert r.input_bytes(n_blocks) == rows.shape[1]
        r.enable_spectrum(n_bins, g)
        r.enable_occupancy()
        r.submit(parity.to_device([np.ascontiguousarray(rows)])[0])
        got = [(r.read_spectrum(k), r.read_occupancy(k)) for k in range(len(rows))]
        r.drain()
    return got


def test_an_s16_context_at_25_16():
    n = resample.input_samples(1, 25, 16)
    row = parity.full_scale_row("s16", n, 3).copy()
    v = row.view("<i2").reshape(1, -1, 2)
    ph = 2.0 * np.pi * 0.2 * np.arange(20 * 256, 40 * 256)
    v[0, 20 * 256:40 * 256, 0] = np.rint(30000 * np.cos(ph))  # a burst in frames 20 .. 39 of 200: records 6 .. 13 of 67
    v[0, 20 * 256:40 * 256, 1] = np.rint(30000 * np.sin(ph))
    (spec, got), = run_one(row, 1, 256, 3, input_rate=(25, 16), input_format="s16")
    want_spec = spectrum.spectrum(row[0], 256, 3, fmt="s16")
    assert_occupancy(got, occupancy.occupancy(*spec), "s16 25/16 on the context's records")
    assert_occupancy(got, occupancy.occupancy(*want_spec), "s16 25/16 on the submitted bytes")
    assert got[0]["n_frames"].tolist() == [3] * 66 + [2]
    hit = occupancy.unpack(got[1], 256)
    assert hit[7:13, round(0.2 * 256)].all() and not hit[:6].any() and not hit[14:].any()


def test_a_10x_context():
    rng = np.random.default_rng(12)
    n = 327680
    row = np.clip(rng.integers(96, 160, 2 * n) + np.rint(tone(n, -0.31, 90.0)), 0, 255).astype(np.uint8).reshape(1, -1)
    (spec, got), = run_one(row, 1, 128, 100, input_10x=True)
    want_spec = spectrum.spectrum(row[0], 128, 100, fmt="u8")
    assert_occupancy(got, occupancy.occupancy(*spec), "10x on the context's records")
    assert_occupancy(got, occupancy.occupancy(*want_spec), "10x on the submitted bytes")
    assert got[0]["n_frames"].tolist() == [100] * 25 + [60]
    assert occupancy.unpack(got[1], 128)[:, 128 - round(0.31 * 128)].all()


def test_rows_follow_the_map_and_max_rows():
    rows = u8_rows()
    with api.Receiver(3, TYPES, 500, 0, max_blocks=2) as r:  # three streams on row 0: one row is provided and analysed
        r.map_streams([0, 1, 2], 0)
        r.enable_spectrum(64, 7)
        r.enable_occupancy()
        r.submit(parity.to_device([np.ascontiguousarray(rows[:1])])[0])
        check_row(r, 0, want_u8(64, 7)[0], label="mapped row 0")
        for bad in (1, 2, -1, 3):
            with pytest.raises(api.TfrecAmdError) as e:
                r.read_occupancy(bad)
            assert e.value.code == api.E_INVAL
        r.drain()
    with api.Receiver(2, TYPES, 500, 0, max_blocks=2) as r:  # max_rows = 1 on a two-row submit
        r.enable_spectrum(64, 7, max_rows=1)
        r.enable_occupancy()
        r.submit(parity.to_device([np.ascontiguousarray(rows[1:3])])[0])
        check_row(r, 0, want_u8(64, 7)[1], label="max_rows 1")
        with pytest.raises(api.TfrecAmdError) as e:
            r.read_occupancy(1)
        assert e.value.code == api.E_INVAL
        r.drain()


def test_two_queued_submits_are_read_in_fifo_order():
    parts = parity.to_device(parity.cut(u8_rows(), (1, 1)))
    with api.Receiver(3, TYPES, 500, 0, max_blocks=1) as r:
        r.enable_spectrum(64, 7)
        r.enable_occupancy()
        with pytest.raises(api.TfrecAmdError) as e:
            r.read_occupancy(0)  # nothing undrained
        assert e.value.code == api.E_STATE
        for p in parts:
            r.submit(p)
        first = None
        for k in range(2):
            got = [check_row(r, row, want_u8(64, 7, 1, k)[row], label="submit %d row %d" % (k, row)) for row in range(3)]
            assert_occupancy(r.read_occupancy(0), got[0], "submit %d again" % k)  # reading pops nothing
            first = first or got
            r.drain()
        assert first[0][0].tobytes() != got[0][0].tobytes()  # (the two submits' records differ: the order can be seen)
        with pytest.raises(api.TfrecAmdError) as e:
            r.read_occupancy(0)
        assert e.value.code == api.E_STATE


def test_four_blocks_equal_one_plus_three_where_the_cut_is_aligned():
    n_bins, g = 256, 128  # a block holds 128 frames: N divides n_in and G divides F in every submit
    rows = np.concatenate([u8_rows()[:1], u8_rows()[:1, ::-1]], axis=1)
    want_spec = spectrum.spectrum(rows[0], n_bins, g, fmt="u8")
    got = []
    for sizes in ((4,), (1, 3)):
        recs, pos = [], 0
        with api.Receiver(1, TYPES, 500, 0, max_blocks=4) as r:
            r.enable_spectrum(n_bins, g)
            r.enable_occupancy()
            for nb, p in zip(sizes, parity.to_device(parity.cut(rows, sizes))):
                r.submit(p)
                recs.append(check_row(r, 0, [a[pos:pos + nb] for a in want_spec], label="blocks %d+%d" % (pos, nb)))
                pos += nb
                r.drain()
        got.append([np.concatenate([x[i] for x in recs]) for i in range(2)])
    assert_occupancy(got[1], got[0], "1 + 3")
    assert got[0][0]["n_frames"].tolist() == [128] * 4


def test_submit_host_gives_the_records_of_submit_device():
    rows = np.ascontiguousarray(u8_rows())
    with api.Receiver(3, TYPES, 500, 0, max_blocks=2) as r:
        r.enable_spectrum(256, 7)
        r.enable_occupancy()
        r.submit(rows)  # a numpy array: tfrec_amd_submit_host
        r.submit(parity.to_device([rows])[0])
        host = [check_row(r, row, want_u8(256, 7)[row], label="host row %d" % row) for row in range(3)]
        r.drain()
        for row in range(3):
            assert_occupancy(r.read_occupancy(row), host[row], "device row %d" % row)
        r.drain()


def test_everything_else_does_not_depend_on_it():
    x = parity.to_device([np.ascontiguousarray(golden())])[0]
    n_bins, g, nb = 256, 50, 3
    out = []
    for occ in (False, True):
        with api.Receiver(1, TYPES, 500, 0, max_blocks=nb, levels=True, all_flushes=True) as r:
            r.enable_capture(1024, nb * api.BLOCK_DEC)
            r.enable_spectrum(n_bins, g)
            before = r.memory()
            if occ:
                r.enable_occupancy()
                after = r.memory()
                records = -(-(nb * BB // 2 // n_bins) // g)
                assert after["device_bytes"] - before["device_bytes"] == api.FIFO_DEPTH * 1 * records * (16 + n_bins // 8)
                assert after["pinned_host_bytes"] == before["pinned_host_bytes"]
            r.submit(x)
            spec = r.read_spectrum(0)
            if occ:
                recs, bits = check_row(r, 0, spectrum.spectrum(golden()[0], n_bins, g, fmt="u8"), label="golden")
                assert recs["n_hit"].sum() > 0  # the scene's bursts
            lv = r.read_levels()
            runs, samples = r.read_captures()
            out.append((parity.sort_events(r.drain()), lv, runs, samples, spec))
    (ev0, lv0, runs0, smp0, spec0), (ev1, lv1, runs1, smp1, spec1) = out
    assert len(ev0) > 0 and (ev0["status"] == 1).any() and len(runs0) > 0
    assert ev0.tobytes() == ev1.tobytes() and lv0.tobytes() == lv1.tobytes()
    assert runs0.tobytes() == runs1.tobytes() and smp0.tobytes() == smp1.tobytes()
    assert_spectrum(spec1, spec0, "with the detector")


def test_call_order_and_argument_errors():
    L = api.load_library()
    assert L.tfrec_amd_enable_occupancy(None, 32, 16) == api.E_INVAL
    with api.Receiver(2, TYPES, 500, 0, max_blocks=1) as r:
        with pytest.raises(api.TfrecAmdError) as e:
            r.enable_occupancy()  # without a spectrum
        assert e.value.code == api.E_INVAL
        with pytest.raises(api.TfrecAmdError) as e:
            r.read_occupancy(0)  # off
        assert e.value.code == api.E_INVAL
        r.enable_spectrum(64, 16384, 2)
        for bad in ((1, 16), (0, 16), (4097, 16), (32, 0), (32, 4097), (-1, 16), (2 ** 32, 16)):
            with pytest.raises(api.TfrecAmdError) as e:
                r.enable_occupancy(*bad)
            assert e.value.code == api.E_INVAL, bad
        mem = r.memory()
        r.enable_occupancy(2, 4096)
        assert r.memory()["device_bytes"] - mem["device_bytes"] == api.FIFO_DEPTH * 2 * 1 * (16 + 8)
        with pytest.raises(api.TfrecAmdError) as e:
            r.enable_occupancy(2, 4096)  # a second call
        assert e.value.code == api.E_INVAL
        r.submit(parity.to_device([np.ascontiguousarray(u8_rows()[:2, :BB])])[0])
        # the arrays may be NULL only to fetch the count; too little room writes nothing but sets the count
        nr = api.C.c_int(-1)
        assert L.tfrec_amd_read_occupancy(r.h, 0, None, None, 0, api.C.byref(nr)) == api.E_INVAL and nr.value == 1
        assert L.tfrec_amd_read_occupancy(r.h, 0, None, None, 0, None) == api.E_INVAL
        recs = np.full(1, 7, dtype=occupancy.OCC_DTYPE)
        assert L.tfrec_amd_read_occupancy(r.h, 0, recs.ctypes.data, None, 1, api.C.byref(nr)) == api.E_INVAL and recs["n_hit"][0] == 7
        for bad in (2, -1):
            with pytest.raises(api.TfrecAmdError) as e:
                r.read_occupancy(bad)
            assert e.value.code == api.E_INVAL
        got = check_row(r, 1, spectrum.spectrum(u8_rows()[1, :BB], 64, 16384, fmt="u8"), 2, 4096, "one short record")
        assert got[0]["n_frames"].tolist() == [512]
        r.drain()
    with api.Receiver(1, TYPES, 500, 0, max_blocks=1) as r:
        r.enable_spectrum(64, 1)
        r.submit(parity.to_device([np.ascontiguousarray(u8_rows()[:1, :BB])])[0])
        with pytest.raises(api.TfrecAmdError) as e:
            r.enable_occupancy()  # after a submit
        assert e.value.code == api.E_STATE
        with pytest.raises(api.TfrecAmdError) as e:
            r.read_occupancy(0)
        assert e.value.code == api.E_INVAL
        r.drain()


def test_cli_finds_and_scans_the_channel_of_the_scan_file(tmp_path):
    cli = parity.build_cli()
    f = tmp_path / "scan.iq"
    scan_file().tofile(f)
    base = [cli, "-r", "2048000", "-c", "868250", "-T", "2f", "-t", "500", "-b", "3"]
    auto = subprocess.run(base + ["-A", "-L", str(f)], capture_output=True, text=True, timeout=300)
    scan = subprocess.run(base + ["-s", "50", "-L", str(f)], capture_output=True, text=True, timeout=300)
    assert auto.returncode == 0 and scan.returncode == 0, auto.stderr + scan.stderr
    lines = auto.stdout.splitlines()
    assert [ln for ln in lines if ln.startswith("found ")] == ["found 868850 bins=70..80 hits=1/4"]
    assert not any(ln.startswith("carrier ") for ln in lines)
    want = [ln for ln in scan.stdout.splitlines() if ln.startswith("scan 868850 ")]
    assert len(want) == 1 and "telegrams=0" not in want[0]
    assert [ln for ln in lines if ln.startswith("scan ")] == want
    assert lines == ["found 868850 bins=70..80 hits=1/4"] + want
