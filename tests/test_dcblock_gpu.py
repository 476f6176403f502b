"""The DC blocker on the GPU (tfrec_amd_create_dc, tfrec_amd_read_dc, tfrec_amd_reset_dc_rows, tfrec_gpu -z), bit for
bit.

d[w] and stage 0 are pinned by the restatement (formats.to_x -> dcblock.dc_block -> tune.mix_in_s16 / resample.resample_x16),
everything behind stage 0 by the oracle's process_s16 fed that chain's output.  The scenes are synthetic recordings of 3 blocks (6
at 4/3, whose submits hold a multiple of 3) with one burst per protocol named and a DC offset of a few u8 LSB on each rail."""
import functools
import subprocess

import numpy as np
import pytest

import parity
from input_rows import stage0_of_x
from meter_rows import OFFSET, golden_scene, offset_scene
from oracle import oracle as O
from tfrec_amd import api, dcblock, formats, resample, synth, tune

pytestmark = pytest.mark.gpu

TYPES, THRESH = 0x2F, 500
DCS = ((8, -4), (-5, 11))  # per row, in u8 LSB
FLOOR_K = 64  # the shortest average that leaves a burst whole


@functools.lru_cache(maxsize=None)
def scene(fmt, p, q, n_blocks, freqs=(0, 0), n_rows=2):
    """[rows, bytes] (read-only): row r is a recording at 1536000 p / q in the format with a burst of protocol j at freqs[j] Hz
    and the DC offset DCS[r]."""
    n = n_blocks * 32768 * p
    rows = []
    for r in range(n_rows):
        bursts = [dict(proto=j + r, start=(6000 * p + j * (n - 12000 * p) // len(freqs)) // q * q, payload_seed=31 + j + 7 * r, f0_hz=f, amp=50)
                  for j, f in enumerate(freqs)]
        u = np.ascontiguousarray(synth.gen_scene(70 + r, n_blocks, bursts, dc_iq=DCS[r], rate_mult=p).reshape(-1, 2)[::q]).reshape(-1)
        if fmt == "u8":
            row = u
        elif fmt == "s8":
            row = u ^ 0x80
        else:
            v = np.clip(((u.astype(np.int32) - 128) << 8) + np.random.default_rng(9 + r).integers(-128, 128, u.shape), -32768, 32767)
            row = v.astype("<i2").view(np.uint8) if fmt == "s16" else (v.astype(np.float32) / np.float32(32768.0)).astype("<f4").view(np.uint8)
        rows.append(row)
    rows = np.ascontiguousarray(np.stack(rows))
    rows.setflags(write=False)
    return rows


def corrected(rows, fmt, k, sizes, p=1, q=1, reset_before=None):
    """Per row the restatement over the submits: (x' of the whole row, [d of submit i]).  reset_before: {submit: rows whose DC state
    is cleared ahead of it}."""
    out = []
    bps = formats.bytes_per_sample(fmt)
    for r, row in enumerate(rows):
        pos, st, xs, ds = 0, None, [], []
        for i, nb in enumerate(sizes):
            n = dcblock.input_samples(nb, p, q) * bps
            if reset_before and r in reset_before.get(i, ()):
                st = None
            x, d, st = dcblock.dc_block(row[pos:pos + n], fmt, k, st)
            xs.append(x)
            ds.append(d)
            pos += n
        assert pos == len(row)
        out.append((np.concatenate(xs), ds))
    return out


def oracle_of(y0, narrow_hz=0, types=TYPES, thresh=THRESH, **kw):
    o = O.Oracle(types, thresh, 0, **kw)
    o.process_s16(tune.mix_s16(y0, narrow_hz, 0) if narrow_hz else y0)
    return o


def run_dc(rows, sizes, p, q, fmt, k, *, n_streams=None, dc_rows=None, host=False, before=None, stage0=True, decimated=False, **kw):
    """A DC receiver over the rows cut into `sizes`, one submit in flight -> (events per submit, stage 0 per submit and stream, d per
    submit and row, decimated samples per submit and stream)."""
    parts = parity.cut_input(rows, sizes, fmt, p, q)
    n = len(rows) if n_streams is None else n_streams
    kw.setdefault("all_flushes", True)
    evs, y0, ds, dec = [], [], [], []
    with api.Receiver(n, TYPES, THRESH, 0, max_blocks=max(sizes), input_format=fmt, input_rate=(p, q), dc_windows=k, dc_rows=dc_rows, **kw) as r:
        assert r.input_rate == (p, q) and r.input_format == fmt and r.dc() == (k, n if dc_rows is None else dc_rows)
        for i, part in enumerate(parts if host else parity.to_device(parts)):
            assert r.input_bytes(sizes[i]) == part.shape[1]
            if before:
                before(r, i)
            r.submit(part)
            if stage0:
                y0.append([r.stage0(s, sizes[i] * 4 * api.BLOCK_DEC) for s in range(n)])
            if decimated:
                dec.append([r.decimated(s, sizes[i] * api.BLOCK_DEC) for s in range(n)])
            ds.append([r.read_dc(row) for row in range(r.rows_in_use)])
            evs.append(r.drain())
    return evs, y0, ds, dec


# ---- d, stage 0, the decimated samples and the events equal the chain of restatements
CONTEXTS = [("u8", 1, 1, 4, (1, 2)), ("u8", 1, 1, 64, (1, 2)), ("u8", 1, 1, 4096, (2, 1)), ("s8", 1, 1, 64, (3,)), ("s16", 25, 16, 4, (1, 2)),
            ("s16", 25, 16, 100, (2, 1)), ("f32", 4, 3, 64, (3, 3))]


@pytest.mark.parametrize("fmt,p,q,k,sizes", CONTEXTS, ids=["%s-%d/%d-K%d" % c[:4] for c in CONTEXTS])
def test_the_chain_equals_the_restatements(fmt, p, q, k, sizes):
    """K = 4: the ring carries within a submit and across two; K = 64 and 100: it fills inside the run; K = 4096: longer than
    everything submitted."""
    rows = scene(fmt, p, q, sum(sizes))
    want = corrected(rows, fmt, k, sizes, p, q)
    evs, y0, ds, dec = run_dc(rows, sizes, p, q, fmt, k, decimated=True)
    ev = np.concatenate(evs)
    telegrams = 0
    for s in range(len(rows)):
        x, d = want[s]
        for i in range(len(sizes)):
            assert ds[i][s].shape == d[i].shape and np.array_equal(ds[i][s], d[i]), (s, i)
        w0 = stage0_of_x(x, p, q)
        parity.assert_stage0(y0, sizes, w0, s, fmt)
        orc = oracle_of(w0, keep_dec=True)
        assert np.array_equal(np.concatenate([dd[s] for dd in dec]), orc.dec()), s
        assert parity.assert_segment(ev, s, orc, "stream %d" % s) > 0
        telegrams += len(parity.decoded(orc))
    if k >= FLOOR_K:
        assert telegrams >= 2
        raw = O.Oracle(TYPES, THRESH, 0)  # ... none of which the uncorrected row yields
        raw.process_s16(stage0_of_x(formats.to_x(fmt, rows[0]), p, q))
        assert parity.decoded(raw) == []


@pytest.mark.parametrize("mode", ["shallow", "serial_chains", "default_mode", "bits", "host"])
def test_every_mode_works(mode, monkeypatch):
    kw, layout, flags = parity.mode_kwargs(mode, monkeypatch)
    fmt, p, q, k, sizes = "u8", 1, 1, 64, (2, 1)
    rows = scene(fmt, p, q, 3)
    want = corrected(rows, fmt, k, sizes)
    layouts = []
    evs, _, ds, _ = run_dc(rows, sizes, p, q, fmt, k, host=flags["host"], stage0=False, timing=True,
                           before=lambda r, i: layouts.append(r.layout()), **kw)
    assert layouts[0] == layout
    ev = np.concatenate(evs)
    for s in range(len(rows)):
        orc = oracle_of(want[s][0], log_bits=flags["bits"])
        assert parity.assert_stream(ev, s, orc, default_mode=flags["default_mode"]) > 0
        if flags["bits"]:
            assert parity.assert_bits(ev, s, orc, "stream %d" % s) > 100
        assert np.array_equal(ds[1][s], want[s][1][1])


# ---- rows and streams
TUNES = (200000, -200000)


def test_two_streams_share_one_corrected_row():
    """max_rows = 1: both streams are mapped to row 0 and tuned to a burst each; the row is corrected once."""
    fmt, p, q, k, sizes = "u8", 1, 1, 64, (2, 1)
    rows = scene(fmt, p, q, 3, TUNES, 1)
    (x, d), = corrected(rows, fmt, k, sizes)

    def before(r, i):
        if i == 0:
            r.map_streams([0, 1], [0, 0])
            r.tune_streams([0, 1], TUNES)
            assert r.rows_in_use == 1

    evs, y0, ds, _ = run_dc(rows, sizes, p, q, fmt, k, n_streams=2, dc_rows=1, before=before)
    ev = np.concatenate(evs)
    for i in range(2):
        assert len(ds[i]) == 1 and np.array_equal(ds[i][0], d[i])
    for s, hz in enumerate(TUNES):
        parity.assert_stage0(y0, sizes, x, s)  # stage 0 is ahead of the tune: the corrected row itself
        orc = oracle_of(x, hz)
        assert parity.assert_segment(ev, s, orc, "stream %d tune %d" % (s, hz)) > 0
        assert parity.decoded(orc) == [s]


def test_input_tune_acts_on_the_corrected_row():
    """25/16, S16: stream 1 has an input-rate tune of +900 kHz ahead of the resampler, stream 0 none; one shared row."""
    fmt, p, q, k, sizes, freqs = "s16", 25, 16, 64, (1, 2), (0, 900000)
    rows = scene(fmt, p, q, 3, freqs, 1)
    (x, d), = corrected(rows, fmt, k, sizes, p, q)

    def before(r, i):
        if i == 0:
            r.map_streams([0, 1], [0, 0])
            r.tune_streams_input([1], [900000])

    evs, y0, ds, _ = run_dc(rows, sizes, p, q, fmt, k, n_streams=2, dc_rows=1, before=before)
    ev = np.concatenate(evs)
    assert np.array_equal(ds[1][0], d[1])
    for s, hz in enumerate(freqs):
        w0 = stage0_of_x(x, p, q, hz)
        parity.assert_stage0(y0, sizes, w0, s)
        orc = oracle_of(w0)
        assert parity.assert_segment(ev, s, orc, "stream %d input tune %d" % (s, hz)) > 0
        assert parity.decoded(orc) == [s]


def test_more_rows_than_max_rows_are_refused_and_nothing_is_queued():
    import torch

    rows = scene("u8", 1, 1, 3)[:, :api.BLOCK_BYTES]
    d_rows = torch.from_numpy(np.ascontiguousarray(rows)).to("cuda:0")
    with api.Receiver(2, TYPES, THRESH, 0, max_blocks=1, all_flushes=True, dc_windows=64, dc_rows=1) as r:
        for part in (d_rows, np.ascontiguousarray(rows)):  # two rows in use, one allowed
            with pytest.raises(api.TfrecAmdError) as e:
                r.submit(part)
            assert e.value.code == api.E_INVAL
        with pytest.raises(api.TfrecAmdError) as e:
            r.read_dc(0)  # nothing was queued
        assert e.value.code == api.E_STATE and len(r.drain()) == 0
        r.map_streams([1], [0])
        assert r.submit(d_rows[:1]) == 1
        want, = corrected(rows[:1], "u8", 64, (1,))
        assert np.array_equal(r.read_dc(0), want[1][0])  # the row's first window ever: the refused submits left no state
        ev = r.drain()
        for s in range(2):
            assert parity.assert_segment(ev, s, oracle_of(want[0]), "stream %d" % s) > 0


def test_reset_dc_rows_on_one_of_two_rows():
    fmt, k, sizes = "u8", 100, (1, 1, 1)
    rows = scene(fmt, 1, 1, 3)
    want = corrected(rows, fmt, k, sizes, reset_before={1: (1,)})
    carried = corrected(rows, fmt, k, sizes)
    evs, y0, ds, _ = run_dc(rows, sizes, 1, 1, fmt, k,
                            before=lambda r, i: (r.reset_dc_rows([1, 1]), r.reset_dc_rows([])) if i == 1 else None)  # a duplicate; n == 0
    ev = np.concatenate(evs)
    for s in range(2):
        for i in range(3):
            assert np.array_equal(ds[i][s], want[s][1][i]), (s, i)
        parity.assert_stage0(y0, sizes, want[s][0], s)
        # the streams were not restarted: one oracle over the whole row
        assert parity.assert_segment(ev, s, oracle_of(want[s][0]), "stream %d" % s) > 0
    assert np.array_equal(want[0][1][1], carried[0][1][1]) and not np.array_equal(want[1][1][1], carried[1][1][1])
    assert np.array_equal(want[1][1][1][0], dcblock.dc_block(rows[1][api.BLOCK_BYTES:2 * api.BLOCK_BYTES], fmt, k)[1][0])


def test_a_stream_reset_leaves_the_estimate_unchanged():
    fmt, p, q, k, sizes = "s16", 25, 16, 100, (1, 2)
    rows = scene(fmt, p, q, 3)
    want = corrected(rows, fmt, k, sizes, p, q)
    evs, y0, ds, _ = run_dc(rows, sizes, p, q, fmt, k, before=lambda r, i: r.reset_streams([0]) if i == 1 else None)
    cut = 2 * dcblock.input_samples(1, p, q)
    for s in range(2):
        for i in range(2):
            assert np.array_equal(ds[i][s], want[s][1][i]), (s, i)
    # stream 0 restarts on the corrected samples behind the cut, from a history of x = 0; stream 1 runs on
    x0 = want[0][0]
    first, second = stage0_of_x(x0[:cut], p, q), stage0_of_x(x0[cut:], p, q)
    assert np.array_equal(y0[0][0], first) and np.array_equal(y0[1][0], second)
    assert parity.assert_segment(evs[0], 0, oracle_of(first), "stream 0 before the reset") + \
        parity.assert_segment(evs[1], 0, oracle_of(second), "stream 0 after the reset") > 0
    parity.assert_stage0(y0, sizes, stage0_of_x(want[1][0], p, q), 1)
    assert parity.assert_segment(np.concatenate(evs), 1, oracle_of(stage0_of_x(want[1][0], p, q)), "stream 1") > 0


def test_two_submits_queued_before_the_first_read():
    fmt, k, sizes = "u8", 4, (1, 2)
    rows = scene(fmt, 1, 1, 3)
    want = corrected(rows, fmt, k, sizes)
    parts = parity.to_device(parity.cut_input(rows, sizes, fmt))
    with api.Receiver(2, TYPES, THRESH, 0, max_blocks=2, all_flushes=True, dc_windows=k) as r:
        for part in parts:
            r.submit(part)
        evs = []
        for i in range(2):
            for s in range(2):
                assert np.array_equal(r.read_dc(s), want[s][1][i]), (i, s)
                assert np.array_equal(r.read_dc(s), want[s][1][i])  # reading pops nothing
            evs.append(r.drain())
        with pytest.raises(api.TfrecAmdError) as e:
            r.read_dc(0)
        assert e.value.code == api.E_STATE
    for s in range(2):
        assert parity.assert_segment(np.concatenate(evs), s, oracle_of(want[s][0]), "stream %d" % s) > 0


def test_submit_host_equals_submit_device():
    fmt, p, q, k, sizes = "f32", 4, 3, 64, (3,)
    rows = scene(fmt, p, q, 3)
    a = run_dc(rows, sizes, p, q, fmt, k)
    b = run_dc(rows, sizes, p, q, fmt, k, host=True)
    assert len(a[0][0]) > 0 and parity.sort_events(a[0][0]).tobytes() == parity.sort_events(b[0][0]).tobytes()
    for s in range(2):
        assert np.array_equal(a[1][0][s], b[1][0][s]) and np.array_equal(a[2][0][s], b[2][0][s])


# ---- beside the side outputs
def test_side_outputs_equal_an_s16_context_on_the_corrected_rows():
    """The identity the wiring rests on: a DC context on the raw rows is an S16 context on x' << 2 -- events, levels and captures
    byte for byte; and the spectrum, which reads the caller's raw rows, equals that of a context without the blocker."""
    fmt, p, q, k, sizes = "u8", 1, 1, 64, (2, 1)
    rows = scene(fmt, p, q, 3)
    want = corrected(rows, fmt, k, sizes)
    xrows = np.stack([formats.encode("s16", x) for x, _ in want])
    got = {}
    for name, kw, data, f in (("dc", dict(input_format=fmt, dc_windows=k), rows, fmt), ("s16", dict(input_format="s16"), xrows, "s16"),
                              ("raw", dict(), rows, fmt)):
        out = []
        with api.Receiver(2, TYPES, THRESH, 0, max_blocks=2, all_flushes=True, levels=True, **kw) as r:
            r.enable_capture(4096, 2 * 2 * api.BLOCK_DEC)
            r.enable_spectrum(256, 16)
            for part in parity.to_device(parity.cut_input(data, sizes, f)):
                r.submit(part)
                out.append((r.read_levels().tobytes(), [a.tobytes() for a in r.read_captures()], [[a.tobytes() for a in r.read_spectrum(s)] for s in range(2)],
                            parity.sort_events(r.drain()).tobytes()))
        got[name] = out
    for i in range(2):
        assert got["dc"][i][0] == got["s16"][i][0] and got["dc"][i][1] == got["s16"][i][1] and got["dc"][i][3] == got["s16"][i][3]
        assert got["dc"][i][2] == got["raw"][i][2] and got["dc"][i][2] != got["s16"][i][2]
    events = {name: b"".join(o[3] for o in out) for name, out in got.items()}
    assert len(events["dc"]) > 0 and events["dc"] != events["raw"] and len(got["dc"][0][1][0]) > 0


def test_memory_counts_everything_the_blocker_holds():
    n, nb, k, rows = 4, 3, 100, 3
    for p, q, fmt in ((1, 1, "u8"), (25, 16, "f32")):
        with api.Receiver(n, TYPES, THRESH, 0, max_blocks=nb, input_format="s16", input_rate=(p, q)) as r:
            base = r.memory()
        with api.Receiver(n, TYPES, THRESH, 0, max_blocks=nb, input_format=fmt, input_rate=(p, q), dc_windows=k, dc_rows=rows) as r:
            mem = r.memory()
        n_max = nb * 32768 * p // q
        assert n_max % 512 == 0
        per_set = rows * n_max * 4 + rows * (n_max // 512) * 4  # the corrected rows and the table of d
        per_ctx = rows * k * 8 + rows * (n_max // 512) * 8 + rows * 8  # the ring, a submit's sums, the counts
        assert mem["device_bytes"] - base["device_bytes"] == api.FIFO_DEPTH * per_set + per_ctx, (p, q)
        assert mem["pinned_host_bytes"] == base["pinned_host_bytes"]


# ---- refusals
def test_refusals_and_argument_errors():
    L = api.load_library()
    C = api.C
    h = C.c_void_p()
    cfg = api.Config(2, TYPES, THRESH, 0, 0, 1, 4096, api.F_INPUT_10X)
    assert L.tfrec_amd_create_dc(C.byref(cfg), 0, 1, 1, 64, 2, C.byref(h)) == api.E_INVAL and not h  # the 15.36 MS/s input
    with pytest.raises(api.TfrecAmdError) as e:
        api.Receiver(2, TYPES, THRESH, 0, max_blocks=1, input_10x=True, dc_windows=64)
    assert e.value.code == api.E_INVAL
    for kw in (dict(dc_windows=0), dict(dc_windows=4097), dict(dc_windows=64, dc_rows=0), dict(dc_windows=64, dc_rows=3),
               dict(dc_windows=64, input_format="x16"), dict(dc_windows=64, input_rate=(1, 2)), dict(dc_windows=2 ** 31)):
        with pytest.raises(api.TfrecAmdError) as e:
            api.Receiver(2, TYPES, THRESH, 0, max_blocks=1, **kw)
        assert e.value.code == api.E_INVAL, kw
    rows = scene("u8", 1, 1, 3)[:, :api.BLOCK_BYTES]
    with api.Receiver(2, TYPES, THRESH, 0, max_blocks=1, all_flushes=True) as r:  # a context without the blocker
        assert r.dc() == (0, 0)
        r.submit(np.ascontiguousarray(rows))
        for call in (lambda: r.read_dc(0), lambda: r.reset_dc_rows([0]), lambda: r.reset_dc_rows([])):
            with pytest.raises(api.TfrecAmdError) as e:
                call()
            assert e.value.code == api.E_INVAL
        r.drain()
    with api.Receiver(2, TYPES, THRESH, 0, max_blocks=1, all_flushes=True, dc_windows=64) as r:
        assert r.dc() == (64, 2)
        nw = C.c_int(7)
        assert L.tfrec_amd_read_dc(r.h, 0, None, 0, C.byref(nw)) == api.E_STATE and nw.value == 0  # nothing undrained
        for bad in ([2], [-1], [0, 5]):
            with pytest.raises(api.TfrecAmdError) as e:
                r.reset_dc_rows(bad)
            assert e.value.code == api.E_INVAL
        assert L.tfrec_amd_reset_dc_rows(r.h, None, 1) == api.E_INVAL and L.tfrec_amd_reset_dc_rows(r.h, None, -1) == api.E_INVAL
        r.submit(np.ascontiguousarray(rows))
        want = corrected(rows, "u8", 64, (1,))  # (the refused [0, 5] marked nothing: row 0's estimate is a first submit's)
        d = np.full((64, 2), 77, dtype=np.int16)
        assert L.tfrec_amd_read_dc(r.h, 0, d.ctypes.data, 63, C.byref(nw)) == api.E_INVAL and nw.value == 64 and (d == 77).all()
        assert L.tfrec_amd_read_dc(r.h, 0, None, 64, C.byref(nw)) == api.E_INVAL and nw.value == 64
        assert L.tfrec_amd_read_dc(r.h, 0, d.ctypes.data, 64, None) == api.E_INVAL
        for bad in (2, -1):
            with pytest.raises(api.TfrecAmdError) as e:
                r.read_dc(bad)
            assert e.value.code == api.E_INVAL
        assert L.tfrec_amd_read_dc(r.h, 1, d.ctypes.data, 64, C.byref(nw)) == api.E_OK and np.array_equal(d, want[1][1][0])
        ev = r.drain()
        assert parity.assert_segment(ev, 0, oracle_of(want[0][0]), "stream 0") > 0


# ---- tfrec_gpu -z
def test_cli_decodes_the_offset_scene_with_z_and_not_without(tmp_path):
    """tfrec_gpu -z -T 2f -t 500 on the golden TFA_2 scene with an offset of (8, -4) u8 LSB prints the clean scene's two telegrams;
    without -z it prints none.  -D (whose decoders print their debug form of a telegram): a dc line per submit with the restatement's
    last estimate."""
    cli = parity.build_cli()
    _, clean = golden_scene("tfa_2")
    f = tmp_path / "offset.iq"
    off = offset_scene("tfa_2")
    off.tofile(f)
    want = parity.telegram_lines(clean)
    assert len(want) == 2
    out = subprocess.run([cli, "-z", "-T", "2f", "-t", "500", "-L", str(f)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    assert parity.telegram_lines(out.stdout) == want
    out = subprocess.run([cli, "-T", "2f", "-t", "500", "-L", str(f)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and parity.telegram_lines(out.stdout) == []
    out = subprocess.run([cli, "-z", "64", "-D", "-b", "4", "-T", "2f", "-t", "500", "-L", str(f)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    d = dcblock.dc_block(off, "u8", 64)[1]
    assert [ln for ln in out.stdout.splitlines() if ln.startswith("dc ")] == ["dc %s I=%d Q=%d" % (f, d[-1, 0], d[-1, 1])]


def test_cli_queue_mode_starts_a_new_estimate_with_a_new_file(tmp_path):
    """tfrec_gpu -n 1: two files go through one stream, one after the other.  At K = 4096 -- longer than both -- the second file's last
    estimate is the mean over that file alone only if the slot's row was reset with its stream."""
    cli = parity.build_cli()
    files, want = [], []
    for name, d in (("tfa_2", OFFSET), ("tfa_1", (-6, 9))):
        f = tmp_path / ("%s.iq" % name)
        off = offset_scene(name, d)
        off.tofile(f)
        est = dcblock.dc_block(off, "u8", 4096)[1]
        files += ["-L", str(f)]
        want.append("dc %s I=%d Q=%d" % (f, est[-1, 0], est[-1, 1]))
    out = subprocess.run([cli, "-z", "4096", "-D", "-n", "1", "-b", "4", "-T", "2f", "-t", "500"] + files, capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0, out.stderr
    assert [ln for ln in out.stdout.splitlines() if ln.startswith("dc ")] == want
