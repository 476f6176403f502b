"""Shared inputs and the wideband tune on the GPU (tfrec_amd_map_streams, tfrec_amd_tune_streams_wide, tfrec_gpu -x; DESIGN.md
6e), against the oracle, bit for bit.

A receiver's events (every field, seq included), decimated samples and threshold equal those of a fresh oracle fed the input of
the ROW the receiver reads, from the receiver's own restart on -- segments.py's scheme with the row looked up
through the map.  With the 10x input the oracle is fed tune.decim10_s16(tune.mix10_s16(...)) of the segment, and stage0() equals
it too."""
import numpy as np
import pytest

import parity
import segments
from input_rows import CFGS, DFLT, EMPTY_HZ, ROW_TUNES, ROWS, WIDE_BURSTS, WIDE_SCENE_BLOCKS, make_rows, wide_scene
from parity import device_parts
from tfrec_amd import api, synth, tune

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("mode", ["deep", "shallow", "serial_chains", "bits"])
def test_shared_rows(mode, monkeypatch):
    """24 receivers on 6 rows with mixed tunes and settings, ragged submits through the full FIFO; remaps, resets, retunes and
    reconfigures between the submits.  The batch holds the 6 rows only."""
    kw, layout, flags = parity.mode_kwargs(mode, monkeypatch)
    n = 24
    sizes = (3, 2, 1, 3, 2)
    iq = make_rows(51, sum(sizes))
    rows0 = [s % ROWS for s in range(n)]
    tunes = [ROW_TUNES[s % ROWS][s // ROWS] for s in range(n)]
    conf = sorted(CFGS)
    ops = {0: [("map", list(range(n)), rows0), ("tune", list(range(n)), tunes), ("conf", conf, [CFGS[s] for s in conf])],
           # a remap with the new row's tune, a map to the row already read, a reset beside them
           1: [("map", [3, 9, 9], [5, 0, 1]), ("tune", [3, 9], [-500000, 767999]), ("map", [6], [0]), ("reset", [11])],
           # one restart out of a reset, a configure, a tune and a map
           3: [("reset", [2]), ("conf", [2], [(0x2F, 500, 0)]), ("tune", [2], [0]), ("map", [2], [4]), ("tune", [16], [31])],
           4: [("reset", [3, 20]), ("map", [0], [5])]}
    with api.Receiver(n, DFLT[0], DFLT[1], DFLT[2], max_blocks=max(sizes), **kw) as r:
        assert r.layout() == layout
        parts, hosts = device_parts(iq, sizes)
        total, segs = segments.run_segments(r, parts, ops, DFLT, hosts=hosts, bits=flags["bits"])
        assert [r.stream_input(s) for s in (0, 2, 3, 6, 9)] == [5, 4, 5, 0, 1]
    assert [len(segs[s]) for s in (0, 2, 3, 6, 9, 11, 16, 20, 1)] == [2, 2, 3, 2, 2, 2, 2, 2, 1]
    assert total > 5 * n
    ok = [g for s in range(n) for g in segs[s] if any(e[7] == 1 for e in g.orc.events_full())]
    assert len(ok) >= n // 2  # the planted bursts decode: the comparison is not one of empty lists


def wide_parts(sizes):
    iq = wide_scene()
    return iq, device_parts(iq[None, :], sizes, api.BLOCK_BYTES * 10)


def test_wideband_receivers_of_one_row():
    """The CPU test's scene on ONE row of a 10x context: a receiver per planted offset, one on an empty frequency, an untuned
    one, one that combines a wide tune with a 1.536 MS/s tune, the two limits; a restart in mid-stream."""
    sizes = (1, 2, 1)
    assert sum(sizes) == WIDE_SCENE_BLOCKS
    wides = [f for f, _ in WIDE_BURSTS] + [EMPTY_HZ, 0, 3300000 - 200000, 7679999, -7679999]
    n = len(wides)
    tunes = [0] * n
    tunes[6] = 200000  # 3.1 MHz + 200 kHz: the burst at 3.3 MHz
    _, (parts, hosts) = wide_parts(sizes)
    ops = {0: [("map", list(range(n)), [0] * n), ("wide", list(range(n)), wides), ("tune", [6], [200000])],
           2: [("wide", [1, 4], [-1100000, 6900000]), ("reset", [2])]}  # (stream 1: the same tune again is a restart too)
    with api.Receiver(n, DFLT[0], DFLT[1], DFLT[2], max_blocks=max(sizes), all_flushes=True, input_10x=True) as r:
        total, segs = segments.run_segments(r, parts, ops, DFLT, hosts=hosts, in10x=True)
    assert [len(g) for g in segs] == [1, 2, 2, 1, 2, 1, 1, 1, 1]
    tel = [[e[0] for e in g[0].orc.events_full() if e[7] == 1] for g in segs]  # telegrams of every receiver's first segment
    # a telegram per planted burst (receivers 1 and 2 restart behind theirs), none on the empty frequency, untuned, at the limits
    assert tel[:4] == [[0], [1], [2], [3]] and tel[6] == [2], tel
    assert tel[4] == [] and tel[5] == [] and tel[7] == [] and tel[8] == [], tel
    assert total > n


def test_an_untuned_stream_keeps_its_history_while_the_10x_kernels_change_around_it():
    """A 10x context runs the plain 10:1 kernel while no stream has a wide tune and the tuned one while one has.  Stream 0 is tuned
    before the second submit and untuned again before the third -- each a restart of stream 0 alone --, so stream 1, never tuned
    and never restarted, has its history written by one kernel and read by the other, in both directions: its stage 0 is that of
    the uninterrupted input.  (Near-silence with full-scale stretches at the start and across the two boundaries.)"""
    block = 10 * api.BLOCK_BYTES
    rng = np.random.default_rng(53)
    iq = rng.integers(125, 132, (2, 3 * block), dtype=np.uint8)
    for pos in (0, block, 2 * block):
        lo, hi = max(0, pos - 3000), pos + 3000
        iq[:, lo:hi] = rng.integers(0, 256, (2, hi - lo), dtype=np.uint8)
    devs, _ = device_parts(iq, (1, 1, 1), block)
    y = []
    with api.Receiver(2, DFLT[0], DFLT[1], DFLT[2], max_blocks=1, all_flushes=True, input_10x=True) as r:
        for k, d in enumerate(devs):
            if k == 1:
                r.tune_streams_wide([0], [3300000])
            if k == 2:
                r.tune_streams_wide([0], [0])
            r.submit(d, 1)
            r.drain()
            y.append([r.stage0(s, 4 * api.BLOCK_DEC) for s in range(2)])
    assert np.array_equal(np.concatenate([v[1] for v in y]), tune.decim10_s16(tune.s16_of_u8(iq[1])))
    want0 = tune.decim10_s16(tune.mix10_s16(tune.s16_of_u8(iq[0][block:2 * block]), 3300000))
    assert np.array_equal(y[1][0], want0)  # (the tuned kernel did run in between)


def test_wide_tune_needs_the_10x_input_and_argument_errors_change_nothing():
    with api.Receiver(2, DFLT[0], DFLT[1], DFLT[2], max_blocks=1, all_flushes=True) as r:
        with pytest.raises(api.TfrecAmdError) as e:
            r.tune_streams_wide([0], [1000])
        assert e.value.code == api.E_INVAL
        for streams, rows in (([0, 2], [0, 0]), ([0, 1], [0, 2]), ([-1], [0]), ([0], [-1])):
            with pytest.raises(api.TfrecAmdError) as e:
                r.map_streams(streams, rows)
            assert e.value.code == api.E_INVAL
        assert r.L.tfrec_amd_map_streams(r.h, None, None, 1) == api.E_INVAL
        assert r.L.tfrec_amd_map_streams(r.h, None, None, -1) == api.E_INVAL
        assert [r.stream_input(s) for s in range(2)] == [0, 1] and r.rows_in_use == 2
        iq = make_rows(52, 1, rows=2)
        r.submit(iq)
        ev = r.drain()
        for s in range(2):  # nothing was marked: the context is the unmapped one
            parity.assert_segment(ev, s, parity.fresh_oracle(iq[s], *DFLT), "stream %d" % s)
    with api.Receiver(2, DFLT[0], DFLT[1], DFLT[2], max_blocks=1, all_flushes=True, input_10x=True) as r:
        for hz in (7680000, -7680000):
            with pytest.raises(api.TfrecAmdError) as e:
                r.tune_streams_wide([0, 1], [100, hz])
            assert e.value.code == api.E_INVAL
        assert r.L.tfrec_amd_tune_streams_wide(r.h, None, None, 1) == api.E_INVAL
        assert [r.stream_tune_wide(s) for s in range(2)] == [0, 0]


@pytest.mark.parametrize("in10x", [False, True], ids=["default", "input_10x"])
def test_submit_host_copies_only_the_rows_in_use(in10x):
    """R = 2 rows in use of 6: the host path equals the device path on those rows.  The host buffer has all 6 rows; rows 2..5
    hold a DIFFERENT scene with bursts of its own, and no receiver reports any of them."""
    n, rows, nb = 6, 2, 2
    mult = 10 if in10x else 1
    if in10x:
        used = np.stack([wide_scene(seed=61 + j, n_blocks=nb) for j in range(rows)])
        other = synth.gen_scene(77, nb, [dict(proto=1, start=400000, payload_seed=99, f0_hz=0, amp=60)], rate_mult=10)
    else:
        used = make_rows(53, nb, rows=rows)
        other = synth.gen_scene(77, nb, [dict(proto=1, start=40000, payload_seed=99, f0_hz=0, amp=60)])
    o = parity.fresh_oracle(other, *DFLT, in10x=in10x)
    foreign = [e for e in o.events_full() if e[7] == 1]
    assert len(foreign) == 1  # the burst that must not be seen decodes when it IS read
    host = np.concatenate([used, np.stack([other] * (n - rows))])
    import torch

    def run(inp):
        with api.Receiver(n, DFLT[0], DFLT[1], DFLT[2], max_blocks=nb, all_flushes=True, input_10x=in10x) as r:
            r.map_streams(list(range(n)), [s % rows for s in range(n)])
            if in10x:
                r.tune_streams_wide([2, 3], [-1100000, 3300000])
            else:
                r.tune_streams([2, 3], [200000, -250000])
            before = r.memory()["device_bytes"]
            r.submit(inp)
            staged = r.memory()["device_bytes"] - before
            return r.drain(), [r.decimated(s, nb * api.BLOCK_DEC) for s in range(n)], staged

    ev_h, dec_h, staged_h = run(host)
    ev_d, dec_d, staged_d = run(torch.from_numpy(np.ascontiguousarray(host[:rows])).to("cuda:0"))
    assert staged_d == 0 and staged_h == rows * nb * api.BLOCK_BYTES * mult  # the staging buffer holds R rows, not n
    assert len(ev_h) > 0 and ev_h.tobytes() == ev_d.tobytes()
    for s in range(n):
        assert np.array_equal(dec_h[s], dec_d[s])
    assert (ev_h["status"] == 1).sum() > 0
    for s in range(n):
        got = [t for t in api.event_tuples_full(ev_h, s) if t[7] == 1]
        assert all(t[5] != foreign[0][5] for t in got), "stream %d reports the burst of a row it must not read" % s


@pytest.fixture(scope="module")
def cli():
    return parity.build_cli()


def test_cli_wide_file_given_three_times(cli, tmp_path):
    """tfrec_gpu -x: one wide file given three times with three f= prints the concatenation of the three single-file runs, and
    hands the sink the same records with the -L occurrence as stream index."""
    w = tmp_path / "w.iq"
    wide_scene().tofile(w)
    c = 868250
    fs = [c + f // 1000 for f, _ in WIDE_BURSTS[:3]]
    base = ["-x", "-c", str(c), "-T", "2f", "-t", "500", "-b", "2"]
    singles = [parity.cli(base + ["-p", "f=%d" % f, "-L", str(w)], str(tmp_path / ("s%d.txt" % i))) for i, f in enumerate(fs)]
    args = list(base)
    for f in fs:
        args += ["-p", "f=%d" % f, "-L", str(w)]
    out, rec = parity.cli(args, str(tmp_path / "all.txt"))
    assert out == "".join(s[0] for s in singles) and len(out.splitlines()) >= 3
    assert rec == [[str(i)] + r[1:] for i, s in enumerate(singles) for r in s[1]] and len(rec) >= 3


def test_cli_narrow_file_given_three_times(cli, tmp_path):
    """Without -x: a file given three times (now read once, one input row) prints what three separate copies of it print -- the
    run that takes the unshared path, a row per file, as every run did before inputs could be shared."""
    x = make_rows(54, 4, rows=1)[0]
    paths = [tmp_path / ("c%d.iq" % i) for i in range(3)]
    for p in paths:
        x.tofile(p)
    specs = ["f=868250", "f=868450,t=300", "T=2f,f=868000"]
    base = ["-T", "2f", "-t", "500", "-b", "3"]

    def args(files):
        a = list(base)
        for s, f in zip(specs, files):
            a += ["-p", s, "-L", str(f)]
        return a

    want = parity.cli(args(paths), str(tmp_path / "copies.txt"))
    got = parity.cli(args([paths[0]] * 3), str(tmp_path / "shared.txt"))
    assert got == want and len(want[0].splitlines()) >= 3
    # with -n (the files queue for two streams) a repeated file is read per occurrence, as before: the output of the copies
    want_n = parity.cli(["-n", "2"] + args(paths), str(tmp_path / "copies_n.txt"))
    assert parity.cli(["-n", "2"] + args([paths[0]] * 3), str(tmp_path / "shared_n.txt")) == want_n
    assert sorted(want_n[0].splitlines()) == sorted(want[0].splitlines())
