"""The input-rate tune on the GPU (tfrec_amd_tune_streams_input, tfrec_gpu -r with -f), bit for bit.

Stage 0 is pinned by the restatement (tune.mix_in_s16, resample.resample_x16), everything behind it by the oracle's process_s16 fed
that restatement's output.  The scenes are input_rows.py's recordings at 2.4 MS/s (25/16) and 3.2 MS/s (25/12); test_input_tune_cpu.py
asserts that the oracle decodes each burst for exactly the receiver tuned to it."""
import functools

import numpy as np
import pytest

import parity
from input_rows import THRESH, TYPES, WIDE_BURSTS, WIDE_ROW_BLOCKS, WIDE_SCENES, input_oracle, oracle_of, tuned_stage0, wide_row, wide_scene
from tfrec_amd import api, resample

pytestmark = pytest.mark.gpu

run_input = functools.partial(parity.run_input, types=TYPES, thresh=THRESH)
SIZES = {(25, 16): (1, 2, 2, 1), (25, 12): (3, 3)}  # the scenes' WIDE_ROW_BLOCKS blocks cut into submits


def receivers(p, q):
    """before(r, k) of a run that maps one receiver per burst of the scene to row 0 and tunes it there at the input rate."""
    freqs = WIDE_SCENES[p, q]
    idx = list(range(len(freqs)))

    def before(r, k):
        if k == 0:
            r.map_streams(idx, [0] * len(idx))
            r.tune_streams_input(idx, freqs)
            assert r.rows_in_use == 1 and [r.stream_tune_input(s) for s in idx] == list(freqs)

    return freqs, before


@pytest.mark.parametrize("p,q,sizes", [(4, 3, (3, 3, 3, 3)), (25, 16, (1, 2, 1, 2)), (25, 12, (3, 3, 3, 3)), (639, 64, (1, 1, 1, 1))])
def test_stage0_equals_the_restatement(p, q, sizes):
    """Four submits: the history carry, both history buffers and the phase carry; a tuned stream near the limit, an untuned one and
    a second tuned one in one launch.  639/64 takes the kernel's half tile."""
    top = (1536000 * p + 2 * q - 1) // (2 * q) - 1
    hz = (top - 1234, 0, -123457)
    iq = parity.loud_and_quiet(p, q, sizes, 3, 1000 * p + q)

    def before(r, k):
        if k == 0:
            r.tune_streams_input([0, 1, 2], hz)

    _, y0 = run_input(iq, sizes, p, q, before=before, all_flushes=True, max_events=1 << 16)
    for s in range(3):
        want = tuned_stage0(iq[s], p, q, hz[s])
        if hz[s] == 0:
            assert np.array_equal(want, resample.resample_s16(iq[s], p, q))
        parity.assert_stage0(y0, sizes, want, s)


@pytest.mark.parametrize("p,q", [(25, 16), (639, 64)])
def test_an_untuned_stream_keeps_its_history_while_the_kernels_change_around_it(p, q):
    """A u8 rate context runs the plain resampler while no stream is tuned and the format kernel's U8 instantiation while one is.
    Stream 0 is tuned before the second submit and untuned again before the third -- each a restart of stream 0 alone --, so
    stream 1, never tuned and never restarted, has its history written by one kernel and read by the other, in both directions:
    its stage 0 is that of the uninterrupted input.  25/16 takes the whole tile, 639/64 the half tile."""
    sizes = (1, 1, 1)
    hz = 300000
    iq = parity.loud_and_quiet(p, q, sizes, 2, 7000 * p + q)

    def before(r, k):
        if k == 1:
            r.tune_streams_input([0], [hz])
        if k == 2:
            r.tune_streams_input([0], [0])

    _, y0 = run_input(iq, sizes, p, q, before=before, all_flushes=True, max_events=1 << 16)
    assert np.array_equal(np.concatenate([y[1] for y in y0]), resample.resample_s16(iq[1], p, q))
    c1 = 2 * resample.input_samples(1, p, q)
    assert np.array_equal(y0[1][0], tuned_stage0(iq[0][c1:], p, q, hz)[:len(y0[1][0])])  # (the tuned kernel did run in between)


@pytest.mark.parametrize("p,q", sorted(WIDE_SCENES))
@pytest.mark.parametrize("mode", ["deep", "shallow", "serial_chains", "default_mode", "bits", "host"])
def test_events_equal_the_oracle_behind_the_restatement(mode, p, q, monkeypatch):
    kw, _, flags = parity.mode_kwargs(mode, monkeypatch)
    row = wide_row(p, q)
    freqs, before = receivers(p, q)
    evs, _ = run_input(row, SIZES[p, q], p, q, host=flags["host"], stage0=False, n_streams=len(freqs), before=before, **kw)
    ev = np.concatenate(evs)
    total = 0
    for s, f in enumerate(freqs):
        orc = input_oracle(row[0], p, q, f, log_bits=flags["bits"])
        total += parity.assert_stream(ev, s, orc, "stream %d tune %d" % (s, f), default_mode=flags["default_mode"])
        if flags["bits"]:
            assert parity.assert_bits(ev, s, orc, "stream %d" % s) > 50
        assert parity.decoded(orc) == [s]  # a telegram per tuned receiver: its own burst
        assert [t[0] for t in api.event_tuples_full(ev, s) if t[7] == 1] == [s]
    assert total >= len(freqs)


@pytest.mark.parametrize("p,q", sorted(WIDE_SCENES))
def test_results_do_not_depend_on_the_cut(p, q):
    row = wide_row(p, q)
    freqs, before = receivers(p, q)
    one, _ = run_input(row, (WIDE_ROW_BLOCKS,), p, q, n_streams=len(freqs), before=before, all_flushes=True)
    cut, _ = run_input(row, SIZES[p, q], p, q, n_streams=len(freqs), before=before, all_flushes=True)
    a, b = parity.sort_events(np.concatenate(one)), parity.sort_events(np.concatenate(cut))
    assert len(a) >= len(freqs) and a.tobytes() == b.tobytes()


def test_a_tune_and_a_reset_in_mid_stream_equal_fresh_receivers():
    """Stream 0 is tuned before the second submit, stream 1 (tuned from the start) is reset before the third: each part equals a
    fresh receiver on the truncated input, the phase restarting at the restart; a reset keeps the tune."""
    p, q = 25, 16
    x = wide_row(p, q)[0]
    f0, f1 = WIDE_SCENES[p, q][2], WIDE_SCENES[p, q][3]
    sizes = (2, 2, 2)

    def before(r, k):
        if k == 0:
            r.tune_streams_input([1], [f1])
        if k == 1:
            r.tune_streams_input([0], [f0])
        if k == 2:
            r.reset_streams([1])
            assert r.stream_tune_input(1) == f1

    evs, y0 = run_input(np.stack([x, x]), sizes, p, q, before=before, all_flushes=True)
    c1, c2 = 2 * resample.input_samples(2, p, q), 2 * resample.input_samples(4, p, q)
    parity.assert_segment(np.concatenate(evs[:1]), 0, oracle_of(x[:c1], p, q), "stream 0 before its tune")
    n = parity.assert_segment(np.concatenate(evs[1:]), 0, input_oracle(x[c1:], p, q, f0), "stream 0 after its tune")
    n += parity.assert_segment(np.concatenate(evs[:2]), 1, input_oracle(x[:c2], p, q, f1), "stream 1 before the reset")
    n += parity.assert_segment(np.concatenate(evs[2:]), 1, input_oracle(x[c2:], p, q, f1), "stream 1 after the reset")
    assert n > 0
    assert np.array_equal(y0[0][0], resample.resample_s16(x, p, q)[:len(y0[0][0])])
    assert np.array_equal(y0[1][0], tuned_stage0(x[c1:], p, q, f0)[:len(y0[1][0])])  # zero history and phase 0 behind the cut
    assert np.array_equal(y0[2][1], tuned_stage0(x[c2:], p, q, f1)[:len(y0[2][1])])
    assert np.array_equal(y0[1][1], tuned_stage0(x, p, q, f1)[len(y0[0][1]):][:len(y0[1][1])])  # stream 1 carried on there


@pytest.mark.parametrize("p,q", sorted(WIDE_SCENES))
def test_receivers_of_one_row_equal_receivers_of_copies(p, q):
    row = wide_row(p, q)
    freqs, shared = receivers(p, q)
    k3 = [0, len(freqs) - 2, len(freqs) - 1]  # the centre and two more, one of them beyond +-768 kHz
    hz = [freqs[j] for j in k3]
    assert any(abs(f) > 768000 for f in hz)

    def one_row(r, k):
        if k == 0:
            r.map_streams([0, 1, 2], [0, 0, 0])
            r.tune_streams_input([0, 1, 2], hz)
            assert r.rows_in_use == 1

    def copies(r, k):
        if k == 0:
            r.tune_streams_input([0, 1, 2], hz)
            assert r.rows_in_use == 3

    ev_shared, y0 = run_input(row, SIZES[p, q], p, q, n_streams=3, before=one_row, all_flushes=True)
    ev_copies, y0c = run_input(np.repeat(row, 3, axis=0), SIZES[p, q], p, q, before=copies, all_flushes=True)
    a, b = parity.sort_events(np.concatenate(ev_shared)), parity.sort_events(np.concatenate(ev_copies))
    assert a.tobytes() == b.tobytes()
    for s in range(3):
        orc = input_oracle(row[0], p, q, hz[s])
        parity.assert_segment(a, s, orc, "stream %d tune %d" % (s, hz[s]))
        assert parity.decoded(orc) == [k3[s]]  # each receiver decodes only its own burst
        assert [t[0] for t in api.event_tuples_full(a, s) if t[7] == 1] == [k3[s]]
        for k in range(len(y0)):
            assert np.array_equal(y0[k][s], y0c[k][s])


def test_the_tune_behind_the_resampler_composes():
    """tune_streams acts on the shifted, resampled y0: 900 kHz ahead of the stage and 200 kHz behind it reach the burst at 1.1 MHz."""
    p, q = 25, 16
    row = wide_row(p, q)
    pairs = ((900000, 200000), (-600000, -450000), (0, 300000))
    want = (2, 3, 1)
    assert [a + b for a, b in pairs] == [WIDE_SCENES[p, q][j] for j in want]

    def before(r, k):
        if k == 0:
            r.map_streams([0, 1, 2], [0, 0, 0])
            r.tune_streams([0, 1, 2], [b for _, b in pairs])
            r.tune_streams_input([0, 1, 2], [a for a, _ in pairs])
            assert [r.stream_tune(s) for s in range(3)] == [b for _, b in pairs]

    evs, y0 = run_input(row, SIZES[p, q], p, q, n_streams=3, before=before, all_flushes=True)
    ev = np.concatenate(evs)
    for s, (a, b) in enumerate(pairs):
        orc = input_oracle(row[0], p, q, a, b)
        parity.assert_segment(ev, s, orc, "stream %d" % s)
        assert parity.decoded(orc) == [want[s]]
        assert np.array_equal(y0[0][s], tuned_stage0(row[0], p, q, a)[:len(y0[0][s])])  # stage 0 is ahead of that tune


def test_on_a_10x_context_the_call_is_the_wide_tune():
    iq = wide_scene()[None, :]
    hz = [f for f, _ in WIDE_BURSTS[:3]]
    out = []
    for name in ("tune_streams_wide", "tune_streams_input"):
        with api.Receiver(3, TYPES, THRESH, 0, max_blocks=2, all_flushes=True, input_10x=True) as r:
            r.map_streams([0, 1, 2], [0, 0, 0])
            getattr(r, name)([0, 1, 2], hz)
            assert [r.stream_tune_wide(s) for s in range(3)] == hz == [r.stream_tune_input(s) for s in range(3)]
            evs = parity.run_fifo(r, parity.cut(iq, (2, 2), 10 * api.BLOCK_BYTES))
            out.append(parity.sort_events(np.concatenate(evs)))
            with pytest.raises(api.TfrecAmdError) as e:  # the wide tune's limit
                r.tune_streams_input([0], [7680000])
            assert e.value.code == api.E_INVAL
    assert out[0].tobytes() == out[1].tobytes()
    assert sorted(t[0] for s in range(3) for t in api.event_tuples_full(out[1], s) if t[7] == 1) == [p for _, p in WIDE_BURSTS[:3]]


def test_a_plain_context_refuses_the_call_and_stays_usable():
    from tfrec_amd import synth

    iq = synth.gen_batch(5, 0, 2, 4)  # (four blocks: the oracle reports four flushes per stream)
    with api.Receiver(2, TYPES, THRESH, 0, max_blocks=4, all_flushes=True) as r:
        with pytest.raises(api.TfrecAmdError) as e:
            r.tune_streams_input([0], [1000])
        assert e.value.code == api.E_INVAL and "tfrec_amd_tune_streams" in str(e.value)
        assert r.stream_tune_input(0) == 0
        r.submit(iq)
        ev = r.drain()
        for s in range(2):
            assert parity.assert_segment(ev, s, parity.fresh_oracle(iq[s], TYPES, THRESH), "stream %d" % s) > 0


def test_error_paths_mark_nothing():
    p, q = 25, 16
    x = wide_row(p, q)
    iq = np.repeat(x, 2, axis=0)
    with api.Receiver(2, TYPES, THRESH, 0, max_blocks=WIDE_ROW_BLOCKS, all_flushes=True, input_rate=(p, q)) as r:
        for streams, hz in (([0, 1], [100, 1200000]), ([0, 1], [100, -1200000]), ([1, 2], [100, 100]), ([-1], [100]),
                            ([0], [2 ** 31 - 1])):
            with pytest.raises(api.TfrecAmdError) as e:
                r.tune_streams_input(streams, hz)
            assert e.value.code == api.E_INVAL
        assert r.L.tfrec_amd_tune_streams_input(r.h, None, None, 1) == api.E_INVAL
        assert r.L.tfrec_amd_tune_streams_input(r.h, None, None, -1) == api.E_INVAL
        assert r.L.tfrec_amd_tune_streams_input(r.h, None, None, 0) == api.E_OK
        with pytest.raises(api.TfrecAmdError) as e:  # still refused on a rate context, and the text names the call to use
            r.tune_streams_wide([0], [1000])
        assert e.value.code == api.E_INVAL and "tfrec_amd_tune_streams_input" in str(e.value)
        assert [r.stream_tune_input(s) for s in range(2)] == [0, 0]
        r.tune_streams_input([0, 0], [5, 1199999])  # the limit itself; the last value wins
        assert r.stream_tune_input(0) == 1199999
        r.tune_streams_input([0], [0])
        r.submit(iq)
        ev = r.drain()
        for s in range(2):  # nothing but tune 0 was marked: both are the untuned receiver
            assert parity.assert_segment(ev, s, oracle_of(iq[s], p, q), "stream %d" % s) > 0
        assert np.array_equal(r.stage0(0, 64), resample.resample_s16(iq[0], p, q)[:128])


def test_memory_is_what_it_was_with_and_without_a_tune():
    with api.Receiver(4, TYPES, THRESH, 0, max_blocks=3) as r:
        plain = r.memory()["device_bytes"]
    with api.Receiver(4, TYPES, THRESH, 0, max_blocks=3, input_rate=(25, 16)) as r:
        rate = r.memory()
        # stage 0 (one buffer per set), the int16 FIR history instead of the u8 one, two raw histories, the tap table
        assert rate["device_bytes"] - plain == api.FIFO_DEPTH * 4 * 4 * 3 * api.BLOCK_DEC * 4 + 2 * 4 * 112 + 2 * 4 * 128 + 16 * 10 * 4
        r.tune_streams_input([0, 2], [900000, -1100000])
        assert r.memory() == rate
        import torch

        iq = torch.full((4, r.input_bytes(3)), 128, dtype=torch.uint8, device="cuda:0")
        r.submit(iq, 3)
        r.drain()
        assert r.memory() == rate


@pytest.fixture(scope="module")
def cli():
    return parity.build_cli()


def test_cli_one_2400000_dump_given_three_times(cli, tmp_path):
    """tfrec_gpu -r 2400000: one file given three times with three f=, one of them beyond 767 kHz, prints the concatenation of the
    three single-file runs, and hands the sink the same records with the -L occurrence as stream index."""
    p, q = 25, 16
    w = tmp_path / "w.iq"
    wide_row(p, q)[0].tofile(w)
    c = 868250
    fs = [c + f // 1000 for f in WIDE_SCENES[p, q][:3]]
    assert fs[2] - c > 767
    base = ["-r", "2400000", "-c", str(c), "-T", "%x" % TYPES, "-t", str(THRESH), "-b", "2"]
    singles = [parity.cli(base + ["-p", "f=%d" % f, "-L", str(w)], str(tmp_path / ("s%d.txt" % i))) for i, f in enumerate(fs)]
    args = list(base)
    for f in fs:
        args += ["-p", "f=%d" % f, "-L", str(w)]
    out, rec = parity.cli(args, str(tmp_path / "all.txt"))
    assert out == "".join(s[0] for s in singles) and len(out.splitlines()) >= 3
    assert rec == [[str(i)] + r[1:] for i, s in enumerate(singles) for r in s[1]] and len(rec) >= 3
    for i, f in enumerate(WIDE_SCENES[p, q][:3]):  # ... and each is the oracle's text behind the restatement
        o = input_oracle(wide_row(p, q)[0], p, q, f) if abs(f) >= 768000 else input_oracle(wide_row(p, q)[0], p, q, 0, f)
        want, got = parity.telegram_lines(o.text()), parity.telegram_lines(singles[i][0])
        assert got == want and len(want) >= 1, i


def test_cli_one_slot_changes_tune_kind_near_far_near(cli, tmp_path):
    """tfrec_gpu -r 2400000 -n 1: the same file three times through ONE stream, tuned near, far, near -- the slot goes from the tune
    behind the resampler to the input-rate tune and back, the other kind cleared each time.  Stdout is the three single-file runs
    one after the other, and the sink's records are theirs with the file index as stream."""
    p, q = 25, 16
    w = tmp_path / "w.iq"
    wide_row(p, q)[0].tofile(w)
    c = 868250
    fs = [c + f // 1000 for f in WIDE_SCENES[p, q][:3]]
    fs = [fs[0], fs[2], fs[1]]
    assert [abs(f - c) > 767 for f in fs] == [False, True, False]
    base = ["-r", "2400000", "-c", str(c), "-T", "%x" % TYPES, "-t", str(THRESH), "-b", "2"]
    singles = [parity.cli(base + ["-p", "f=%d" % f, "-L", str(w)], str(tmp_path / ("s%d.txt" % i))) for i, f in enumerate(fs)]
    args = base + ["-n", "1"]
    for f in fs:
        args += ["-p", "f=%d" % f, "-L", str(w)]
    out, rec = parity.cli(args, str(tmp_path / "all.txt"))
    assert out == "".join(s[0] for s in singles) and len(out.splitlines()) >= 3
    assert rec == [[str(i)] + r[1:] for i, s in enumerate(singles) for r in s[1]] and len(rec) >= 3
