"""The resampling stage on the GPU (tfrec_amd_create_rate, tfrec_gpu -r), bit for bit.

Stage 0 is pinned by the restatement tfrec_amd/resample.py, everything behind it by the oracle's process_s16 fed that
restatement's output.  The scenes are recordings at 2.048 MS/s (4/3) and 2.4 MS/s (25/16); test_resample_cpu.py asserts that
the oracle decodes a telegram of every protocol from them."""
import functools
import subprocess

import numpy as np
import pytest

import parity
from input_rows import SCENE_BLOCKS, SCENE_RATES, THRESH, TYPES, oracle_of, rate_scene
from tfrec_amd import api, resample

pytestmark = pytest.mark.gpu


run_input = functools.partial(parity.run_input, types=TYPES, thresh=THRESH)


@pytest.mark.parametrize("p,q", SCENE_RATES)
def test_stage0_equals_the_restatement(p, q):
    """The first submit and three following ones: the history carry and both history buffers."""
    iq = rate_scene(p, q)
    sizes = (3, 3, 3, 3)
    _, y0 = run_input(iq, sizes, p, q, all_flushes=True)
    for s in range(len(iq)):
        want = resample.resample_s16(iq[s], p, q)
        assert len(want) == 2 * SCENE_BLOCKS * 4 * api.BLOCK_DEC
        parity.assert_stage0(y0, sizes, want, s)


@pytest.mark.parametrize("p,q", SCENE_RATES)
@pytest.mark.parametrize("mode", ["deep", "shallow", "serial_chains", "default_mode", "bits", "host"])
def test_events_equal_the_oracle_behind_the_restatement(mode, p, q, monkeypatch):
    kw, layout, flags = parity.mode_kwargs(mode, monkeypatch)
    iq = rate_scene(p, q)
    layouts = []
    evs, _ = run_input(iq, (3, 3, 3, 3), p, q, host=flags["host"], stage0=False, before=lambda r, k: layouts.append(r.layout()), **kw)
    assert layouts[0] == layout
    ev = np.concatenate(evs)
    total = telegrams = 0
    for s in range(len(iq)):
        orc = oracle_of(iq[s], p, q, log_bits=flags["bits"])
        total += parity.assert_stream(ev, s, orc, default_mode=flags["default_mode"])
        if flags["bits"]:
            assert parity.assert_bits(ev, s, orc, "stream %d" % s) > 1000
        telegrams += sum(1 for e in orc.events_full() if e[7] == 1)
    assert total >= 8 and telegrams >= 8  # four protocols or more per stream decode


@pytest.mark.parametrize("p,q", SCENE_RATES)
def test_results_do_not_depend_on_the_cut(p, q):
    iq = rate_scene(p, q)
    one, _ = run_input(iq, (12,), p, q, all_flushes=True)
    four, _ = run_input(iq, (3, 3, 3, 3), p, q, all_flushes=True)
    a, b = parity.sort_events(np.concatenate(one)), parity.sort_events(np.concatenate(four))
    assert len(a) > 20 and a.tobytes() == b.tobytes()


def test_reset_in_mid_stream_equals_a_fresh_receiver():
    p, q = 4, 3
    iq = rate_scene(p, q)
    sizes = (3, 3, 3, 3)
    evs, y0 = run_input(iq, sizes, p, q, all_flushes=True, before=lambda r, k: r.reset_streams([1]) if k == 2 else None)
    cut = 2 * resample.input_samples(6, p, q)
    # stream 0 carries on; stream 1 is a receiver on the input before the cut, then a fresh one on the input after it
    parity.assert_segment(np.concatenate(evs), 0, oracle_of(iq[0], p, q), "stream 0")
    first = parity.assert_segment(np.concatenate(evs[:2]), 1, oracle_of(iq[1][:cut], p, q), "stream 1 before the reset")
    second = parity.assert_segment(np.concatenate(evs[2:]), 1, oracle_of(iq[1][cut:], p, q), "stream 1 after the reset")
    assert first > 0 and second > 0
    fresh = resample.resample_s16(iq[1][cut:], p, q)  # zero history behind the cut
    assert np.array_equal(y0[2][1], fresh[:len(y0[2][1])])
    assert not np.array_equal(y0[2][1][:16], resample.resample_s16(iq[1], p, q)[2 * 6 * 4 * api.BLOCK_DEC:][:16])


TUNES = (200000, -250000)


@pytest.mark.parametrize("p,q", SCENE_RATES)
def test_tunes_and_shared_rows_compose(p, q):
    """tune_streams acts on y0: the oracle on tune.py's mixer applied to the restatement's output.  Three streams mapped to one
    row with different tunes equal three receivers fed copies of it."""
    hz = (0,) + TUNES
    row = parity.tuned_row(p, q, hz)
    sizes = (3, 3)

    def shared(r, k):
        if k == 0:
            r.map_streams([0, 1, 2], [0, 0, 0])
            r.tune_streams([0, 1, 2], hz)
            assert r.rows_in_use == 1

    def copies(r, k):
        if k == 0:
            r.tune_streams([0, 1, 2], hz)

    ev_shared, y0 = run_input(row, sizes, p, q, n_streams=3, before=shared, all_flushes=True)
    ev_copies, _ = run_input(np.repeat(row, 3, axis=0), sizes, p, q, before=copies, all_flushes=True)
    a, b = parity.sort_events(np.concatenate(ev_shared)), parity.sort_events(np.concatenate(ev_copies))
    assert a.tobytes() == b.tobytes()
    for s in range(3):
        orc = parity.tuned_oracle(p, q, hz, narrow_hz=hz[s], types=TYPES, thresh=THRESH)
        parity.assert_segment(a, s, orc, "stream %d tune %d" % (s, hz[s]))
        assert parity.decoded(orc) == [s], s  # each receiver decodes the burst it is tuned to
        assert np.array_equal(y0[0][s], resample.resample_s16(row[0], p, q)[:len(y0[0][s])])  # stage 0 is ahead of the tune


def test_error_paths_leave_the_context_usable():
    p, q = 4, 3
    iq = rate_scene(p, q, n_blocks=3)
    cfg = api.Config(2, TYPES, THRESH, 0, 0, 4, 4096, api.F_ALL_FLUSHES | api.F_INPUT_10X)
    h = api.C.c_void_p()
    L = api.load_library()
    assert L.tfrec_amd_create_rate(api.C.byref(cfg), p, q, api.C.byref(h)) == api.E_INVAL and not h
    cfg.flags = api.F_ALL_FLUSHES
    assert L.tfrec_amd_create_rate(api.C.byref(cfg), 3, 4, api.C.byref(h)) == api.E_INVAL and not h
    with api.Receiver(2, TYPES, THRESH, 0, max_blocks=4, all_flushes=True, input_rate=(p, q)) as r:
        for nb in (1, 2, 4):  # no multiple of 3: not a whole number of input samples
            with pytest.raises(api.TfrecAmdError) as e:
                r.input_bytes(nb)
            assert e.value.code == api.E_INVAL
            with pytest.raises(api.TfrecAmdError) as e:
                r.submit(iq, n_blocks=nb)
            assert e.value.code == api.E_INVAL
        with pytest.raises(api.TfrecAmdError) as e:
            r.tune_streams_wide([0], [1000])
        assert e.value.code == api.E_INVAL
        assert r.input_bytes(3) == iq.shape[1] == 2 * 3 * 32768 * 4 // 3
        before = r.memory()["device_bytes"]
        assert r.submit(iq) == 3  # nothing was queued or marked: the context is the fresh one
        assert r.memory()["device_bytes"] - before == iq.size  # submit_host staged exactly the rows' bytes
        ev = r.drain()
        for s in range(2):
            assert parity.assert_segment(ev, s, oracle_of(iq[s], p, q), "stream %d" % s) > 0
    for kw, rate, bb in ((dict(), (1, 1), api.BLOCK_BYTES), (dict(input_10x=True), (10, 1), 10 * api.BLOCK_BYTES)):
        with api.Receiver(1, TYPES, THRESH, 0, max_blocks=2, **kw) as r:  # the other kinds of context answer too
            rp, rq = api.C.c_int32(0), api.C.c_int32(0)
            assert L.tfrec_amd_get_input_rate(r.h, api.C.byref(rp), api.C.byref(rq)) == api.E_OK
            assert (rp.value, rq.value) == rate == r.input_rate
            assert r.input_bytes(2) == 2 * bb == 2 * r.block_bytes
            with pytest.raises(api.TfrecAmdError):
                r.input_bytes(0)


def test_memory_counts_the_stage():
    with api.Receiver(4, TYPES, THRESH, 0, max_blocks=3) as r:
        plain = r.memory()["device_bytes"]
    with api.Receiver(4, TYPES, THRESH, 0, max_blocks=3, input_rate=(25, 16)) as r:
        rate = r.memory()["device_bytes"]
    # stage 0 (one buffer per set), the int16 FIR history instead of the u8 one, two raw histories, the tap table
    assert rate - plain == api.FIFO_DEPTH * 4 * 4 * 3 * api.BLOCK_DEC * 4 + 2 * 4 * 112 + 2 * 4 * 128 + 16 * 10 * 4


@pytest.fixture(scope="module")
def cli():
    return parity.build_cli()


def test_cli_replays_a_2048000_dump(cli, tmp_path):
    """tfrec_gpu -r 2048000 prints the telegram lines of the host decoders fed by the oracle behind the restatement; -b 4 is
    rounded up to 6, so the 12 blocks run as two submits."""
    p, q = 4, 3
    iq = rate_scene(p, q)
    for s in range(len(iq)):
        f = tmp_path / ("s%d.iq" % s)
        np.concatenate([iq[s], np.full(1000, 128, dtype=np.uint8)]).tofile(f)  # (a trailing partial piece is dropped)
        out = subprocess.run([cli, "-r", "2048000", "-T", "%x" % TYPES, "-t", str(THRESH), "-b", "4", "-L", str(f)],
                             capture_output=True, text=True, timeout=600)
        assert out.returncode == 0 and "rounded up to 6" in out.stderr, out.stderr
        want = [ln for ln in oracle_of(iq[s], p, q).text().splitlines()
                if ln.strip() and not ln.startswith("Inverted") and not ln.startswith("WHB:")]
        got = [ln for ln in out.stdout.splitlines() if ln.strip() and not ln.startswith("WHB:")]
        assert got == want and len(want) >= 4, s
