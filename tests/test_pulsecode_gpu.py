"""The pulse slicer on the GPU (tfrec_amd_enable_burst_symbols, tfrec_amd_read_burst_symbols, tfrec_gpu -J), bit for bit:
the records and both bitmaps' words against tfrec_amd/pulsecode.py run on the context's OWN run table and track of the same submit.
tests/pulse_rows.py says what each hand-made row is there for.  Exact integers: nothing here has a tolerance."""
import numpy as np
import pytest

import parity
import pulse_rows as P
from pulse_rows import B
from recorder import assert_tables, cli_lines, hand_receiver, raises, same_records, same_words
from recorder_rows import CTX_TYPES, scene
from tfrec_amd import api, pulsecode
from tfrec_amd.pulsecode import GAP, WIDTH, Settings

pytestmark = pytest.mark.gpu
LAYOUTS = {"uncut": (2,), "blocks": (1, 1)}
ONES = "1" * 100
# the merged chains' symbols by (stream, start_sample) with lo 1, mid 50, hi 300 and SHORT_ONE, counted by hand
WANT = {WIDTH: {(0, 64): ONES + "11", (0, 2000): "0", (0, 4000): "01", (0, B - 1700): ONES + "/1", (0, 2 * B - 3): "1", (1, 200): "10",
                (1, B - 2600): "000"},
        GAP: {(0, 64): "/" + ONES + "0", (0, 2000): "/", (0, 4000): "/0", (0, B - 1700): "/" + ONES + "1", (0, 2 * B - 3): "/1", (1, 200): "/1",
              (1, B - 2600): "//0"}}


def run(st, rows, sizes, cap=None, resets=None, overflow=False):
    """The rows in submits of `sizes` blocks, queued before the first read unless resets ({submit: streams}) come between them;
    every submit's records and words compared -> [(records, bits words, marks words)]."""
    n, subs, state = len(rows), [], None
    with hand_receiver(n, max(sizes), (), cap=cap or (32 * n, n * max(sizes) * B)) as r:
        r.enable_burst_track_amplitude(1)
        r.enable_burst_symbols(st.mode, st.lo, st.mid, st.hi, st.short_one)
        r.set_burst_track_level(range(n), [P.LEVEL] * n)
        ends = np.cumsum(sizes) * B
        parts = [np.ascontiguousarray(rows[:, e - nb * B:e]) for nb, e in zip(sizes, ends)]
        if not resets:
            for x in parts:
                r.submit(x)
        for i, x in enumerate(parts):
            if resets:
                if i in resets:
                    r.reset_streams(resets[i])
                r.submit(x)
            r.read_captures(allow_overflow=overflow)
            if overflow:
                raises(api.E_OVERFLOW, r.read_burst_symbols)
            trecs, twords = r.read_burst_tracks(allow_overflow=overflow)
            got, bits, marks = r.read_burst_symbols(allow_overflow=overflow)
            assert got.dtype == pulsecode.SYMBOLS_DTYPE and r.symbols_total == r.track_total and len(bits) == len(marks) == len(twords)
            want, wbits, wmarks, state = pulsecode.symbols_bruteforce(trecs, twords, st, state, n, max_samples=r._capture[1])
            same_records(got, want, "symbols")
            same_words(bits, wbits, "symbol bits")
            same_words(marks, wmarks, "symbol marks")
            subs.append((got, bits, marks))
            r.drain()
    return subs


def texts(subs, restarts=None):
    return {(int(c["stream"]), int(c["start_sample"])): pulsecode.text(c) for c in pulsecode.chains(subs, restarts)}


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("mode", [WIDTH, GAP])
def test_records_and_bitmaps_of_two_streams_of_two_blocks_of_hand_made_rows(mode, layout):
    subs = run(Settings(mode, 1, 50, 300, True), P.hand_rows(), LAYOUTS[layout])
    assert texts(subs) == WANT[mode]
    last = subs[-1][0]
    short = last[last["stream"] == 0][-1]  # the run of 3 samples at the input's end, open; stream 1's first run shares its word
    assert short["n_samples"] == 3 and short["flags"] & P.OPEN and short["n_symbols"] == (1 if mode == WIDTH else 2)
    assert last[last["stream"] == 1][0]["bit_offset"] == short["bit_offset"] + 3 and short["bit_offset"] % 32 < 29


def test_65_streams_and_glitches():
    rows = P.hand_rows()[np.arange(65) % 2]
    subs = run(Settings(WIDTH, 3, 50, 300), rows, (1, 1))
    got = texts(subs)
    assert all(got[s, k] == got[s % 2, k] for s in range(65) for k in (64, 200) if (s % 2, k) in got) and len(got) == 33 * 5 + 32 * 2
    assert got[0, 64] == "00" and got[64, B - 1700] == "/0" and sum(int(r["n_glitches"]) for recs, _, _ in subs for r in recs) == 33 * 201


def test_a_reset_mid_chain_drops_the_history():
    st = Settings(WIDTH, 1, 50, 1200, True)
    assert texts(run(st, P.hand_rows()[:1], (1, 1)))[0, B - 1700] == ONES + "/1"  # 2500 samples of pulse across the cut: a break
    subs = run(st, P.hand_rows()[:1], (1, 1), resets={1: [0]})
    behind = subs[1][0][0]
    assert not behind["flags"] & P.CONT and behind["start_sample"] == 0
    assert pulsecode.text(pulsecode.piece_of(behind, *subs[1][1:])) == "01"  # the 1000 samples behind the reset alone: long


def test_overflow_on_max_runs_and_on_max_samples_delivers_the_tracks_prefixes():
    st, rows = Settings(GAP, 1, 50, 300, True), P.hand_rows()
    (whole, _, _), = run(st, rows, (2,))
    (got, bits, _), = run(st, rows, (2,), cap=(len(whole) - 1, 4 * B), overflow=True)  # the table a run short
    same_records(got, whole[:-1], "the prefix")
    assert len(bits) == (int(whole[-1]["bit_offset"]) + 31) // 32
    room = int(whole[3]["bit_offset"] + whole[3]["n_samples"])  # the pool holds the first four runs, and not the fifth
    (got, bits, _), = run(st, rows, (2,), cap=(32, room + 2), overflow=True)
    same_records(got[:4], whole[:4], "the runs that fit")
    assert len(got) == len(whole) and not got["n_symbols"][4:].any() and len(bits) == (room + 31) // 32


def test_the_refusals_the_memory_and_a_context_without_the_call():
    n, x = 3, scene()[:3, :api.BLOCK_BYTES]
    seen = []
    for on in (False, True):
        with api.Receiver(n, CTX_TYPES, 500, 0, max_blocks=2) as r:
            r.enable_capture(64, 1024)
            raises(api.E_INVAL, r.enable_burst_symbols, WIDTH, 1, 2, 3)  # no track
            r.enable_burst_track_amplitude(16)
            m = r.memory()
            for bad in ((2, 1, 2, 3), (WIDTH, 0, 2, 3), (WIDTH, 3, 2, 3), (GAP, 1, 4, 3), (GAP, 1, 2, 2047), (2 ** 31, 1, 2, 3)):
                raises(api.E_INVAL, r.enable_burst_symbols, *bad)
            assert r.L.tfrec_amd_enable_burst_symbols(r.h, 0, 1, 2, 3, 2) == api.E_INVAL and r.memory() == m  # an unknown flag; nothing was allocated
            raises(api.E_INVAL, r.read_burst_symbols)
            if on:
                r.enable_burst_symbols(GAP, 1, 2, 3, True)
                assert r.memory()["device_bytes"] - m["device_bytes"] == pulsecode.device_bytes(n, 64, 1024)
                assert r.memory()["pinned_host_bytes"] == m["pinned_host_bytes"]
                raises(api.E_INVAL, r.enable_burst_symbols, GAP, 1, 2, 3)  # a second call
            r.submit(x)
            raises(api.E_INVAL if on else api.E_STATE, r.enable_burst_symbols, WIDTH, 1, 2, 3)  # a second call; after the first submit
            seen.append((r.read_captures(), r.read_burst_tracks(), r.drain()))
    (runs, trk, ev), (runs1, trk1, ev1) = seen
    assert_tables(runs1, runs)  # the table, the track and the events do not notice
    assert trk1[0].tobytes() == trk[0].tobytes() and trk1[1].tobytes() == trk[1].tobytes()
    assert parity.sort_events(ev1).tobytes() == parity.sort_events(ev).tobytes()


def test_cli_symbols_line_of_an_fs20_like_burst_across_a_batch_boundary(tmp_path):
    parity.build_cli()
    x, level, want = P.cli_scene()
    f = str(tmp_path / "fs20.iq")
    x.tofile(f)
    want = [ln % f for ln in want]
    assert [ln.split()[0] for ln in want] == ["bits", "pulses", "symbols"] and want[2].endswith(" 12 0 0 " + "".join(map(str, P.CLI_BITS)))
    every = ("bits", "pulses", "symbols")
    got = cli_lines(["-G", "2500", "-O", str(level), "-J", "width,100,192,300", "-T", "2f", "-t", "500", "-b", "2", "-L", f], every)
    assert got[every] == want
