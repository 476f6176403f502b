"""The pulse slicer without a GPU (tfrec_amd/pulsecode.py, tests/pulse_rows.py, tfrec_amd/host/job.h): the restatement
against results counted by hand, the cuts, the API's surface and the host's merge and line."""
import ctypes
import os
import re
import subprocess

import pytest

import amplitude_rows as A
import parity
import pulse_rows as P
from pulse_rows import B, stretches
from tfrec_amd import api, pulsecode
from tfrec_amd.pulsecode import GAP, WIDTH, Settings

WIDE = (100, 192, 2046)
# (the track, mode, (lo, mid, hi), SHORT_ONE) -> the symbols and the glitches, counted by hand
HAND = [
    (stretches(99, 9, 100, 9, 191, 9, 192, 9, 300, 9, 301, 9), WIDTH, P.FS20, False, "0011/", 1),  # lo - 1, lo, mid - 1, mid, hi, hi + 1
    (stretches(2046, 9, 2047, 9, 3000, 9), WIDTH, WIDE, False, "1//", 0),  # hi = 2046 is long; the cap decides nothing
    (stretches(5, 99, 5, 100, 5, 191, 5, 192, 5, 300, 5, 301, 5, 2046, 5, 2047, 5, 3000, 5), GAP, P.FS20, False, "/0011////", 1),
    (stretches(5, 2046, 5, 2047, 5), GAP, WIDE, True, "/0/", 0),
    (stretches(150, 150, 10), WIDTH, P.FS20, False, "0", 0),  # a chain that begins on 1: its first pulse is a pulse ...
    (stretches(150, 150, 10), GAP, P.FS20, False, "/0", 0),  # ... and its first sample a rise behind no gap: a break
    (stretches(150, 10, 200, 5, first=0), GAP, P.FS20, False, "/1", 0),  # a leading gap reaches the chain's start, whatever its width
    (stretches(150, 10, 200, 5, first=0), WIDTH, P.FS20, False, "", 1),  # (no fall behind the last pulse)
]


@pytest.mark.parametrize("t,mode,widths,one,want,glitches", HAND)
def test_the_restatement_against_results_counted_by_hand(t, mode, widths, one, want, glitches):
    sy, gl = pulsecode.decide(t, [], Settings(mode, *widths, one))
    assert ("".join(str(x) for x in sy), gl) == (want, glitches)


def test_the_fs20_like_burst_gives_back_the_bits_put_in():
    bits = [1, 0, 0, 1, 1, 1, 0, 1, 0, 0, 0, 1]
    tsubs = A.submits(A.pw_row(bits, 2).reshape(-1), (2,), 1, A.ON // 2)
    text = lambda st: [pulsecode.text(c) for c in pulsecode.chains(P.restated(tsubs, st))]  # noqa: E731
    assert text(Settings(WIDTH, *P.FS20)) == ["".join(map(str, bits))]
    assert text(Settings(GAP, *P.FS20, True)) == ["/" + "".join(str(1 - b) for b in bits[:-1])]  # the last gap is lost


@pytest.mark.parametrize("mode", [WIDTH, GAP])
def test_every_block_cut_and_a_three_piece_cut_merge_to_the_uncut_stream(mode):
    g = A.lcg(77)
    t = stretches(*[(1 + next(g) % 200) if next(g) % 9 else 2040 + next(g) % 20 for _ in range(300)])[:3 * B]
    t[B - 70:B + 90] = [0] * 40 + [1] * 80 + [0] * 40  # a pulse across the first cut
    assert len(t) == 3 * B
    st = Settings(mode, 20, 100, 2000)
    whole, = pulsecode.chains(P.restated(P.cut_chain(t, (3,)), st))
    assert int(whole["n_symbols"]) > 40 and 0 < int(whole["n_breaks"]) and 0 < int(whole["n_glitches"])
    for sizes in ((1, 2), (2, 1), (1, 1, 1)):
        subs = P.restated(P.cut_chain(t, sizes), st)
        got, = pulsecode.chains(subs)
        assert got.rec.tobytes() == whole.rec.tobytes() and pulsecode.text(got) == pulsecode.text(whole), sizes
        assert all(int(r["n_symbols"]) <= (int(r["n_samples"]) + 1) // 2 for recs, _, _ in subs for r in recs)


def test_the_c_abi_exports_the_pulse_slicer_and_the_memory_sums():
    lib = ctypes.CDLL(api.load_library()._name)
    assert lib.tfrec_amd_enable_burst_symbols and lib.tfrec_amd_read_burst_symbols
    assert {"tfrec_amd_enable_burst_symbols", "tfrec_amd_read_burst_symbols"} <= set(api.EXPORTS)
    text = open(parity.ROOT + "/include/tfrec_amd.h").read()
    body = re.search(r"typedef struct \{[^}]*\} tfrec_amd_burst_symbols;", text).group(0)
    size = {"uint32_t": 4, "int32_t": 4, "int64_t": 8, "uint64_t": 8}
    assert sum(size[t] for t in re.findall(r"^\s*(u?int\d+_t)\s", body, re.M)) == 48 == pulsecode.SYMBOLS_DTYPE.itemsize
    for bad in ((2, 1, 2, 3), (-1, 1, 2, 3), (WIDTH, 0, 2, 3), (WIDTH, 3, 2, 3), (GAP, 1, 4, 3), (GAP, 1, 2, 2047)):  # the refused settings
        with pytest.raises(ValueError):
            Settings(*bad)
    Settings(GAP, 1, 1, 1), Settings(WIDTH, 2046, 2046, 2046)
    assert pulsecode.device_bytes(3, 64, 1025) == api.FIFO_DEPTH * (64 * 48 + 5 * 4 * 33) + 3 * 260 and pulsecode.pinned_bytes(3) == 0


def test_the_hosts_merge_and_line_are_the_restatements(tmp_path):
    exe = str(tmp_path / "pulse_driver")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(parity.ROOT, "tests", "pulse_driver.cpp")])
    g = A.lcg(5)
    t = stretches(*[1 + next(g) % 3 for _ in range(9000)])[:2 * B]  # more than 2048 symbols: the line's +
    subs = P.restated(P.cut_chain(t, (1, 1)), Settings(WIDTH, 2, 3, 3))
    lines = ["file 2"] + ["piece 1 %d %d %d 37 %d %d %s" % (r["flags"], r["start_sample"], r["n_samples"], r["n_breaks"], r["n_glitches"],
                                                        pulsecode.text(pulsecode.piece_of(r, b, m))) for (r,), b, m in subs]
    out = subprocess.run([exe], input="".join(x + "\n" for x in lines), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    whole, = pulsecode.chains(subs)
    assert int(subs[0][0][0]["n_symbols"]) < pulsecode.LISTED < int(whole["n_symbols"])  # the listed symbols end inside the second piece
    assert out.stdout.splitlines() == [pulsecode.line("f", whole)]


def test_cli_symbols_usage_errors(tmp_path):
    parity.build_cli()
    for args, text in ((["-J", "width,100,192,300"], "-J slices the track"), (["-G", "2500", "-J", "width,192,100,300"], "bad -J"),
                       (["-G", "2500", "-J", "period,1,2,3"], "bad -J"), (["-G", "2500", "-J", "gap,1,2,3", "-s", "50"], "-G reads the bursts")):
        out = parity.run_cli(args + ["-L", str(tmp_path / "missing.iq")])
        assert out.returncode == 1 and text in out.stderr, (args, out.stderr)
