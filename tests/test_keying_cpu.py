"""The envelope clock's restatement (tfrec_amd/clock.py: keyings, summary and line with KEYING), the two exports and
tfrec_gpu -a's usage errors -- no GPU needed.  Exact integers; nothing here has a tolerance."""
import os
import subprocess

import numpy as np
import pytest

import amplitude_rows as A
import parity
from tfrec_amd import api, capture, clock

B = api.BLOCK_DEC


def records_of(z):
    runs, _, _ = capture.captures(z, 0x2F, A.T, None)
    return runs, clock.keyings([z.reshape(-1)], runs)


def test_keyings_against_the_per_sample_form_on_a_crafted_row():
    """One block: a loud run over segment 0 whose amplitude reaches 65534 (sh = 3), and nothing whole in segment 1."""
    z = A.row_with(A.keyed([37, 91] * 40, True, 9, on=9000), 1, 0)
    z[100] = (32767, -32767)
    runs = np.zeros(2, dtype=capture.RUN_DTYPE)
    runs["start_sample"], runs["n_samples"] = (0, 4097), (4096, 4095)
    got = clock.keyings([z.reshape(-1)], runs)
    assert got.tobytes() == clock.keyings_bruteforce([z.reshape(-1)], runs).tobytes()
    assert got["n_segments"].tolist() == [1, 0] and got[0]["spec"].any() and not got[1]["spec"].any()


def rec_with(spec, n_segments=1):
    r = np.zeros((), dtype=clock.CLOCK_DTYPE)
    r["n_segments"] = n_segments
    for j, v in spec.items():
        r["spec"][j - 1] = v
    return r


@pytest.mark.parametrize("spec, want", [
    ({2: 900, 3: 1000, 4: 400}, (375 * 3 + (375 * -500 + 700) // 1400, 100 * 125 * 1000 // 1400)),  # jp = 3: bin 2 is a neighbour only
    ({2: 1001, 3: 1000}, (375 * 3, 100 * 125)),  # ... and one that exceeds the peak: no refinement
    ({126: 10, 127: 1000, 128: 600}, (375 * 127 + (375 * 590 + 1390) // 2780, 100 * 125 * 1000 // 1010)),  # jp = 127: bin 128 likewise
    ({49: 700, 50: 1000, 51: 1}, (375 * 50 + (375 * -699 + 1299) // 2598, 100 * 125 * 1000 // 1701)),  # a negative numerator: floor, not truncation
    ({1: 5, 2: 5, 128: 5}, None),  # tot == 0: the band is empty
])
def test_the_summary_on_hand_set_spectra(spec, want):
    assert clock.summary(rec_with(spec), clock.KEYING) == want
    assert (375 * -699 + 1299) // 2598 == -101 != int((375 * -699 + 1299) / 2598)
    assert clock.summary(rec_with(spec, n_segments=0), clock.KEYING) is None


def test_the_quarter_hz_print_and_the_clocks_own_line():
    r = rec_with({50: 1000, 51: 400})  # off = floor((375 * 400 + 1600) / 3200) = 47: 18797 quarter-Hz
    r["start_sample"], r["n_samples"] = 7, 5000
    assert clock.line("f", r, clock.KEYING) == "keying f 7 5000 1 4699.25 89.28"
    assert clock.line("f", rec_with({}), clock.KEYING) == "keying f 0 0 1 - -"
    assert clock.line("f", r).startswith("clock f 7 5000 1 ")  # the burst clock's line keeps its form: Hz, no decimals
    assert "." not in clock.line("f", r).split()[5]


def test_the_two_exports():
    assert {"tfrec_amd_enable_burst_keying", "tfrec_amd_read_burst_keyings"} <= set(api.EXPORTS)
    assert callable(api.Receiver.enable_burst_keying) and callable(api.Receiver.read_burst_keyings)


@pytest.mark.parametrize("args", [["-X", "x.hex"], ["-s", "100"], ["-A"], ["-k", "p"], ["-K", "p"]])
def test_cli_usage_errors_are_decided_before_a_device_is_opened(args, tmp_path):
    parity.build_cli()
    f = tmp_path / "empty.iq"
    f.write_bytes(b"")
    out = subprocess.run([parity.CLI, "-a"] + args + ["-L", str(f)], capture_output=True, text=True, timeout=60)
    assert out.returncode in (1, 2) and "-a" in out.stderr and "hip" not in out.stderr.lower()
    usage = subprocess.run([parity.CLI, "-h"], capture_output=True, text=True, timeout=60)
    assert "  -a  " in usage.stdout + usage.stderr


def test_an_ook_burst_keyed_with_a_256_sample_period_reads_1500_hz():
    runs, got = records_of(A.row_with(A.keyed([128] * 200, True, 5), 4, 300))
    assert len(got) == 1 and got[0]["n_segments"] == 5
    qhz, q = clock.summary(got[0], clock.KEYING)
    assert abs(qhz - 4 * 1500) <= 375 and clock.line("f", got[0], clock.KEYING) == "keying f 300 26165 5 1500.00 106.68"


def test_the_pulse_width_burst_reads_a_rate_between_its_two_symbol_rates():
    runs, got = records_of(A.pw_row(A.hex_bits("a5c3961e") * 3, 6))
    qhz, q = clock.summary(got[0], clock.KEYING)
    assert 384000 / (2 * A.PW_LONG) < qhz / 4 < 384000 / (2 * A.PW_SHORT)
    assert clock.line("f", got[0], clock.KEYING) == "keying f 500 37403 8 1031.50 28.26"  # (what the restatement gives)


def test_the_hosts_merge_summary_and_line_under_the_sanitizers(tmp_path):
    """job.h's parameterised summary and line and the clock's merger, in a stand-alone program under ASan and UBSan: a chain of two
    pieces whose sum saturates, the guard at both ends of the band, a negative numerator, an empty band and no segment."""
    exe = str(tmp_path / "keying_driver")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(parity.ROOT, "tests", "keying_driver.cpp")])
    top = (1 << 64) - 1
    pieces = [(capture.RUN_OPEN, 0, B, 2, 0, {50: top - 5, 51: 400, 3: 7}), (capture.RUN_CONTINUES, B, 900, 1, 1, {50: 9, 51: 1, 49: 700}),
              (0, 20000, 5000, 1, 0, {2: 900, 3: 1000, 4: 400}), (0, 30000, 5000, 1, 0, {126: 10, 127: 1000, 128: 600}),
              (0, 40000, 5000, 1, 0, {49: 700, 50: 1000, 51: 1}), (0, 50000, 5000, 1, 0, {1: 5, 2: 5, 128: 5}), (0, 60000, 5000, 0, 0, {})]
    recs = []
    for flags, start, n, nseg, nsil, spec in pieces:
        r = rec_with(spec, nseg)
        r["flags"], r["start_sample"], r["n_samples"], r["n_silent"] = flags, start, n, nsil
        recs.append(r)
    want = [clock.line("f", c, clock.KEYING) for c in [clock.merge(recs[:2])] + recs[2:]]
    text = "".join("%d %d %d %d %d %s\n" % (p[:5] + (" ".join("%d:%d" % kv for kv in p[5].items()),)) for p in pieces)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stderr == "" and out.stdout.splitlines() == want
    assert want[0].split()[2:5] == ["0", str(B + 900), "3"] and want[-2].endswith(" - -") and want[-1].endswith(" - -")
