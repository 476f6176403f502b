"""The burst band's restatement (tfrec_amd/band.py), the two exports, tfrec_gpu -I's usage errors and its output code
-- no GPU needed.  Exact integers; nothing here has a tolerance."""
import os
import subprocess

import numpy as np
import pytest

import parity
from recorder_rows import GOLDEN, golden_dec, quiet
from tfrec_amd import api, band, capture

B = api.BLOCK_DEC
SEG = band.SEG


def test_bands_against_the_per_sample_form_on_crafted_segments():
    """A tone between two bins at sh = 1, a segment that is all (32767, -32768) (sh = 3), a silent one, and a run with no whole segment."""
    z = quiet(1, 3)
    ph = 2 * np.pi * 40.3 * np.arange(SEG) / SEG
    z[SEG:2 * SEG] = np.rint(9000 * np.stack([np.cos(ph), np.sin(ph)], axis=1))
    z[2 * SEG:3 * SEG] = (32767, -32768)
    z[3 * SEG:4 * SEG] = 0
    runs = np.zeros(2, dtype=capture.RUN_DTYPE)
    runs["start_sample"], runs["n_samples"] = (SEG, 4 * SEG + 1), (3 * SEG + 5, 2 * SEG - 2)
    got = band.bands([z.reshape(-1)], runs)
    assert got.tobytes() == band.bands_bruteforce([z.reshape(-1)], runs).tobytes()
    assert got["n_segments"].tolist() == [2, 0] and got["n_silent"].tolist() == [1, 0] and got[0]["spec"].any() and not got[1]["spec"].any()


def rec_with(spec, n_segments=1):
    r = np.zeros((), dtype=band.BAND_DTYPE)
    r["n_segments"] = n_segments
    for j, v in spec.items():
        r["spec"][j + 128] = v
    return r


# worked by hand from the header's Summary: (peak_hz, centre_hz, bw_hz, lo_hz, hi_hz)
@pytest.mark.parametrize("spec, want", [
    ({-128: 1000, -127: 400}, (-96000, -95786, 1500, -96000, -95250)),  # the peak at the lower end bin: no refinement
    ({126: 400, 127: 1000}, (95250, 95035, 1500, 94500, 95250)),  # ... and at the upper
    ({127: 1000}, (95250, 95250, 750, -96000, 95250)),  # the centroid in the top bin: c = 126
    ({-1: 1, 0: 6}, (-34, -108, 1500, -750, 0)),  # a negative numerator and a negative centroid: floor, not truncation
    ({-10: 4, 0: 1000, 10: 6}, (0, 14, 8250, 0, 7500)),  # 200 * 4 <= 1010 < 200 * 6: the lower skirt is cut, the upper is kept
    ({}, None),  # tot == 0
])
def test_the_summary_on_hand_set_spectra(spec, want):
    assert band.summary(rec_with(spec)) == want
    assert band.summary(rec_with(spec, n_segments=0)) is None
    assert band.line("f", rec_with(spec)) == "band f 0 0 1 " + ("- - - - -" if want is None else "%d %d %d %d %d" % want)


def test_the_records_size_and_the_two_exports():
    assert band.BAND_DTYPE.itemsize == 2080 and band.BAND_DTYPE.fields["spec"][1] == 32
    assert {"tfrec_amd_enable_burst_band", "tfrec_amd_read_burst_bands"} <= set(api.EXPORTS)
    assert callable(api.Receiver.enable_burst_band) and callable(api.Receiver.read_burst_bands)


@pytest.mark.parametrize("args", [["-X", "x.hex"], ["-s", "100"], ["-A"], ["-k", "p"], ["-K", "p"]])
def test_cli_usage_errors_are_decided_before_a_device_is_opened(args, tmp_path):
    parity.build_cli()
    f = tmp_path / "empty.iq"
    f.write_bytes(b"")
    out = subprocess.run([parity.CLI, "-I"] + args + ["-L", str(f)], capture_output=True, text=True, timeout=60)
    assert out.returncode in (1, 2) and "-I" in out.stderr and "hip" not in out.stderr.lower()


# what the restatement gives for every trigger window of the five golden scenes (DESIGN.md 6zd holds the same table)
GOLDEN_LINES = {
    "tfa_1": ["10004 4056 7 -26095 -6127 72000 -26250 12750", "28315 4056 7 -15580 3354 59250 -15750 23250"],
    "tfa_2": ["10003 2167 3 -33751 -4003 80250 -33750 18000", "25583 2168 4 -45693 -11146 114000 -45750 40500"],
    "tfa_3": ["10004 3976 7 -45479 -6643 108750 -45750 40500", "24647 3977 6 -48859 -3436 102750 -48750 37500"],
    "tx22": ["10004 4605 8 -47058 -4559 107250 -47250 55500", "24737 5300 9 -48684 -12017 114000 -48750 58500"],
    "whb": ["10004 28344 54 3098 3048 15750 3000 3750"],
}


@pytest.mark.parametrize("name", GOLDEN)
def test_the_golden_scenes_summaries(name):
    dec = golden_dec(name)
    recs = band.bands([dec], capture.captures(dec, 0x2F, 500)[0])
    assert [band.line("f", r) for r in recs] == ["band f " + ln for ln in GOLDEN_LINES[name]]


def test_the_hosts_merge_summary_and_line_under_the_sanitizers(tmp_path):
    """job.h's band_add, band_summary and band_line and the merger, in a stand-alone program under ASan and UBSan: a chain of two
    pieces whose sum saturates, then the hand-set spectra above and a record with no segment."""
    exe = str(tmp_path / "band_driver")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(parity.ROOT, "tests", "band_driver.cpp")])
    top = (1 << 64) - 1
    pieces = [(capture.RUN_OPEN, 0, B, 16, 0, {-50: top - 5, -49: 400, 3: 7}), (capture.RUN_CONTINUES, B, 900, 1, 1, {-50: 9, -49: 1, -51: 700}),
              (0, 20000, 5000, 1, 0, {-128: 1000, -127: 400}), (0, 30000, 5000, 1, 0, {126: 400, 127: 1000}), (0, 40000, 5000, 1, 0, {127: top}),
              (0, 50000, 5000, 1, 0, {-1: 1, 0: 6}), (0, 60000, 5000, 1, 0, {-10: 4, 0: 1000, 10: 6}), (0, 70000, 5000, 1, 0, {}),
              (0, 80000, 5000, 0, 0, {5: 9})]
    recs = []
    for flags, start, n, nseg, nsil, spec in pieces:
        r = rec_with(spec, nseg)
        r["flags"], r["start_sample"], r["n_samples"], r["n_silent"] = flags, start, n, nsil
        recs.append(r)
    want = [band.line("f", c) for c in [band.merge(recs[:2])] + recs[2:]]
    text = "".join("%d %d %d %d %d %s\n" % (p[:5] + (" ".join("%d:%d" % kv for kv in p[5].items()),)) for p in pieces)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stderr == "" and out.stdout.splitlines() == want
    assert want[0].split()[2:5] == ["0", str(B + 900), "17"] and want[-2].endswith(" - - - - -") and want[-1].endswith(" - - - - -")
