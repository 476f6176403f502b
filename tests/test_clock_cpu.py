"""The burst clock without a GPU (tfrec_amd_enable_burst_clock, tfrec_gpu -C): the restatement tfrec_amd/clock.py
against its per-sample form, the readings of the golden scenes against the protocols' nominal rates (also rotated, and with a
shifted bit rate), the segment rule at its edges, silent segments, the normalising shift at its steps, the summary's guard, the
behaviour under cutting, saturation, tfrec_gpu's merge (tfrec_amd/host/job.h, compiled into a stand-alone program under the address
and undefined-behaviour sanitizers), the struct and the exports, and what tfrec_gpu decides before it opens a device.

The records are exact integers.  The only tolerances are on readings in Hz: 150 Hz against a nominal rate (the bin is 375 Hz; the
largest error on the golden scenes is 101 Hz), and what rounding a rotated scene to int16 can move (see recorder_rows.rotated())."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import parity
from recorder_rows import golden_dec, keyed, mx_rows, rotated, silent_rows
from tfrec_amd import api, capture, clock, levels, synth
from meter_rows import crafted_dec

B = levels.BLOCK_DEC
SEG = clock.SEG
GOLDEN = ("tfa_1", "tfa_2", "tfa_3", "tx22", "whb")
NOMINAL = dict(tfa_1=38400, tfa_2=17240, tfa_3=9600, tx22=8842, whb=6000)  # synth's bit rates
CONT, OPEN = capture.RUN_CONTINUES, capture.RUN_OPEN
MARGIN = 150  # Hz


def records(dec, types=0x2F, thresh=500, state=None, base=0):
    runs, _, state = capture.captures(dec, types, thresh, state)
    return clock.clocks([dec], runs, base=[base]), runs, state


@functools.lru_cache(maxsize=None)
def golden_records(name, thresh=500):
    return records(golden_dec(name), thresh=thresh)[0]


def submits(dec, sizes, types=0x2F, thresh=500):
    """The stream cut into submits of `sizes` blocks -> the submits' records."""
    st, pos, out = None, 0, []
    for nb in sizes:
        recs, _, st = records(dec[2 * pos * B:2 * (pos + nb) * B], types, thresh, st, pos * B)
        out.append(recs)
        pos += nb
    return out


def table(*rows):
    """A run table by hand: (start, n[, flags]) of stream 0."""
    t = np.zeros(len(rows), dtype=capture.RUN_DTYPE)
    for k, r in enumerate(rows):
        t[k]["start_sample"], t[k]["n_samples"], t[k]["thresh"] = r[0], r[1], 500
        t[k]["flags"] = r[2] if len(r) > 2 else 0
    return t


def same(a, b):
    assert a.dtype == b.dtype == clock.CLOCK_DTYPE and a.tobytes() == b.tobytes()


# ---- the restatement against its per-sample form
def test_the_vectorised_form_equals_the_per_sample_one_on_crafted_samples():
    dec, _ = crafted_dec(max(levels.windows(0x2F)), 0x2F)
    dec = dec.reshape(-1)
    runs = capture.captures(dec, 0x2F, 500)[0]
    runs = np.concatenate([runs, table((0, len(dec) // 2, OPEN))])  # ... and one run over everything: every segment of the rows
    recs = clock.clocks([dec], runs)
    same(recs, clock.clocks_bruteforce([dec], runs))
    assert recs[-1]["n_segments"] + recs[-1]["n_silent"] == len(dec) // 2 // SEG and recs[-1]["n_segments"] >= 1
    k = keyed(1, 10)
    t = table((0, B), (1, B - 1), (3000, 2100))
    same(clock.clocks([k], t), clock.clocks_bruteforce([k], t))


@pytest.mark.parametrize("name", GOLDEN)
def test_the_vectorised_form_equals_the_per_sample_one_on_the_golden_scenes(name):
    dec = golden_dec(name)
    runs = capture.captures(dec, 0x2F, 500)[0]
    same(golden_records(name), clock.clocks_bruteforce([dec], runs))
    assert (golden_records(name)["n_silent"] == 0).all()
    assert max(int(v).bit_length() for r in golden_records(name) for v in r["spec"]) <= 43


# ---- the readings
CROSS = [("tfa_1", 10004, 4056, 3, 38300, 5715), ("tfa_1", 28315, 4056, 3, 38307, 5664), ("tfa_2", 10003, 2167, 1, 17250, 2526),
         ("tfa_2", 25583, 2168, 2, 17250, 3039), ("tfa_3", 10004, 3976, 3, 9701, 3562), ("tfa_3", 24647, 3977, 2, 9681, 3043),
         ("tx22", 10004, 4605, 4, 8927, 2985), ("tx22", 24737, 5300, 4, 8940, 2986), ("whb", 10004, 28344, 27, 5997, 6005)]


def test_the_prototypes_cross_check_values():
    got = [(name, int(r["start_sample"]), int(r["n_samples"]), int(r["n_segments"])) + clock.summary(r)
           for name in GOLDEN for r in golden_records(name)]
    assert got == CROSS


@pytest.mark.parametrize("thresh", [500, 3000])
def test_every_golden_telegram_reads_its_nominal_rate(thresh):
    worst = 0
    for name in GOLDEN:
        recs = golden_records(name, thresh)
        assert len(recs) >= 1 and (recs["n_segments"] >= 1).all()
        for r in recs:
            hz, q = clock.summary(r)
            print(name, thresh, int(r["start_sample"]), hz, hz - NOMINAL[name], q)
            assert abs(hz - NOMINAL[name]) <= MARGIN and q >= 2500  # (a clean telegram: 25 or more)
            worst = max(worst, abs(hz - NOMINAL[name]))
    assert worst == 101  # the figure DESIGN.md 6s states; the nearest pair of protocols is 758 Hz apart


@pytest.mark.parametrize("hz", [20000, -35000])
def test_the_readings_do_not_depend_on_the_carrier_offset(hz):
    for name in GOLDEN:
        recs = records(rotated(golden_dec(name), hz))[0]
        plain = golden_records(name)
        assert len(recs) == len(plain)
        for r, p in zip(recs, plain):
            (a, qa), (b, qb) = clock.summary(r), clock.summary(p)
            print(name, hz, a, b, qa, qb)
            assert r["n_segments"] == p["n_segments"] and abs(a - NOMINAL[name]) <= MARGIN
            assert abs(a - b) <= 2 and 100 * abs(qa - qb) <= qb


def synth_reading(proto, ppm):
    x = synth.gen_scene(5, 6, [dict(proto=proto, start=40000, payload_seed=7, baud_ppm=ppm, amp=60)])
    dec = parity.fresh_oracle(x, 0x2F, 500, keep_dec=True).dec().reshape(-1)
    recs = records(dec)[0]
    assert len(recs) == 1 and recs[0]["n_segments"] >= 1
    return clock.summary(recs[0])[0]


@pytest.mark.parametrize("proto", range(5))
def test_a_synth_burst_with_a_faster_bit_rate_reads_the_shifted_rate(proto):
    baud = (38400, 17240, 9600, 8842, 6000)[proto]
    fast = synth_reading(proto, 20000)
    print(proto, fast, baud * 1.02)
    assert abs(fast - baud * 1.02) <= MARGIN
    if proto == 0:  # 768 Hz faster: two bins
        assert fast - synth_reading(0, 0) > 375


# ---- the segment rule
def test_segment_edges():
    dec = keyed(2, 10)
    q = 3
    t = table((SEG * q, 2 * SEG), (SEG * q + 1, 2 * SEG), (SEG * q + 1, 2 * SEG - 1), (SEG * q, 2 * SEG - 1), (SEG * q + 1, 2046),
              (SEG * q + 1, 2048), (0, 2 * B, OPEN), (B - SEG, 2 * SEG), (B - SEG + 1, 2 * SEG))
    recs = clock.clocks([dec], t)
    same(recs, clock.clocks_bruteforce([dec], t))
    assert recs["n_segments"].tolist() == [2, 1, 1, 1, 0, 1, 16, 2, 1] and (recs["n_silent"] == 0).all()
    one = lambda k: clock.clocks([dec], table((SEG * k, SEG)))[0]["spec"]  # noqa: E731
    assert np.array_equal(recs[0]["spec"], one(q) + one(q + 1))
    for k in (1, 2, 5):
        assert np.array_equal(recs[k]["spec"], one(q + 1))  # a run from 1024 q + 1 loses segment q
    assert np.array_equal(recs[3]["spec"], one(q))  # a run that ends a sample short of a boundary loses the last one
    # 2046 samples from 1024 q + 1, the longest run without a whole segment: no summary (2047 reach the next boundary: recs[2])
    assert not recs[4]["spec"].any() and clock.summary(recs[4]) is None and clock.line("f", recs[4]) == "clock f 3073 2046 0 - -"
    assert np.array_equal(recs[7]["spec"], one(7) + one(8))  # across the block boundary
    hz, qual = clock.summary(recs[6])  # keyed every 10 samples: 38400 Hz; the band's neighbours refine it
    assert abs(hz - 38400) <= 375 and qual > 2500


def test_a_silent_segment():
    dec = silent_rows()
    runs = capture.captures(dec, 0x2F, 500)[0]
    assert len(runs) == 1 and runs[0]["start_sample"] == 1 and runs[0]["flags"] & OPEN  # the trigger never drops
    recs = clock.clocks([dec], runs)
    same(recs, clock.clocks_bruteforce([dec], runs))
    assert (recs[0]["n_segments"], recs[0]["n_silent"]) == (0, 7) and not recs[0]["spec"].any() and clock.summary(recs[0]) is None
    mixed = dec.copy()
    mixed[2 * 2 * SEG:2 * 3 * SEG] = keyed(1, 10)[:2 * SEG]  # one live segment among them
    recs = clock.clocks([mixed], runs)
    same(recs, clock.clocks_bruteforce([mixed], runs))
    assert (recs[0]["n_segments"], recs[0]["n_silent"]) == (1, 6) and clock.summary(recs[0]) is not None


def test_the_normalising_shift_at_its_steps():
    dec = mx_rows()
    z = dec.reshape(-1, 2).astype(np.int64)
    seg = lambda k: clock.g16_of(z[SEG * k:SEG * (k + 1)])  # noqa: E731
    want = [(32767 * 32767) >> 16, (16384 * 16384) >> 16, (32767 * 32767) >> 16, (16384 * 16384) >> 16, (16384 * 16384) >> 16,
            (32761 * 32761) >> 16, (16562 * 16562) >> 16]  # sh = 0, 1, 1, 2, 17, 0, 1
    for k, g in enumerate(want):
        assert (seg(k)[2:] == g).all() and (seg(k)[:2] == 0).all(), k
    d = z[SEG * 7 + 1:SEG * 8] * 0  # the last segment: d = c = -65535 >> 1 = -2^15 throughout, g = 2^31, g16 held at 32767
    d[:, 0] = z[SEG * 7 + 1:SEG * 8, 0] * z[SEG * 7:SEG * 8 - 1, 0] + z[SEG * 7 + 1:SEG * 8, 1] * z[SEG * 7:SEG * 8 - 1, 1]
    d[:, 1] = z[SEG * 7 + 1:SEG * 8, 1] * z[SEG * 7:SEG * 8 - 1, 0] - z[SEG * 7 + 1:SEG * 8, 0] * z[SEG * 7:SEG * 8 - 1, 1]
    assert (d == -65535).all() and (seg(7)[2:] == 32767).all()
    t = table((0, B, OPEN))
    recs = clock.clocks([dec], t)
    same(recs, clock.clocks_bruteforce([dec], t))
    assert (recs[0]["n_segments"], recs[0]["n_silent"]) == (8, 0)


# ---- the summary
def rec_with(spec, n_segments=1):
    r = np.zeros((), dtype=clock.CLOCK_DTYPE)
    r["n_segments"], r["n_samples"] = n_segments, 1024
    for j, v in spec.items():
        r["spec"][j - 4] = v
    return r


def test_the_summary_and_the_guard_of_its_refinement():
    assert clock.summary(rec_with({50: 1000, 49: 400, 51: 600})) == (375 * 50 + (375 * 200 + 1000) // 2000, 100 * 117 * 1000 // 2000)
    hz, _ = clock.summary(rec_with({50: 1000, 49: 601, 51: 400}))  # a negative num: -74376 / 1998 = -37.2 -> -38: floor, not truncation
    assert hz == 375 * 50 + (375 * -201 + 999) // 1998 == 375 * 50 - 38
    # equal bins: the lowest j is the peak, and its equal upper neighbour pulls it half a bin up
    assert clock.summary(rec_with({50: 1000, 49: 1000, 51: 1000, 52: 1})) == (375 * 49 + 188, 100 * 117 * 1000 // 3001)
    # den == 0: only at the band's lower edge, where the neighbour below lies outside the band and may equal the peak
    assert clock.summary(rec_with({12: 7, 11: 7, 13: 7})) == (375 * 12, 100 * 117 * 7 // 14)
    # an out-of-band neighbour larger than the peak: no refinement (den may still be positive or not)
    assert clock.summary(rec_with({12: 1000, 11: 5000, 13: 10})) == (375 * 12, 100 * 117 * 1000 // 1010)
    assert clock.summary(rec_with({12: 1000, 11: 1500, 13: 10}))[0] == 375 * 12  # den = 490 > 0, the neighbour still exceeds
    assert clock.summary(rec_with({128: 1000, 129: 5000, 127: 10})) == (375 * 128, 100 * 117 * 1000 // 1010)
    assert clock.summary(rec_with({128: 1000, 129: 1500, 127: 10}))[0] == 375 * 128
    assert clock.summary(rec_with({128: 1000, 129: 900, 127: 0}))[0] == 375 * 128 + (375 * 900 + 1100) // 2200  # in reach of the guard
    assert clock.summary(rec_with({11: 9, 129: 9, 4: 1, 131: 1})) is None  # nothing inside the band
    assert clock.summary(rec_with({50: 1000}, n_segments=0)) is None
    r = rec_with({50: 1000, 49: 400, 51: 600}, 3)
    r["start_sample"] = 77
    assert clock.line("a.iq", r) == "clock a.iq 77 1024 3 18788 58.50"


# ---- cutting
@pytest.mark.parametrize("name,thresh", [(g, 500) for g in GOLDEN] + [("tx22", 3000)])
def test_the_merged_chains_are_the_uncut_streams_for_every_block_cut(name, thresh):
    dec = golden_dec(name)
    dec = dec[:2 * B * min(8, len(dec) // (2 * B))]
    nb = len(dec) // (2 * B)
    key = lambda r: (int(r["stream"]), int(r["start_sample"]))  # noqa: E731
    whole = sorted(clock.chains(submits(dec, (nb,), thresh=thresh)), key=key)
    assert len(whole) >= 1
    cuts = 0
    for sizes in [(1,) * nb] + [(k, nb - k) for k in range(1, nb)]:
        subs = submits(dec, sizes, thresh=thresh)
        cuts += sum(1 for recs in subs for r in recs if r["flags"] & CONT)
        got = sorted(clock.chains(subs), key=key)
        assert len(got) == len(whole)
        for a, b in zip(got, whole):
            assert a.tobytes() == b.tobytes(), (sizes, key(a))
    assert cuts >= 1 or name != "whb"  # the WHB telegram spans blocks


def test_merge_takes_the_ends_flags_and_spec_saturates():
    p = np.zeros(3, dtype=clock.CLOCK_DTYPE)
    p["flags"], p["n_samples"], p["n_segments"], p["n_silent"] = (OPEN, CONT | OPEN, CONT), (5000, 8192, 3000), (4, 8, 2), (0, 1, 0)
    p["start_sample"], p["thresh"] = (3192, 8192, 16384), (500, 600, 700)
    p["spec"][:, 0], p["spec"][:, 1], p["spec"][:, 2] = (1 << 63, 1 << 62, 1 << 62), (1 << 63, (1 << 63) - 1, 0), (5, 6, 7)
    m = clock.merge(p)
    assert (m["flags"], m["start_sample"], m["thresh"], m["n_samples"], m["n_segments"], m["n_silent"]) == (0, 3192, 500, 16192, 14, 1)
    assert m["spec"][:3].tolist() == [(1 << 64) - 1, (1 << 64) - 1, 18] and not m["spec"][3:].any()
    assert clock.merge(p[:2])["flags"] == OPEN and clock.merge(p[1:])["flags"] == CONT
    assert clock.merge([clock.merge(p[:2]), p[2]]).tobytes() == m.tobytes()


# ---- tfrec_gpu's merge: job.h in a stand-alone program
@pytest.fixture(scope="module")
def merge_driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("clock_merge") / "clock_merge_driver")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(parity.ROOT, "tests", "merge_driver.cpp")])
    return exe


def rec_line(f, r):
    v = [f] + [int(r[k]) for k in ("flags", "start_sample", "n_samples", "thresh", "n_segments", "n_silent")] + [int(x) for x in r["spec"]]
    return "rec " + " ".join("%d" % x for x in v)


def test_the_host_merge_prints_the_restatements_lines(merge_driver):
    """Two files through one slot, batches of 1 block: the golden WHB scene's first 6 blocks, whose telegram spans four of them, and
    the golden TFA_2 scene; then a file of hand-made records: the summary's guard cases, a saturating chain, a run without a segment."""
    files = [("a.iq", golden_dec("whb")[:2 * 6 * B]), ("b.iq", golden_dec("tfa_2")[:2 * 4 * B])]
    lines, want = ["file %s %d" % (name, len(dec) // (2 * B)) for name, dec in files] + ["file c.iq 64"], []
    for f, (name, dec) in enumerate(files):
        subs = submits(dec, (1,) * (len(dec) // (2 * B)))
        for recs in subs:
            lines.append("batch 1 %d" % f)
            lines += [rec_line(f, r) for r in recs]
        assert f or any(r["flags"] & CONT for recs in subs for r in recs)
        want += [clock.line(name, c) for c in clock.chains(subs)]
    hand = [rec_with({50: 1000, 49: 400, 51: 600}), rec_with({50: 1000, 49: 601, 51: 400}), rec_with({50: 1000, 49: 1000, 51: 1000}), rec_with({12: 7, 11: 7, 13: 7}),
            rec_with({12: 1000, 11: 1500, 13: 10}), rec_with({128: 1000, 129: 1500, 127: 10}), rec_with({128: 1000, 129: 900}),
            rec_with({11: 9, 129: 9}), rec_with({50: 1000}, 0), rec_with({j: (1 << 64) - 1 for j in range(4, 132)}),
            rec_with({60: (1 << 64) - 1, 59: (1 << 64) - 2, 61: 3})]
    for k, r in enumerate(hand):
        r["stream"], r["start_sample"] = 2, 8192 * k
        lines += ["batch 1 2", rec_line(2, r)]
        want.append(clock.line("c.iq", r))
    chain = np.zeros(3, dtype=clock.CLOCK_DTYPE)  # a chain whose spec saturates, across three batches
    chain["stream"], chain["flags"], chain["n_samples"], chain["n_segments"] = 2, (OPEN, CONT | OPEN, CONT), 8192, 8
    chain["start_sample"] = [8192 * (20 + k) for k in range(3)]
    chain["spec"][:, 46], chain["spec"][:, 45], chain["spec"][:, 47] = 1 << 63, (1 << 62, 1 << 61, 5), (7, 1 << 62, 1 << 62)
    for r in chain:
        lines += ["batch 1 2", rec_line(2, r)]
    m = clock.merge(chain)
    assert m["spec"][46] == (1 << 64) - 1 and m["n_segments"] == 24
    want.append(clock.line("c.iq", m))
    out = subprocess.run([merge_driver, "clock"], input="".join(ln + "\n" for ln in lines), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.splitlines() == want
    assert want[0].split()[4:] == ["27", "5997", "60.05"] and want[-5].endswith(" 1 - -") and want[-4].endswith(" 0 - -")


# ---- the struct, the exports, the command line
def test_the_struct_and_the_exports(tmp_path):
    D = clock.CLOCK_DTYPE
    assert D.itemsize == 1056 and api.CLOCK_DTYPE is D
    offs = [("stream", 0), ("flags", 4), ("start_sample", 8), ("n_samples", 16), ("thresh", 20), ("n_segments", 24), ("n_silent", 28),
            ("spec", 32)]
    assert [(f, D.fields[f][1]) for f in D.names] == offs
    src = tmp_path / "clock.c"
    src.write_text('#include <stddef.h>\n#include "tfrec_amd.h"\n'
                   "_Static_assert(sizeof(tfrec_amd_clock) == 1056, \"size\");\n" +
                   "".join("_Static_assert(offsetof(tfrec_amd_clock, %s) == %d, \"%s\");\n" % (f, o, f) for f, o in offs) +
                   "_Static_assert(sizeof(((tfrec_amd_clock *)0)->spec) == 1024, \"spec\");\n")
    subprocess.check_call(["cc", "-std=c11", "-fsyntax-only", "-I", os.path.join(parity.ROOT, "include"), str(src)])
    assert "tfrec_amd_enable_burst_clock" in api.EXPORTS and "tfrec_amd_read_burst_clocks" in api.EXPORTS
    L = api.load_library()
    for sym in ("tfrec_amd_enable_burst_clock", "tfrec_amd_read_burst_clocks"):
        getattr(L, sym)
    # no GPU is needed to be refused
    assert L.tfrec_amd_enable_burst_clock(None) == api.E_INVAL
    n = C.c_uint32(7)
    assert L.tfrec_amd_read_burst_clocks(None, None, 0, C.byref(n)) == api.E_INVAL and n.value == 7


def test_cli_clock_usage_errors(tmp_path):
    parity.build_cli()
    f = str(tmp_path / "missing.iq")

    out = parity.run_cli(["-C", "-X", f])
    assert out.returncode == 1 and "-C measures" in out.stderr
    out = parity.run_cli(["-M", "-Q", "-C", "-X", f])  # -M's own refusal comes first and is what it was
    assert out.returncode == 1 and "-M measures" in out.stderr
    out = parity.run_cli(["-Q", "-C", "-X", f])
    assert out.returncode == 1 and "-Q measures" in out.stderr
    out = parity.run_cli(["-h"])
    assert "-C " in out.stderr and "[-C]" in out.stderr
    for args in (["-C", "-k", str(tmp_path / "keep"), "-L", f], ["-C", "-K", str(tmp_path / "keep"), "-L", f]):
        out = parity.run_cli(args)
        assert out.returncode == 2 and "not with -C" in out.stderr, args
    for args in (["-C", "-L", f], ["-C", "-M", "-Q", "-L", f], ["-C", "-s", "50", "-L", f],
                 ["-C", "-S", str(tmp_path / "cap"), "-n", "1", "-L", f]):
        out = parity.run_cli(args)  # accepted: the file is looked for
        assert out.returncode == 2 and "missing.iq" in out.stderr, args
    out = parity.run_cli(["-C", "-R", str(tmp_path / "nothing")])  # accepted with -R: the capture is looked for
    assert out.returncode == 2 and "-R replays" not in out.stderr
