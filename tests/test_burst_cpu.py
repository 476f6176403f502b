"""The burst meter without a GPU (tfrec_amd_enable_burst_meter, tfrec_gpu -M): the restatement tfrec_amd/burst.py
against its per-sample form, the argmax bin against a float atan2 and against the evaluation the kernel uses, a quantised tone, the
behaviour under cutting, the summary on the golden TFA_2 scene, tfrec_gpu's merge (tfrec_amd/host/job.h, compiled into a stand-alone
program under the address and undefined-behaviour sanitizers), the struct and the exports, and what tfrec_gpu decides before it opens
a device.

Everything is an exact integer; the one tolerance, of the tone's mean frequency, is derived where it is used."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import parity
from tfrec_amd import api, burst, capture, levels, tune
from meter_rows import crafted_dec

B = levels.BLOCK_DEC
GOLDEN = ("tfa_1", "tfa_2", "tfa_3", "tx22", "whb")
ZERO = [np.zeros(2, dtype=np.int16)]


def golden_dec(name):
    return np.load(os.path.join(parity.ROOT, "tests", "golden", "iq_%s.npz" % name))["dec"]


def records(dec, types=0x2F, thresh=500, state=None, prev=ZERO, base=0):
    runs, _, st = capture.captures(dec, types, thresh, state)
    return burst.bursts([dec], runs, prev, base=[base]), runs, st


def same(a, b):
    assert a.dtype == b.dtype == burst.BURST_DTYPE and a.tobytes() == b.tobytes()


# ---- the restatement against its per-sample form
@pytest.mark.parametrize("types,thresh", [(0x2F, 500), (0x02, 0), (0x01, 500)])
def test_the_vectorised_form_equals_the_per_sample_one_on_crafted_samples(types, thresh):
    W = max(levels.windows(types))
    dec, _ = crafted_dec(W, types)
    dec = dec.reshape(-1)
    runs = capture.captures(dec, types, thresh)[0]
    assert len(runs) >= 4
    want = burst.bursts_bruteforce([dec], runs, ZERO)
    same(burst.bursts([dec], runs, ZERO), want)
    assert (want["hist"].sum(axis=1) == want["n_products"]).all() and (want["n_products"] <= want["n_samples"] - 1).all()
    assert want["pwr_max"].max() == 6000


@pytest.mark.parametrize("name", GOLDEN)
def test_the_vectorised_form_equals_the_per_sample_one_on_the_golden_scenes(name):
    dec = golden_dec(name)
    runs = capture.captures(dec, 0x2F, 500)[0]
    assert len(runs) >= 1
    same(burst.bursts([dec], runs, ZERO), burst.bursts_bruteforce([dec], runs, ZERO))


# ---- the bin
def boundaries():
    """The product on the boundary between directions j and j + 1, j = 0..63: both score the same, every other direction less."""
    c, s = burst.directions()
    return [(s[(j + 1) % 64] - s[j], c[j] - c[(j + 1) % 64]) for j in range(64)]


def test_the_bin_equals_a_float_atan2_away_from_the_boundaries():
    beta = np.array([math.atan2(crs, dot) % (2 * math.pi) for dot, crs in boundaries()])  # ascending: boundary j lies behind direction j
    assert (np.diff(beta) > 0).all() and abs(beta[0] - math.pi / 64) < 3e-4
    rng = np.random.default_rng(5)
    n = 0
    for lim in (1 << 31, 1 << 20, 300):
        for dot, crs in rng.integers(-lim, lim + 1, (4000, 2)).tolist():
            if dot == 0 and crs == 0:
                continue
            th = math.atan2(crs, dot) % (2 * math.pi)
            gap = np.abs((beta - th + math.pi) % (2 * math.pi) - math.pi).min()
            if gap <= 1e-6:
                continue
            want = int(np.searchsorted(beta, th)) % 64
            assert burst.bin_of(dot, crs) == want == burst.bin_fast(dot, crs), (dot, crs)
            n += 1
    assert n > 11000
    assert burst.bin_of(0, 0) is None and burst.bin_fast(0, 0) is None


def test_ties_go_to_the_lower_bin_and_the_fast_evaluation_agrees_everywhere_near_them():
    c, s = burst.directions()
    C4 = tune.table()[0]
    k = np.arange(4096)
    assert (C4[(-k) % 4096] == C4).all() and (C4[(2048 - k) % 4096] == -C4).all()  # what the quarter turn relies on
    ds = [s[j + 1] - s[j] for j in range(16)]
    dc = [c[j] - c[j + 1] for j in range(16)]
    assert all(v > 0 for v in ds + dc) and all(dc[j] * ds[j + 1] < dc[j + 1] * ds[j] for j in range(15))  # ... and the count
    for j, (dot, crs) in enumerate(boundaries()):
        score = [dot * c[i] + crs * s[i] for i in range(64)]
        best = max(score)
        assert [i for i in range(64) if score[i] == best] == sorted([j, (j + 1) % 64])  # a tie of exactly these two
        for m in (1, 2, 7, 1000, 600000):  # (600000 * 3212 < 2^31)
            assert burst.bin_of(m * dot, m * crs) == burst.bin_fast(m * dot, m * crs) == min(j, (j + 1) % 64)
            for dd, dq in ((1, 0), (-1, 0), (0, 1), (0, -1)):
                v = (m * dot + dd, m * crs + dq)
                assert burst.bin_of(*v) == burst.bin_fast(*v) and burst.bin_of(*v) in (j, (j + 1) % 64), (j, v)
    for q, (dot, crs) in enumerate(((1, 0), (0, 1), (-1, 0), (0, -1))):  # the axes, and the diagonals
        for m in (1, 32767, 1 << 31):
            assert burst.bin_of(m * dot, m * crs) == burst.bin_fast(m * dot, m * crs) == 16 * q
            d2, c2 = m * (dot - crs), m * (crs + dot)
            assert burst.bin_of(d2, c2) == burst.bin_fast(d2, c2) == 16 * q + 8
    assert [burst.signed_bin(j) for j in (0, 31, 32, 63)] == [0, 31, -32, -1]


# ---- a tone
@pytest.mark.parametrize("f", [0, 18000, 31000, -47000, 100000, -150000, 185000])
def test_a_quantised_tone_falls_into_its_bin_and_its_mean_frequency_is_within_the_bound(f):
    A, n = 20000, 3 * B
    ph = 2 * np.pi * f / 384000.0 * np.arange(n) + 0.3
    dec = np.stack([np.round(A * np.cos(ph)), np.round(A * np.sin(ph))], 1).astype(np.int16).reshape(-1)
    recs, runs, _ = records(dec)
    assert len(recs) == 1 and recs[0]["n_samples"] == n and recs[0]["n_products"] == n - 1
    b = round(f / 6000)
    assert recs[0]["hist"][b % 64] == n - 1  # every product
    assert burst.summary(recs[0]) == (6000 * b, 0)
    # A sample is off by at most 0.7071 / A rad (half a step per component), a product by twice that, and the sum of vectors
    # inside a cone stays inside it
    got = math.atan2(int(recs[0]["sum_crs"]), int(recs[0]["sum_dot"])) * 384000 / (2 * math.pi)
    assert abs(got - f) <= 384000 / (2 * math.pi) * 1.4143 / A, (got, f)
    assert recs[0]["pwr_max"] <= int(1.4143 * A) + 2 and abs(int(recs[0]["energy"]) - n * A * A) < n * 2 * 1.4143 * A


# ---- cutting
@pytest.mark.parametrize("name,thresh", [("tfa_2", 500), ("whb", 500), ("tfa_1", 0)])
def test_the_merged_chains_do_not_depend_on_the_cut(name, thresh):
    dec = golden_dec(name)[:2 * 4 * B]
    if thresh == 0:  # an auto stream over noise that keeps it triggered: one chain across every cut
        dec = np.random.default_rng(11).integers(-400, 401, 2 * 4 * B).astype(np.int16)
    whole = burst.chains([records(dec, 0x2F, thresh)[0]])
    assert len(whole) >= 1
    for sizes in ((1, 3), (2, 2), (1, 1, 1, 1)):
        st, prev, pos, subs = None, ZERO, 0, []
        for nb in sizes:
            part = dec[2 * pos * B:2 * (pos + nb) * B]
            recs, runs, st = records(part, 0x2F, thresh, st, prev, pos * B)
            subs.append(recs)
            prev, pos = [part.reshape(-1, 2)[-1]], pos + nb
        got = burst.chains(subs)
        if thresh == 0:
            assert any(int(r["flags"]) & capture.RUN_CONTINUES for recs in subs[1:] for r in recs)
        key = lambda r: int(r["start_sample"])  # noqa: E731
        assert [c.tobytes() for c in sorted(got, key=key)] == [c.tobytes() for c in sorted(whole, key=key)], sizes


def test_the_zero_rule_and_the_first_product_of_a_run_at_sample_0():
    dec = np.zeros((B, 2), dtype=np.int16)
    dec[0] = (3000, 0)  # a trigger at the submit's first sample, then zeros: every later product is (0, 0) and skipped
    dec[5] = (0, 2000)
    dec[6] = (-2000, 0)  # a quarter turn up: bin 16
    prev = [np.array([0, 1000], dtype=np.int16)]  # the pair ahead of the submit: a quarter turn DOWN to sample 0
    run = np.zeros(1, dtype=capture.RUN_DTYPE)
    run[0]["n_samples"], run[0]["thresh"] = 700, 500
    fresh = burst.bursts([dec.reshape(-1)], run, prev)[0]
    assert fresh["n_products"] == 1 and fresh["hist"][16] == 1 and (fresh["sum_dot"], fresh["sum_crs"]) == (0, 4000000)
    assert fresh["energy"] == 9000000 + 2 * 4000000 and fresh["pwr_max"] == 3000
    run[0]["flags"] = capture.RUN_CONTINUES  # the piece continues a chain: the product with the pair ahead is this piece's
    cont = burst.bursts([dec.reshape(-1)], run, prev)[0]
    assert cont["n_products"] == 2 and cont["hist"][16] == 1 and cont["hist"][48] == 1 and cont["sum_crs"] == 4000000 - 3000000
    same(burst.bursts_bruteforce([dec.reshape(-1)], run, prev), burst.bursts([dec.reshape(-1)], run, prev))
    assert burst.summary(cont) == (0, 96000)  # bins 16 and -16 both hold half: lo = -16, hi = 16
    empty = cont.copy()
    empty["n_products"], empty["hist"] = 0, 0
    assert burst.summary(empty) is None and burst.line("x", empty) == "burst x 0 700 3000 - -"


# ---- the summary on the golden TFA_2 scene
def rotated(dec, f):
    d = dec.reshape(-1, 2).astype(np.float64)
    w = (d[:, 0] + 1j * d[:, 1]) * np.exp(2j * np.pi * f * np.arange(len(d)) / 384000.0)
    return np.stack([np.round(w.real), np.round(w.imag)], 1).astype(np.int16).reshape(-1)


def test_summary_of_the_golden_tfa_2_burst_and_of_its_rotations():
    dec = golden_dec("tfa_2")
    runs = capture.captures(dec, 0x2F, 500)[0][:1]  # the first telegram's window
    rec = burst.bursts([dec], runs, ZERO)[0]
    assert (int(rec["start_sample"]), int(rec["n_samples"]), int(rec["n_products"])) == (10003, 2167, 2164)
    thr = (2164 + 15) // 16
    occupied = {burst.signed_bin(j): int(h) for j, h in enumerate(rec["hist"]) if h >= thr}
    assert occupied == {-5: 489, -4: 143, -1: 142, 0: 139, 4: 136, 5: 217, 6: 156}  # the two FSK peaks and the transitions between them
    assert burst.summary(rec) == (3000, 33000)
    assert burst.line("f.iq", rec) == "burst f.iq 10003 2167 8306 3000 33000"
    # rotated (the same samples, the same table): the centre moves by the rotation to within one bin, the rule's quantisation
    for f, want in ((20000, (21000, 33000)), (-35000, (-33000, 33000)), (-90000, (-87000, 33000))):
        got = burst.summary(burst.bursts([rotated(dec, f)], runs, ZERO)[0])
        assert got == want and abs(got[0] - 3000 - f) <= 6000


# ---- tfrec_gpu's merge: job.h in a stand-alone program
@pytest.fixture(scope="module")
def merge_driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("burst_merge") / "burst_merge_driver")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(parity.ROOT, "tests", "merge_driver.cpp")])
    return exe


def rec_line(f, r):
    v = [f, int(r["flags"]), int(r["start_sample"]), int(r["n_samples"]), int(r["thresh"]), int(r["pwr_max"]), int(r["n_products"]),
         int(r["sum_dot"]), int(r["sum_crs"]), int(r["energy"])] + [int(h) for h in r["hist"]]
    return "rec " + " ".join("%d" % x for x in v)


def test_the_host_merge_prints_the_restatements_lines(merge_driver):
    """Two files through one slot (-n 1), batches of 1 block: the golden TFA_2 scene's 4 blocks, then 3 blocks of noise that keeps
    an auto stream triggered up to the file's end -- its chain is flushed there, not carried into nothing."""
    noise = np.random.default_rng(12).integers(-400, 401, 2 * 3 * B).astype(np.int16)
    files = [("a.iq", golden_dec("tfa_2")[:2 * 4 * B], 500), ("b.iq", noise, 0)]
    lines, want = [], []
    for name, dec, _ in files:
        lines.append("file %s %d" % (name, len(dec) // (2 * B)))
    for f, (name, dec, thresh) in enumerate(files):
        st, prev, subs = None, ZERO, []
        for k in range(len(dec) // (2 * B)):
            part = dec[2 * k * B:2 * (k + 1) * B]
            recs, _, st = records(part, 0x2F, thresh, st, prev, k * B)
            prev = [part.reshape(-1, 2)[-1]]
            subs.append(recs)
            lines.append("batch 1 %d" % f)
            lines += [rec_line(f, r) for r in recs]
        chains = burst.chains(subs)
        assert any(int(c["n_samples"]) > B for c in chains) or f == 0
        want += [burst.line(name, c) for c in chains]
    out = subprocess.run([merge_driver, "burst"], input="".join(ln + "\n" for ln in lines), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.splitlines() == want and len(want) >= 3
    assert want[-1].split()[3] == str(3 * B - int(want[-1].split()[2]))  # the noise file's chain reaches the file's end


# ---- the struct, the exports, the command line
def test_the_struct_and_the_exports(tmp_path):
    assert burst.BURST_DTYPE.itemsize == 320 and api.BURST_DTYPE is burst.BURST_DTYPE
    assert [burst.BURST_DTYPE.fields[f][1] for f in burst.BURST_DTYPE.names] == [0, 4, 8, 16, 20, 24, 28, 32, 40, 48, 56, 312]
    src = tmp_path / "burst.c"
    src.write_text('#include <stddef.h>\n#include "tfrec_amd.h"\n'
                   "_Static_assert(sizeof(tfrec_amd_burst) == 320, \"size\");\n"
                   "_Static_assert(offsetof(tfrec_amd_burst, stream) == 0 && offsetof(tfrec_amd_burst, flags) == 4 && "
                   "offsetof(tfrec_amd_burst, start_sample) == 8 && offsetof(tfrec_amd_burst, n_samples) == 16 && "
                   "offsetof(tfrec_amd_burst, thresh) == 20 && offsetof(tfrec_amd_burst, pwr_max) == 24 && "
                   "offsetof(tfrec_amd_burst, n_products) == 28 && offsetof(tfrec_amd_burst, sum_dot) == 32 && "
                   "offsetof(tfrec_amd_burst, sum_crs) == 40 && offsetof(tfrec_amd_burst, energy) == 48 && "
                   "offsetof(tfrec_amd_burst, hist) == 56, \"layout\");\n")
    subprocess.check_call(["cc", "-std=c11", "-fsyntax-only", "-I", os.path.join(parity.ROOT, "include"), str(src)])
    assert "tfrec_amd_enable_burst_meter" in api.EXPORTS and "tfrec_amd_read_bursts" in api.EXPORTS
    L = api.load_library()
    for sym in ("tfrec_amd_enable_burst_meter", "tfrec_amd_read_bursts"):
        getattr(L, sym)
    # no GPU is needed to be refused
    assert L.tfrec_amd_enable_burst_meter(None) == api.E_INVAL
    n = C.c_uint32(7)
    assert L.tfrec_amd_read_bursts(None, None, 0, C.byref(n)) == api.E_INVAL and n.value == 7


def test_cli_meter_usage_errors(tmp_path):
    parity.build_cli()
    f = str(tmp_path / "missing.iq")

    out = parity.run_cli(["-M", "-X", f])
    assert out.returncode == 1 and "-M measures" in out.stderr
    out = parity.run_cli(["-h"])
    assert "-M " in out.stderr
    for args in (["-M", "-L", f], ["-M", "-s", "50", "-L", f], ["-M", "-S", str(tmp_path / "cap"), "-n", "1", "-L", f]):
        out = parity.run_cli(args)  # accepted: the file is looked for
        assert out.returncode == 2 and "missing.iq" in out.stderr, args
    out = parity.run_cli(["-M", "-R", str(tmp_path / "nothing")])  # accepted with -R: the capture is looked for
    assert out.returncode == 2 and "-R replays" not in out.stderr
