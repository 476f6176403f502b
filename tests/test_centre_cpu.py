"""The burst track's auto-centre mode without a GPU (tfrec_amd_enable_burst_track_auto, tfrec_amd_read_burst_track_centres, tfrec_gpu
-G rate,auto): the restatement tfrec_amd/track.py (head_centres, auto_tracks) against its per-sample form on crafted
rows and on the five golden scenes, the figures the feature was specified with, the golden telegrams under seven carrier offsets,
the mixed stream no single centre reads, hand-set histograms, the behaviour under cutting, tfrec_gpu's centre pieces
(tfrec_amd/host/job.h, compiled into a stand-alone program under the address and undefined-behaviour sanitizers), the record as the
C header declares it, the exports, the memory sums and what tfrec_gpu decides before it opens a device.

Everything is exact integers: there is no tolerance anywhere.  TFA_1 and WHB still do not slice (DESIGN.md 6t's limit): only the
two forms' agreement is asserted on them.  Nothing here is measured on real recordings."""
import itertools
import os
import subprocess

import numpy as np
import pytest

import centre_rows as C
import parity
from centre_rows import B, CONT, F, I, M, OPEN
from recorder_rows import GOLDEN, RATE, TELEGRAMS, golden_dec, rotated
from tfrec_amd import api, burst, capture, track

figures = lambda c: (int(c["n_counted"]), int(c["source"]), int(c["centre_hz"]), int(c["deviation_hz"]))  # noqa: E731


def table(*rows):
    """A run table by hand: (start, n[, flags]) of stream 0, packed in order."""
    t = np.zeros(len(rows), dtype=capture.RUN_DTYPE)
    off = 0
    for k, r in enumerate(rows):
        t[k]["start_sample"], t[k]["n_samples"], t[k]["thresh"] = r[0], r[1], C.T
        t[k]["flags"] = r[2] if len(r) > 2 else 0
        t[k]["pool_offset"] = off
        off += r[1]
    return t


def both(dec, thr, runs, K, fallback=0, state=None):
    """The vectorised form's records and state, held to the per-sample one's."""
    dec = np.ascontiguousarray(dec, dtype=np.int16).reshape(-1)
    a, sa = track.head_centres([dec], [thr], runs, K, [fallback], state)
    b, sb = track.head_centres_bruteforce([dec], [thr], runs, K, [fallback], state)
    assert a.dtype == b.dtype == track.CENTRE_DTYPE and a.tobytes() == b.tobytes()
    assert np.array_equal(sa["index"], sb["index"]) and np.array_equal(sa["centre_hz"], sb["centre_hz"])
    assert a["index"].tolist() == [track.index_of(h) for h in a["centre_hz"]] and not a["reserved"].any()
    return a, sa


def one(z, K=1024, fallback=0, pad=50):
    """The centre record of a burst z (int16 [n, 2]) that stands alone on a floor, its run `pad` samples longer than it."""
    row = C.floor(len(z) + 2 * pad + 1, 9)
    row[1:1 + len(z)] = z
    return both(row, C.T, table((1, len(z) + pad)), K, fallback)[0][0]


def same_subs(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert all(p.tobytes() == q.tobytes() for p, q in zip(x, y))


# ---- the restatement against its per-sample form
@pytest.mark.parametrize("K", [64, 1024, 4096])
def test_the_two_forms_agree_on_crafted_rows(K):
    rows = C.hand_rows()
    for s in range(2):
        row = rows[s].reshape(-1)
        runs = capture.captures(row, 0x2F, C.T)[0]
        cen = both(row, C.T, runs, K, C.FALLBACK[s])[0]
        if K == 1024:
            assert {(s, int(c["start_sample"])): figures(c) for c in cen} == {k: v for k, v in C.HAND_1024.items() if k[0] == s}
        if K == 64:  # k = 1 .. 63: 63 products at the most, never the 64 a measured centre needs
            assert (cen["source"] == F).all() and (cen["n_counted"] <= 63).all() and (cen["centre_hz"] == C.FALLBACK[s]).all()
        same_subs(C.submits(row, (1, 1), 5, K, C.FALLBACK[s], thresh=C.T), C.submits(row, (1, 1), 5, K, C.FALLBACK[s], thresh=C.T, brute=True))


@pytest.mark.parametrize("name", GOLDEN)
def test_the_two_forms_agree_on_the_golden_scenes(name):
    d = golden_dec(name)
    nb = len(d) // (2 * B)
    L = track.smooth_of(RATE[name])
    for sizes in ((nb,), (1, nb - 1)):
        same_subs(C.submits(d, sizes, L, 1024), C.submits(d, sizes, L, 1024, brute=True))
    if name in ("tfa_1", "whb"):  # they still do not slice (6t's limit); their heads are all but unmodulated
        cen = C.submits(d, (nb,), L, 1024)[0][0]
        assert len(cen) >= 1 and (cen["source"] == M).all() and (cen["deviation_hz"] <= 6000).all()


# ---- the figures the feature was specified with
@pytest.mark.parametrize("name,hz", sorted(C.FIGURES))
def test_the_golden_figures(name, hz):
    d = rotated(golden_dec(name), hz) if hz else golden_dec(name)
    cen = C.submits(d, (len(d) // (2 * B),), track.smooth_of(RATE[name]), 1024)[0][0]
    assert [figures(c) for c in cen] == [(1023, M) + f for f in C.FIGURES[name, hz]]


@pytest.mark.parametrize("hz", C.ROTATIONS)
@pytest.mark.parametrize("name", sorted(TELEGRAMS))
def test_the_golden_telegrams_read_under_every_rotation(name, hz):
    d = rotated(golden_dec(name), hz) if hz else golden_dec(name)
    cen, trk = C.chains(C.submits(d, (len(d) // (2 * B),), track.smooth_of(RATE[name]), 1024))
    assert len(trk) == 2 and all(c["source"] == M and c["n_counted"] == 1023 for c in cen)
    for c, t, tel in zip(cen, trk, TELEGRAMS[name]):
        assert C.reads(t, RATE[name], tel), (tel, figures(c))


def test_the_mixed_stream_reads_in_auto_mode_and_about_no_single_centre():
    d, rate = C.mixed_dec(), RATE["tfa_2"]
    L = track.smooth_of(rate)
    cen, trk = C.chains(C.submits(d, (len(d) // (2 * B),), L, 1024))
    assert [figures(c) for c in cen] == [(1023, M) + f for f in C.MIXED_FIGURES]
    assert [C.reads(t, rate, tel) for t, tel in zip(trk, TELEGRAMS["tfa_2"])] == [True, True]
    assert int(cen[0]["start_sample"]) + int(cen[0]["n_samples"]) < C.MIXED_CUT < int(cen[1]["start_sample"])  # the cut is between them
    for centre in (-40000, -20000, 0, 20000, 40000):
        fixed = C.fixed(d, L, centre)
        assert len(fixed) == 2 and sum(C.reads(t, rate, tel) for t, tel in zip(fixed, TELEGRAMS["tfa_2"])) <= 1, centre


# ---- hand-set histograms
def test_63_products_fall_back_and_64_are_measured():
    assert figures(one(C.tone([18000] * 64), fallback=-7000)) == (63, F, -7000, 0)
    assert figures(one(C.tone([18000] * 65), fallback=-7000)) == (64, M, 18000, 0)
    assert figures(one(C.tone([18000] * 65), K=64)) == (63, F, 0, 0)  # the head ends before the 64th product
    assert one(C.tone([18000] * 64), fallback=-7000)["index"] == track.index_of(-7000) == 4021


def test_a_bin_with_exactly_a_sixteenth_is_occupied_and_one_below_is_not():
    for p in (160, 161, 175, 176, 177):  # (P + 15) // 16 = 10, 11, 11, 11, 12
        need = (p + 15) // 16
        for n_other, want in ((need, (p, M, -9000, 39000)), (need - 1, (p, M, 30000, 0))):
            f = np.full(p + 1, 30000)
            f[50:50 + n_other] = -48000
            assert figures(one(C.tone(f))) == want, (p, n_other)


def test_the_outermost_bins_and_a_histogram_without_an_occupied_bin():
    assert figures(one(C.tone([-192000] * 100 + [186000] * 100))) == (199, M, -3000, 189000)  # lo = -32, hi = 31
    assert figures(one(C.tone([-192000] * 100))) == (99, M, -192000, 0) and one(C.tone([-192000] * 100))["index"] == 2048
    assert figures(one(C.tone([186000] * 100))) == (99, M, 186000, 0)
    # 129 samples, 4 products in each of 32 bins: a sixteenth is 8, no bin has it -- the fallback, whatever P
    spread = np.repeat(np.arange(-16, 16) * 6000, 4)
    assert figures(one(C.tone(np.concatenate([[0], spread])), fallback=55000)) == (128, F, 55000, 0)


def test_samples_under_the_threshold_drop_both_products_they_touch():
    z = C.tone([42000] * 300)
    z[[100, 101, 200]] = 0
    assert figures(one(z)) == (299 - 3 - 2, M, 42000, 0)
    z[1::2] = 0  # every other sample: no product has both
    assert figures(one(z, fallback=9000)) == (0, F, 9000, 0)
    # the mask's bits are taken as given: a threshold above the burst counts nothing
    row = C.floor(400, 9)
    row[1:301] = C.tone([42000] * 300)
    assert figures(both(row, 20000, table((1, 350)), 1024, 9000)[0][0]) == (0, F, 9000, 0)
    over = np.zeros(400, dtype=bool)
    over[1:101] = True
    assert figures(both(row, over, table((1, 350)), 1024, 9000)[0][0]) == (99, M, 42000, 0)


def test_a_run_shorter_than_k_and_a_head_shorter_than_the_burst():
    z = C.tone([-24000] * 200 + [60000] * 200)  # bins -4 and 10
    assert figures(one(z, K=4096)) == (399, M, 18000, 42000)  # the whole run: n < K
    assert figures(one(z, K=200)) == (199, M, -24000, 0)  # k < 200: the second tone's first product is k = 200
    assert figures(one(z, K=201)) == (200, M, -24000, 0)  # one product of 200: not a sixteenth
    assert figures(one(z, K=220)) == (219, M, 18000, 42000)  # 20 of 219: (219 + 15) // 16 = 14


def test_a_head_across_a_block_boundary_and_a_continuation():
    row = C.floor(2 * B, 5)
    row[B - 300:B + 900] = C.fsk(1200, -30000, seed=4)
    whole = both(row, C.T, table((B - 300, 1200 + C.W - 1)), 1024, 0)
    assert figures(whole[0][0]) == (1023, M, -30000, 30000) and whole[1]["index"][0] == -1  # not OPEN: nothing is carried
    # the same run cut at the boundary: the first piece is centred on its 300 samples, and the second inherits that
    first = both(row[:B], C.T, table((B - 300, 300, OPEN)), 1024, 0)
    assert figures(first[0][0]) == (299, M, -30000, 30000) and first[1]["index"][0] == track.index_of(-30000)
    second = both(row[B:], C.T, table((0, 900 + C.W - 1, CONT)), 1024, 12000, first[1])
    assert figures(second[0][0]) == (0, I, -30000, 0) and second[0][0]["index"] == first[0][0]["index"]
    # without a carried centre -- the OPEN piece had no record, or the context has just begun -- the set centre is used
    lost = both(row[B:], C.T, table((0, 900 + C.W - 1, CONT)), 1024, 12000, None)
    assert figures(lost[0][0]) == (0, F, 12000, 0) and lost[0][0]["index"] == track.index_of(12000)


# ---- cuts
def compositions(n):
    return [c for k in range(1, n + 1) for c in itertools.product(range(1, n + 1), repeat=k) if sum(c) == n]


@pytest.mark.parametrize("name", ["tfa_2", "tfa_3"])
def test_every_block_cut_merges_to_the_uncut_result(name):
    d = golden_dec(name)
    nb = len(d) // (2 * B)
    L = track.smooth_of(RATE[name])
    ucen, utrk = C.chains(C.submits(d, (nb,), L, 1024))
    assert len(compositions(nb)) == 2 ** (nb - 1) and len(ucen) == 2
    for sizes in compositions(nb):  # the bursts lie inside blocks: every first piece holds the head
        cen, trk = C.chains(C.submits(d, sizes, L, 1024))
        assert [c.tobytes() for c in cen] == [c.tobytes() for c in ucen], sizes
        for a, b in zip(trk, utrk):
            assert np.array_equal(a.bits, b.bits) and a["n_ones"] == b["n_ones"] and a["last_over"] == b["last_over"], sizes


def test_a_chain_is_centred_on_what_its_first_piece_has():
    rows = C.hand_rows()
    # stream 1: 500 samples of the burst ahead of the cut -- centred on those, and the continuation keeps that centre
    subs = C.submits(rows[1].reshape(-1), (1, 1), 5, 1024, C.FALLBACK[1], thresh=C.T)
    o, c = subs[0][0][-1], subs[1][0][0]
    assert o["flags"] == OPEN and o["n_samples"] == 500 and figures(o) == (499, M, 48000, 30000)
    assert c["flags"] & CONT and figures(c) == (0, I, 48000, 0) and c["index"] == o["index"]
    merged = [m for m in C.chains(subs)[0] if m["start_sample"] == B - 500][0]
    assert figures(merged) == (499, M, 48000, 30000) and merged["n_samples"] == 2000 + C.W - 1 and merged["flags"] == 0
    # stream 0: 3 samples ahead of the cut -- the fallback, which the continuation inherits, where the uncut run is measured
    subs = C.submits(rows[0].reshape(-1), (1, 1), 5, 1024, C.FALLBACK[0], thresh=C.T)
    o, c = subs[0][0][-1], subs[1][0][0]
    assert o["flags"] == OPEN and o["n_samples"] == 3 and figures(o) == (2, F, C.FALLBACK[0], 0)
    assert c["flags"] & CONT and figures(c) == (0, I, C.FALLBACK[0], 0)
    uncut = C.chains(C.submits(rows[0].reshape(-1), (2,), 5, 1024, C.FALLBACK[0], thresh=C.T))[0]
    assert figures([m for m in uncut if m["start_sample"] == B - 3][0]) == C.HAND_1024[0, B - 3]
    # the piece behind a restart does not continue: it is measured as a first piece, on the burst's other 1500 samples
    subs = C.submits(rows[1].reshape(-1), (1, 1), 5, 1024, C.FALLBACK[1], thresh=C.T, restarts=(1,))
    r = subs[1][0][0]
    assert r["flags"] == 0 and r["start_sample"] == 0 and figures(r) == (1023, M, 48000, 30000)
    assert len(C.chains(subs, restarts={1: [0]})[0]) == len(subs[0][0]) + len(subs[1][0])


# ---- tfrec_gpu's centre pieces: job.h in a stand-alone program
@pytest.fixture(scope="module")
def centre_driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("centre") / "centre_driver")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(parity.ROOT, "tests", "centre_driver.cpp")])
    return exe


def test_the_host_merges_and_prints_the_restatements_centres(centre_driver):
    cases = [(C.hand_rows()[s].reshape(-1), sizes, C.T, C.FALLBACK[s]) for s in range(2) for sizes in ((2,), (1, 1))]
    cases += [(C.mixed_dec(), sizes, 500, 0) for sizes in ((4,), (2, 2), (1, 1, 1, 1))]
    for dec, sizes, thresh, fb in cases:
        subs = C.submits(dec, sizes, 5, 1024, fb, thresh=thresh)
        lines = []
        for cen, recs, _ in subs:
            lines += ["piece %d %d %d %d %d %d %d %d %d" % (c["flags"], c["start_sample"], c["n_samples"], t["last_over"], c["n_counted"],
                                                            c["source"], c["centre_hz"], c["deviation_hz"], c["index"]) for c, t in zip(cen, recs)]
            lines.append("batch")
        lines.append("batch")  # (a chain still open behind the last batch ends with a batch that does not continue it)
        cen, trk = C.chains(subs + [(np.zeros(0, dtype=track.CENTRE_DTYPE), np.zeros(0, dtype=track.TRACK_DTYPE), np.zeros(0, dtype="<u4"))])
        want = []
        for c, t in zip(cen, trk):
            want += [track.centre_line("f.iq", c), "merged %d %d %d %d" % (c["flags"], c["n_samples"], t["last_over"], c["index"])]
        out = subprocess.run([centre_driver], input="".join(ln + "\n" for ln in lines), capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        assert out.stdout.splitlines() == want and len(want) >= 4
    rec = np.zeros((), dtype=track.CENTRE_DTYPE)
    rec["start_sample"], rec["n_samples"], rec["n_counted"], rec["centre_hz"], rec["deviation_hz"] = 7, 900, 899, -141000, 33000
    assert track.centre_line("a b", rec) == "centre a b 7 900 899 -141000 33000 m"
    rec["source"], rec["deviation_hz"] = F, 0
    assert track.centre_line("x", rec) == "centre x 7 900 899 -141000 - f"
    rec["source"] = I
    assert track.centre_line("x", rec).endswith(" - i")


# ---- the record, the exports, the memory sums, the command line
def test_the_record_the_exports_and_the_memory_sums(tmp_path):
    D = track.CENTRE_DTYPE
    offs = [("stream", 0), ("flags", 4), ("start_sample", 8), ("n_samples", 16), ("thresh", 20), ("n_counted", 24), ("source", 28),
            ("centre_hz", 32), ("deviation_hz", 36), ("index", 40), ("reserved", 44)]
    assert D.itemsize == 48 and [(f, D.fields[f][1]) for f in D.names] == offs
    src = tmp_path / "centre.c"
    src.write_text('#include <stddef.h>\n#include "tfrec_amd.h"\n'
                   "_Static_assert(sizeof(tfrec_amd_track_centre) == 48, \"size\");\n" +
                   "".join("_Static_assert(offsetof(tfrec_amd_track_centre, %s) == %d, \"%s\");\n" % (f, o, f) for f, o in offs) +
                   "_Static_assert(TFREC_AMD_CENTRE_MEASURED == %d && TFREC_AMD_CENTRE_FALLBACK == %d && TFREC_AMD_CENTRE_INHERITED == %d, "
                   "\"sources\");\n" % (M, F, I))
    subprocess.check_call(["cc", "-std=c11", "-fsyntax-only", "-I", os.path.join(parity.ROOT, "include"), str(src)])
    names = ("tfrec_amd_enable_burst_track_auto", "tfrec_amd_read_burst_track_centres")
    L = api.load_library()
    for sym in names:
        assert sym in api.EXPORTS
        getattr(L, sym)
    # no GPU is needed to be refused
    assert L.tfrec_amd_enable_burst_track_auto(None, 5, 1024) == api.E_INVAL
    assert L.tfrec_amd_read_burst_track_centres(None, None, 0, None) == api.E_INVAL
    assert hasattr(api.Receiver, "enable_burst_track_auto") and hasattr(api.Receiver, "read_burst_track_centres")
    # per FIFO set max_runs * 48 bytes, per stream the carried 8; the track's own sums stay what they were
    assert track.device_bytes(3, 10, 65) == api.FIFO_DEPTH * (400 + 12 + 12) + 3 * 68
    assert track.auto_device_bytes(3, 10, 65) == track.device_bytes(3, 10, 65) + api.FIFO_DEPTH * 480 + 24
    head = open(os.path.join(parity.ROOT, "include", "tfrec_amd.h")).read()
    for sym in names:
        assert "int %s(tfrec_amd_ctx *ctx" % sym in head
    for limit in ("first piece", "not circular", "real recordings"):
        assert limit in head[head.index("Auto-centre track"):head.index("tfrec_amd_enable_burst_track_auto(tfrec_amd_ctx")]
    assert track.index_of(0) == 0 and burst.N_BINS == 64 and track.HEAD_MIN == track.COUNT_MIN == 64 and track.HEAD_MAX == 4096


def test_cli_auto_usage_errors_and_accepted_forms(tmp_path):
    parity.build_cli()
    f = str(tmp_path / "missing.iq")
    for args in (["-G", "17240,auto", "-O", "2000", "-L", f], ["-O", "2000", "-G", "17240,auto", "-L", f]):
        out = parity.run_cli(args)
        assert out.returncode == 1 and "not with -O" in out.stderr, args
    for bad in ("17240,aut", "17240,auto,1", "17240,Auto", "auto", ",auto", "999,auto", "96001,auto", "17240,auto "):
        out = parity.run_cli(["-G", bad, "-L", f])
        assert out.returncode == 1 and "bad -G" in out.stderr, bad
    # refused wherever -G is, with -G's own messages
    for args in (["-G", "4800,auto", "-X", f], ["-G", "4800,auto", "-s", "50", "-L", f], ["-G", "4800,auto", "-A", "-L", f]):
        out = parity.run_cli(args)
        assert out.returncode == 1 and "-G reads" in out.stderr, args
    for k in ("-k", "-K"):
        out = parity.run_cli(["-G", "4800,auto", k, str(tmp_path / "keep"), "-L", f])
        assert out.returncode == 2 and "not with -G" in out.stderr, k
    out = parity.run_cli(["-h"])
    assert "-G r,auto" in out.stderr and "[-G rate,auto]" in out.stderr and "centre <file>" in out.stderr
    assert "-G r[,c]" in out.stderr and "[-G rate[,centre_hz]]" in out.stderr and "[-O level]" in out.stderr  # the others' lines stay
    for args in (["-G", "17240,auto", "-L", f], ["-G", "1000,auto", "-L", f], ["-G", "96000,auto", "-L", f],
                 ["-G", "17240,auto", "-Y", "2dd4,0,4", "-L", f], ["-G", "17240,auto", "-M", "-Q", "-C", "-L", f],
                 ["-G", "17240,auto", "-S", str(tmp_path / "cap"), "-n", "1", "-L", f], ["-G", "17240,auto", "-d", "0", "-L", f]):
        out = parity.run_cli(args)  # accepted: the file is looked for
        assert out.returncode == 2 and "missing.iq" in out.stderr, args
    out = parity.run_cli(["-G", "17240,auto", "-R", str(tmp_path / "nothing")])  # accepted with -R: the capture is looked for
    assert out.returncode == 2 and "-R replays" not in out.stderr and "bad -G" not in out.stderr
