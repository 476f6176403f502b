"""The burst track's phase mode without a GPU (tfrec_amd_enable_burst_track_phase, tfrec_gpu -G rate,psk): the
restatement tfrec_amd/track.py (head_carriers, phase_tracks) against its per-sample form on crafted rows and on the five golden
scenes, the carrier search on hand-set sums, the behaviour under cutting, the figures the feature was specified with -- the golden
TFA_1 and WHB scenes, which no earlier mode of the track reads, unrotated and under six carrier offsets --, the sync on that track,
the declarations the C header makes, the exports, the memory sums and what tfrec_gpu decides before it opens a device.

Everything is exact integers: there is no tolerance anywhere.  The three FSK scenes assert only that the two forms agree: a phase
detector has nothing to say about them.  tfrec_gpu's host code gained no pure code of its own (a field and a predicate in job.h's
settings): the centre records are read, merged and printed by -G rate,auto's, which tests/test_centre_cpu.py holds under the
sanitizers.  Nothing here is measured on real recordings."""
import itertools
import os
import subprocess

import numpy as np
import pytest

import parity
import phase_rows as P
from phase_rows import B, CONT, F, I, M, OPEN
from recorder_rows import GOLDEN, RATE, golden_dec, rotated
from tfrec_amd import api, capture, envelope, sync, track


def table(*rows):
    """A run table by hand: (start, n[, flags]) of stream 0, packed in order."""
    t = np.zeros(len(rows), dtype=capture.RUN_DTYPE)
    off = 0
    for k, r in enumerate(rows):
        t[k]["start_sample"], t[k]["n_samples"], t[k]["thresh"] = r[0], r[1], P.T
        t[k]["flags"] = r[2] if len(r) > 2 else 0
        t[k]["pool_offset"] = off
        off += r[1]
    return t


def both(dec, thr, runs, L, m, K, fallback=0, state=None):
    """The vectorised form's records, words and state, held to the per-sample one's."""
    dec = np.ascontiguousarray(dec, dtype=np.int16).reshape(-1)
    a = track.phase_tracks([dec], [thr], runs, L, m, K, [fallback], state)
    b = track.phase_tracks_bruteforce([dec], [thr], runs, L, m, K, [fallback], state)
    assert a[0].dtype == track.CENTRE_DTYPE and a[1].dtype == track.TRACK_DTYPE
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and np.array_equal(a[2], b[2])
    for x, y in zip(a[3], b[3]):
        assert all(np.array_equal(x[f], y[f]) for f in x)
    assert not a[0]["reserved"].any() and not a[0]["deviation_hz"].any()
    return a


def one(z, K=1024, fallback=0, pad=50):
    """The carrier record of a burst z (int16 [n, 2]) that stands alone on a floor, its run `pad` samples longer than it."""
    row = np.zeros((len(z) + 2 * pad + 1, 2), dtype=np.int16)
    row[1:1 + len(z)] = z
    return both(row, P.T, table((1, len(z) + pad)), 5, 10, K, fallback)[0][0]


def same_subs(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert all(p.tobytes() == q.tobytes() for p, q in zip(x, y))


def compositions(n):
    return [c for k in range(1, n + 1) for c in itertools.product(range(1, n + 1), repeat=k) if sum(c) == n]


# ---- the restatement against its per-sample form
@pytest.mark.parametrize("m", [1, 10, 64])
@pytest.mark.parametrize("L", [1, 5, 16])
def test_the_two_forms_agree_on_crafted_rows(L, m):
    rows = P.hand_rows()
    for s in range(2):
        row = rows[s].reshape(-1)
        for sizes in ((2,), (1, 1)):
            a = P.submits(row, sizes, L, m, 1024, P.FALLBACK[s], thresh=P.T)
            same_subs(a, P.submits(row, sizes, L, m, 1024, P.FALLBACK[s], thresh=P.T, brute=True))
    # the runs are where phase_rows says they are
    runs = [capture.captures(rows[s].reshape(-1), 0x2F, P.T)[0] for s in range(2)]
    assert [(s, int(r["start_sample"])) for s in range(2) for r in runs[s]] == P.HAND_RUNS


@pytest.mark.parametrize("K", [64, 4096])
def test_the_two_forms_agree_at_the_heads_limits(K):
    rows = P.hand_rows()
    for s in range(2):
        row = rows[s].reshape(-1)
        a = P.submits(row, (2,), 5, 10, K, P.FALLBACK[s], thresh=P.T)
        same_subs(a, P.submits(row, (2,), 5, 10, K, P.FALLBACK[s], thresh=P.T, brute=True))
        if K == 64:  # k = 1 .. 63: 63 products at the most, never the 64 a measured carrier needs
            cen = a[0][0]
            assert (cen["source"] == F).all() and (cen["n_counted"] <= 63).all() and (cen["centre_hz"] == P.FALLBACK[s]).all()


@pytest.mark.parametrize("name", GOLDEN)
def test_the_two_forms_agree_on_the_golden_scenes(name):
    d = golden_dec(name)
    nb = len(d) // (2 * B)
    L, m = track.smooth_of(RATE[name]), min(track.LAG_MAX, track.lag_of(RATE[name]))
    for sizes in ((nb,), (1, nb - 1)):
        same_subs(P.submits(d, sizes, L, m), P.submits(d, sizes, L, m, brute=True))


def test_the_hand_made_frames_read_at_their_own_lag():
    """At m = a symbol the track is the symbol, from the second one on, at every sample but the L - 1 behind a symbol's edge."""
    rows = P.hand_rows()
    L, m = 5, P.SPB
    for s in range(2):
        cen, trk = P.chains(P.submits(rows[s].reshape(-1), (2,), L, m, 1024, P.FALLBACK[s], thresh=P.T))
        for fs, at, hz, sym in P.FRAMES:
            if fs != s:
                continue
            c, t = [(c, t) for c, t in zip(cen, trk) if int(c["start_sample"]) == at][0]
            assert c["source"] == M and abs(int(c["centre_hz"]) - hz) <= 94, (at, int(c["centre_hz"]))  # the table's step is 93.75 Hz
            got = [int(t.bits[P.SPB * i + L + 1]) for i in range(1, len(sym))]
            assert got == sym[1:], (s, at)
    # the (0, 0) pairs: every sum is exactly 0, and a zero sum gives 0
    s, a, e = P.ZERO_SUMS
    cen, trk = P.chains(P.submits(rows[s].reshape(-1), (2,), L, m, 1024, P.FALLBACK[s], thresh=P.T))
    t = [t for t in trk if int(t["start_sample"]) == 2500][0]
    assert not t.bits[a - 2500 + m + L:e - 2500].any() and t.bits[:800].any()


# ---- cuts
@pytest.mark.parametrize("name", ["tfa_1", "whb"])
def test_every_block_cut_merges_to_the_uncut_result(name):
    rate, m, L = P.GOLDEN[name][:3]
    d = golden_dec(name)
    nb = len(d) // (2 * B)
    ucen, utrk = P.chains(P.submits(d, (nb,), L, m))
    assert len(compositions(nb)) == 2 ** (nb - 1) and len(ucen) == len(P.GOLDEN[name][3])
    for sizes in compositions(nb):  # every first piece holds its head (6380 samples of the run at 10004, all of the one at 28315)
        cen, trk = P.chains(P.submits(d, sizes, L, m))
        assert [c.tobytes() for c in cen] == [c.tobytes() for c in ucen], sizes
        for a, b in zip(trk, utrk):
            assert np.array_equal(a.bits, b.bits) and a["n_ones"] == b["n_ones"] and a["last_over"] == b["last_over"], sizes


def test_a_first_piece_of_three_samples_and_nothing_ahead_of_the_chain():
    row = P.hand_rows()[0].reshape(-1)
    fb = P.FALLBACK[0]
    runs0 = capture.captures(row[:2 * B], 0x2F, P.T)[0]
    assert runs0[-1]["start_sample"] == B - 3 and runs0[-1]["n_samples"] == 3 and runs0[-1]["flags"] == OPEN
    first = both(row[:2 * B], P.T, runs0, 1, 10, 1024, fb)
    assert first[3][0]["prior"][0] == 3 and first[0][-1]["source"] == F and first[0][-1]["n_counted"] == 2
    assert not track.bits_of(first[1][-1], first[2]).any()  # c(k) < 3 < m: every product is 0
    cont = table((0, 1197 + P.W - 1, CONT))
    second = both(row[2 * B:], P.T, cont, 1, 10, 1024, fb, first[3])
    assert second[0][0]["source"] == I and second[0][0]["index"] == track.index_of(fb)
    bits = track.bits_of(second[1][0], second[2])
    assert not bits[:7].any() and bits[7:1197].any()  # c(k) = k + 3 < 10: the piece's first 7 products are 0 (L = 1: so are the bits)
    # whatever lies ahead of the chain -- the 77 carried pairs before its 3 -- does not matter
    pst = {"carry": first[3][0]["carry"].copy(), "prior": first[3][0]["prior"].copy()}
    pst["carry"][0, :track.PHASE_AHEAD - 3] = np.random.default_rng(5).integers(-30000, 30000, (track.PHASE_AHEAD - 3, 2))
    for L in (1, 16):
        a = both(row[2 * B:], P.T, cont, L, 10, 1024, fb, (first[3][0], first[3][1]))
        b = both(row[2 * B:], P.T, cont, L, 10, 1024, fb, (pst, first[3][1]))
        assert a[1].tobytes() == b[1].tobytes() and np.array_equal(a[2], b[2])
    # ... and the chain's own 3 do: the product of the piece's sample 7 reads the chain's first sample
    pst["carry"][0, -3] = (-pst["carry"][0, -3].astype(np.int64)).astype(np.int16)
    c = both(row[2 * B:], P.T, cont, 1, 10, 1024, fb, (pst, first[3][1]))
    assert track.bits_of(c[1][0], c[2])[7] != bits[7] and np.array_equal(track.bits_of(c[1][0], c[2])[10:], bits[10:])
    # prior is held at 80: a long OPEN piece carries exactly that (every block cut of the scene merges to the uncut track: above)
    part = golden_dec("whb")[:4 * B]
    runs = capture.captures(part, 0x2F, 500)[0]
    st = track.phase_tracks([part], [envelope.thresholds(part, 0x2F, 500)[0]], runs, 16, 64, 1024)[3]
    assert runs[-1]["flags"] == OPEN and runs[-1]["n_samples"] == 2 * B - 10004 and st[0]["prior"].tolist() == [track.PHASE_AHEAD]


# ---- the carrier search
def test_the_carrier_search_on_hand_set_sums():
    assert track.carrier_index(5, 0) == track.carrier_index(1 << 42, 0) == 0  # cross(0) = 0 and score(0) > 0; r = 2048 has score < 0
    assert track.carrier_index(-5, 0) == 2048 and track.carrier_index(0, 7) == 1024 and track.carrier_index(0, -7) == 3072
    assert [track.carrier_hz(r) for r in (0, 1, 2047, 2048, 4095, 1024)] == [0, 93, 191906, -192000, -94, 96000]
    still = np.tile(np.array([[3000, 0]], dtype=np.int16), (100, 1))
    c = one(still, fallback=5000)  # 99 products (9e6, 0)
    assert (int(c["n_counted"]), int(c["source"]), int(c["centre_hz"]), int(c["index"])) == (99, M, 0, 0)
    # quarter turns: an even count of products sums to (0, 0) and falls back; one more is (0, 9e6): a quarter of the rate
    c = one(P.quarter_turns(201), fallback=5000)
    assert (int(c["n_counted"]), int(c["source"]), int(c["centre_hz"]), int(c["index"])) == (200, F, 5000, track.index_of(5000))
    c = one(P.quarter_turns(202), fallback=5000)
    assert (int(c["n_counted"]), int(c["source"]), int(c["centre_hz"]), int(c["index"])) == (201, M, 96000, 1024)
    # 63 products fall back, 64 are measured
    c = one(still[:64], fallback=-7000)
    assert (int(c["n_counted"]), int(c["source"]), int(c["centre_hz"]), int(c["index"])) == (63, F, -7000, 4021)
    assert (int(one(still[:65])["n_counted"]), int(one(still[:65])["source"])) == (64, M)
    assert int(one(still, K=64)["source"]) == F and int(one(still, K=64)["n_counted"]) == 63
    # the fallback's index at both ends of the range
    for hz in (192000, -192000, 191999, -191999):
        c = one(still[:10], fallback=hz)
        assert (int(c["source"]), int(c["centre_hz"]), int(c["index"])) == (F, hz, track.index_of(hz))
    assert track.index_of(192000) == track.index_of(-192000) == 2048


def test_the_carrier_search_against_all_4096_candidates():
    rng = np.random.default_rng(11)
    top = (1 << 43) - 1
    pairs = [(1, 0), (0, 1), (-1, 0), (0, -1), (1, 1), (-1, 1), (1, -1), (-1, -1), (top, top), (-top, top), (top, -top), (-top, -top),
             (top, 1), (1, -top), (3, -2), (32767, 1), (-32767, -1)]
    for bits in (4, 16, 31, 43):  # small sums, where the table's rounding decides, and the largest
        pairs += [(int(a), int(b)) for a, b in rng.integers(-(1 << bits) + 1, 1 << bits, (12, 2)) if a or b]
    for A, Bs in pairs:
        assert track.carrier_index(A, Bs) == track.carrier_index_bruteforce(A, Bs), (A, Bs)
    # a carrier at a table direction is found: a tone that turns by r / 4096 of a turn per sample
    for r in (37, 1000, 2048, 4031):
        k = np.arange(300)
        z = 6000 * np.exp(2j * np.pi * r * k / 4096)
        c = one(np.stack([np.rint(z.real), np.rint(z.imag)], axis=1).astype(np.int16))
        assert (int(c["source"]), int(c["index"])) == (M, r)


# ---- the figures the feature was specified with
def read(name, hz):
    rate, m, L = P.GOLDEN[name][:3]
    d = rotated(golden_dec(name), hz) if hz else golden_dec(name)
    subs = P.submits(d, (len(d) // (2 * B),), L, m)
    return subs, P.chains(subs)


@pytest.mark.parametrize("hz", (0,) + P.ROTATIONS)
def test_the_golden_tfa_1_scene_reads(hz):
    rate, m, L, runs, idx, n_bits = P.GOLDEN["tfa_1"]
    subs, (cen, trk) = read("tfa_1", hz)
    assert len(cen) == 2 and all(c["source"] == M for c in cen)
    if hz == 0:
        assert [P.figures(c) for c in cen] == [(a, n, p, r) for a, n, _, p, r in runs]
    else:
        assert tuple(int(c["index"]) for c in cen) == idx[P.ROTATIONS.index(hz)]
    assert [(int(t["start_sample"]), int(t["n_samples"]), int(t["last_over"])) for t in trk] == [r[:3] for r in runs]
    for t, tel in zip(trk, P.TFA_1_TELEGRAMS):
        bits = P.sliced(t, rate)
        assert len(bits) == n_bits
        assert bits[P.FROM_BIT:P.FROM_BIT + 88] == P.lsb_first(tel)  # the whole telegram, 11 bytes, in positive polarity


def test_the_sync_finds_the_golden_tfa_1_frames_on_the_phase_track():
    subs, (cen, trk) = read("tfa_1", 0)
    st = sync.Settings(38400, P.WORD, 16, 0)
    srecs, swords, _ = sync.syncs(subs[0][1], subs[0][2], st, None, 1)
    sch = sync.chains([(srecs, swords)])
    assert [tuple(sync.plateaus(s.bits)) for s in sch] == [(p,) for p in P.TFA_1_PLATEAUS]
    for t, s, pay in zip(trk, sch, P.TFA_1_PAYLOADS):
        fr = sync.frames(t, s, st, 4)
        assert len(fr) == 1 and fr[0][1:3] == (0, "+") and track.hex_of(fr[0][3]) == pay


@pytest.mark.parametrize("hz", (0,) + P.ROTATIONS)
def test_the_golden_whb_scene_reads_behind_the_descrambler(hz):
    rate, m, L, runs, idx, n_bits = P.GOLDEN["whb"]
    subs, (cen, trk) = read("whb", hz)
    assert len(cen) == 1 and cen[0]["source"] == M
    if hz == 0:
        assert [P.figures(c) for c in cen] == [(a, n, p, r) for a, n, _, p, r in runs]
    else:
        assert (int(cen[0]["index"]),) == idx[P.ROTATIONS.index(hz)]
    assert [(int(t["start_sample"]), int(t["n_samples"]), int(t["last_over"])) for t in trk] == [r[:3] for r in runs]
    bits = P.descrambled(P.sliced(trk[0], rate))
    assert len(bits) == n_bits
    want = P.lsb_first(P.whb_event_bytes())
    assert len(bits) - P.FROM_BIT == 232 and bits[P.FROM_BIT:] == want[:232]  # every bit the synthetic burst holds


def test_the_golden_scenes_do_not_read_on_the_frequency_track():
    """What 6t, 6u and 6w say of them, kept as the contrast: about a fixed centre neither telegram is in the slice."""
    import recorder_rows as RR
    d = golden_dec("tfa_1")
    for t, tel in zip(track.chains(RR.submits(d, (len(d) // (2 * B),), 5)), P.TFA_1_TELEGRAMS):
        s = RR.bit_string(P.sliced(t, 38400))
        assert RR.bit_string(P.lsb_first(tel)) not in s


# ---- the declarations, the exports, the memory sums, the command line
def test_the_header_the_exports_and_the_memory_sums(tmp_path):
    src = tmp_path / "phase.c"
    src.write_text('#include <stddef.h>\n#include "tfrec_amd.h"\n'
                   "_Static_assert(sizeof(tfrec_amd_track) == 40 && sizeof(tfrec_amd_track_centre) == 48, \"the records are the other modes'\");\n"
                   "_Static_assert(offsetof(tfrec_amd_track_centre, n_counted) == 24 && offsetof(tfrec_amd_track_centre, index) == 40, \"fields\");\n"
                   "int (*enable)(tfrec_amd_ctx *, int32_t, int32_t, int32_t) = tfrec_amd_enable_burst_track_phase;\n")
    subprocess.check_call(["cc", "-std=c11", "-fsyntax-only", "-I", os.path.join(parity.ROOT, "include"), str(src)])
    L = api.load_library()
    assert "tfrec_amd_enable_burst_track_phase" in api.EXPORTS
    # no GPU is needed to be refused
    assert L.tfrec_amd_enable_burst_track_phase(None, 5, 1024, 10) == api.E_INVAL
    assert hasattr(api.Receiver, "enable_burst_track_phase")
    # the auto-centre track's sums with 80 carried pairs per stream for its 16; the other modes' sums stay what they were
    assert track.device_bytes(3, 10, 65) == api.FIFO_DEPTH * (400 + 12 + 12) + 3 * 68
    assert track.auto_device_bytes(3, 10, 65) == track.device_bytes(3, 10, 65) + api.FIFO_DEPTH * 480 + 24
    assert track.phase_device_bytes(3, 10, 65) == track.auto_device_bytes(3, 10, 65) + 3 * 4 * 64
    assert track.phase_device_bytes(3, 10, 65) == api.FIFO_DEPTH * (880 + 12 + 12) + 3 * (320 + 4 + 8)
    assert track.PHASE_AHEAD == track.LAG_MAX + track.AHEAD == 80 and (track.LAG_MIN, track.LAG_MAX) == (1, 64)
    assert [track.lag_of(r) for r in (38400, 6000, 5954, 5953, 96000, 1000)] == [10, 64, 64, 65, 4, 384]
    head = open(os.path.join(parity.ROOT, "include", "tfrec_amd.h")).read()
    assert "int tfrec_amd_enable_burst_track_phase(tfrec_amd_ctx *ctx" in head
    text = head[head.index("Phase track"):head.index("tfrec_amd_enable_burst_track_phase(tfrec_amd_ctx")]
    for words in ("80 = 64 + 16", "score(r) > 0", "first piece", "real recordings", "tfrec_amd_save_streams"):
        assert words in text, words


def test_cli_psk_usage_errors_and_accepted_forms(tmp_path):
    parity.build_cli()
    f = str(tmp_path / "missing.iq")
    for args in (["-G", "38400,psk", "-O", "2000", "-L", f], ["-O", "2000", "-G", "38400,psk,10", "-L", f]):
        out = parity.run_cli(args)
        assert out.returncode == 1 and "not with -O" in out.stderr, args
    for bad in ("38400,psk,0", "38400,psk,65", "38400,psk,-1", "38400,psk,", "38400,psk,x", "38400,psk,10,1", "38400,pskx", "38400,PSK",
                "38400,ps", "psk", ",psk", "999,psk,10", "96001,psk", "38400,psk "):
        out = parity.run_cli(["-G", bad, "-L", f])
        assert out.returncode == 1 and "bad -G" in out.stderr, bad
    for rate in ("5953", "1000"):  # a symbol is more than 64 samples: no default lag
        out = parity.run_cli(["-G", rate + ",psk", "-L", f])
        assert out.returncode == 1 and "bad -G" in out.stderr and "more than the lag's 64" in out.stderr, rate
    # refused wherever -G is, with -G's own messages
    for args in (["-G", "38400,psk", "-X", f], ["-G", "38400,psk", "-s", "50", "-L", f], ["-G", "38400,psk", "-A", "-L", f]):
        out = parity.run_cli(args)
        assert out.returncode == 1 and "-G reads" in out.stderr, args
    for k in ("-k", "-K"):
        out = parity.run_cli(["-G", "38400,psk", k, str(tmp_path / "keep"), "-L", f])
        assert out.returncode == 2 and "not with -G" in out.stderr, k
    out = parity.run_cli(["-h"])
    assert "-G r,psk[,m]" in out.stderr and "[-G rate,psk[,lag]]" in out.stderr
    assert "-G r,auto" in out.stderr and "[-G rate,auto]" in out.stderr and "-G r[,c]" in out.stderr and "[-O level]" in out.stderr  # the others' stay
    for args in (["-G", "38400,psk", "-L", f], ["-G", "5954,psk", "-L", f], ["-G", "1000,psk,64", "-L", f], ["-G", "96000,psk,1", "-L", f],
                 ["-G", "38400,psk", "-Y", "b42b,0,4", "-L", f], ["-G", "6000,psk,64", "-M", "-Q", "-C", "-L", f],
                 ["-G", "38400,psk", "-S", str(tmp_path / "cap"), "-n", "1", "-L", f], ["-G", "38400,psk", "-d", "0", "-L", f]):
        out = parity.run_cli(args)  # accepted: the file is looked for
        assert out.returncode == 2 and "missing.iq" in out.stderr, args
    out = parity.run_cli(["-G", "38400,psk", "-R", str(tmp_path / "nothing")])  # accepted with -R: the capture is looked for
    assert out.returncode == 2 and "-R replays" not in out.stderr and "bad -G" not in out.stderr
