"""The burst track's amplitude mode without a GPU (tfrec_amd_enable_burst_track_amplitude, tfrec_amd_set_burst_track_level,
tfrec_gpu -O): the restatement tfrec_amd/track.py (amplitude_tracks) against its per-sample form on crafted rows and
hand-set sums, a synthetic NRZ on-off keyed frame through the slicer, the sync and the framing as they are, its behaviour under
cutting, a pulse-width burst through pulses, tfrec_gpu's pulses (tfrec_amd/host/job.h, compiled into a stand-alone program under the
address and undefined-behaviour sanitizers), the exports, the memory sums and what tfrec_gpu decides before it opens a device.

Everything is exact integers: there is no tolerance anywhere.  The bursts are made here from a fixed integer generator; nothing
here is measured on real recordings."""
import os
import subprocess

import numpy as np
import pytest

import amplitude_rows as A
import parity
from amplitude_rows import B, CONT, OPEN
from recorder_rows import stripped
from tfrec_amd import api, capture, sync, track


def table(*rows):
    """A run table by hand: (start, n[, flags]) of stream 0, packed in order."""
    t = np.zeros(len(rows), dtype=capture.RUN_DTYPE)
    off = 0
    for k, r in enumerate(rows):
        t[k]["start_sample"], t[k]["n_samples"], t[k]["thresh"] = r[0], r[1], A.T
        t[k]["flags"] = r[2] if len(r) > 2 else 0
        t[k]["pool_offset"] = off
        off += r[1]
    return t


def same(a, b):
    (ra, wa, sa), (rb, wb, sb) = a, b
    assert ra.dtype == rb.dtype == track.TRACK_DTYPE and ra.tobytes() == rb.tobytes()
    assert wa.dtype == wb.dtype == np.dtype("<u4") and wa.tobytes() == wb.tobytes()
    assert np.array_equal(sa["carry"], sb["carry"]) and np.array_equal(sa["prior"], sb["prior"])


def both(dec, thr, runs, L, level, state=None, **kw):
    """The vectorised form's result, held to the per-sample one."""
    dec = np.ascontiguousarray(dec, dtype=np.int16).reshape(-1)
    a = track.amplitude_tracks([dec], [thr], runs, L, [level], state, **kw)
    same(a, track.amplitude_tracks_bruteforce([dec], [thr], runs, L, [level], state, **kw))
    return a


def bits(res, e=0):
    return track.bits_of(res[0][e], res[1]).tolist()


# ---- the restatement against its per-sample form
@pytest.mark.parametrize("L", [1, 5, 16])
def test_the_two_forms_agree_on_crafted_rows(L):
    row = A.hand_rows()[0].reshape(-1)
    runs = capture.captures(row, 0x2F, A.T)[0]
    assert len(runs) == 4
    for level in (0, 1, 1500, 65535):
        a = both(row, A.T, runs, L, level)
        assert a[0]["n_ones"].any() == (level < 65535)
    # a table by hand on the same samples: neighbours that share a word, a run at sample 0, one to the last sample; and a state to
    # continue from, with 3 and with 16 samples of the chain ahead
    t = table((0, 37, CONT), (40, 1), (41, 70), (5000, 2 * B - 5000, OPEN))
    for prior in (3, 16):
        st = track.fresh_state(1)
        st["carry"][0] = np.arange(32).reshape(16, 2) * 700 - 9000
        st["prior"][0] = prior
        a = both(row, A.T, t, L, 1500, st)
        assert a[2]["prior"][0] == 16 and a[0]["bit_offset"].tolist() == [0, 37, 38, 108]
    # prior decides how many of the carried pairs count: |I| + |Q| of the carried pair k is |700 (2 k) - 9000| + |700 (2 k + 1) - 9000|
    p = [abs(1400 * k - 9000) + abs(1400 * k - 8300) for k in range(16)]
    first = int(np.abs(row[0:2].astype(np.int64)).sum())
    for prior in (0, 3, 16):
        st = track.fresh_state(1)
        st["carry"][0] = np.arange(32).reshape(16, 2) * 700 - 9000
        st["prior"][0] = prior
        want = first + sum(p[16 - i] for i in range(1, min(L, prior + 1)))
        assert bits(both(row, A.T, table((0, 37, CONT)), L, (want - 1) // L, st))[0] == int(want > L * ((want - 1) // L))
        assert bits(both(row, A.T, table((0, 37, CONT)), L, -(-want // L), st))[0] == 0  # L * level >= the sum


@pytest.mark.parametrize("L", [1, 5, 16])
def test_the_hand_set_sums(L):
    n = 64
    # a sum exactly L * level is 0, L * level + 1 is 1
    z = np.zeros((n, 2), dtype=np.int16)
    z[:] = (-700, 300)  # p = 1000
    z[40] = (-700, 301)
    a = both(z, 0, table((0, n)), L, 1000)
    assert bits(a) == [int(40 <= k < 40 + L) for k in range(n)] and a[0]["n_ones"][0] == L
    # the pair (-32768, -32768): p = 65536, above the largest level
    z[:] = (-32768, -32768)
    assert bits(both(z, 0, table((0, n)), L, 65535)) == [int(k >= L - 1) for k in range(n)]
    z[:] = (-32768, 32767)  # p = 65535: not above it
    assert not any(bits(both(z, 0, table((0, n)), L, 65535)))
    # all-zero samples at level 0: the sum is not greater than 0
    z[:] = 0
    a = both(z, 0, table((0, n)), L, 0)
    assert not any(bits(a)) and a[0]["last_over"][0] == -1
    z[9] = (0, -1)
    assert bits(both(z, 0, table((0, n)), L, 0)) == [int(9 <= k < 9 + L) for k in range(n)]
    # a chain's first L - 1 samples: the samples ahead of it count as 0, whatever they hold
    z[:] = (300, -200)  # p = 500
    z[:20] = (30000, 30000)
    a = both(z, 0, table((20, 30)), L, 400)  # a full sum: 500 L > 400 L; k + 1 samples: 500 (k + 1) > 400 L
    assert bits(a) == [int(500 * min(k + 1, L) > 400 * L) for k in range(30)]
    if L == 5:
        assert bits(a)[:5] == [0, 0, 0, 0, 1]
    # ... and in a CONTINUES piece the carried pairs count as far as prior reaches
    st = track.fresh_state(1)
    st["carry"][0][:] = (300, -200)
    st["prior"][0] = 2
    t = table((0, 30, CONT))
    assert bits(both(z[20:], 0, t, L, 400, st)) == [int(500 * min(k + 3, L) > 400 * L) for k in range(30)]


def test_the_levels_are_checked_and_default_to_zero():
    z = np.zeros((8, 2), dtype=np.int16)
    z[:] = (1, 0)
    assert all(bits(track.amplitude_tracks([z.reshape(-1)], [0], table((0, 8)), 1)))  # no levels given: 0, and 1 > 0
    for bad in (-1, 65536):
        with pytest.raises(AssertionError):
            track.amplitude_tracks([z.reshape(-1)], [0], table((0, 8)), 1, [bad])


# ---- a synthetic NRZ on-off keyed burst
def nrz_chain(sizes=(2,), **kw):
    subs = A.submits(A.nrz_row(), sizes, A.L_NRZ, A.ON // 2, **kw)
    ch = track.chains(subs)
    assert len(ch) == 1
    return subs, ch[0]


def test_the_nrz_frame_is_sliced_and_framed():
    subs, c = nrz_chain()
    assert A.L_NRZ == 16 and (int(c["start_sample"]), int(c["last_over"]) + 1) == (B - 2500, 64 * A.SPB)
    symbols = track.slice_bits(c.bits[:int(c["last_over"]) + 1], A.RATE)
    assert track.hex_of(symbols) == A.FRAME and A.FRAME in track.line("f", c, A.RATE)
    # the two forms on it
    slow = A.submits(A.nrz_row(), (2,), A.L_NRZ, A.ON // 2, brute=True)
    assert slow[0][0].tobytes() == subs[0][0].tobytes() and slow[0][1].tobytes() == subs[0][1].tobytes()
    # the sync and the framing, as they are, on that track: one plateau and the four bytes
    st = sync.Settings(A.RATE, A.WORD, 16, 0)
    srecs, swords, _ = sync.syncs(subs[0][0], subs[0][1], st)
    s = sync.chains([(srecs, swords)])
    assert len(s) == 1 and len(sync.plateaus(s[0].bits)) == 1
    fr = sync.frames(c, s[0], st, 4)
    assert len(fr) == 1 and fr[0][1:3] == (0, "+") and track.hex_of(fr[0][3]) == A.PAYLOAD
    # the level decides: at the on-amplitude and above nothing is read, at 0 the floor's noise is
    assert not track.chains(A.submits(A.nrz_row(), (2,), A.L_NRZ, A.ON + 40))[0].bits.any()
    assert track.chains(A.submits(A.nrz_row(), (2,), A.L_NRZ, 0))[0].bits[16:].all()


def test_the_nrz_burst_merges_to_the_uncut_result_for_every_cut():
    z = A.nrz_row(4, 2 * B - 2500).reshape(-1)
    whole = track.chains(A.submits(z, (4,), A.L_NRZ, A.ON // 2))
    assert len(whole) == 1
    cuts = 0
    for sizes in [(1,) * 4] + [(k, 4 - k) for k in range(1, 4)]:
        subs = A.submits(z, sizes, A.L_NRZ, A.ON // 2)
        cuts += sum(1 for recs, _ in subs for r in recs if r["flags"] & CONT)
        got = track.chains(subs)
        assert len(got) == 1 and stripped(got[0].rec) == stripped(whole[0].rec) and np.array_equal(got[0].bits, whole[0].bits), sizes
        assert track.pulses_line("f", got[0]) == track.pulses_line("f", whole[0])
    assert cuts == 2  # the burst lies across the middle boundary
    # three pieces of 1000, 500 and the rest of the run's samples, each a submit of its own with a table by hand
    r = whole[0].rec
    a, n = int(r["start_sample"]), int(r["n_samples"])
    zz = z.reshape(-1, 2)
    got, st, pos = [], None, 0
    for k, m in enumerate((1000, 500, n - 1500)):
        lo = 0 if k == 0 else a + pos  # the first submit holds what lies ahead of the run too
        t = table((a + pos - lo, m, (CONT if k else 0) | (OPEN if k < 2 else 0)))
        t["start_sample"] = a + pos
        recs, words, st = both(zz[lo:a + pos + m], A.T, t, A.L_NRZ, A.ON // 2, st, base=[lo])
        assert st["prior"][0] == (16 if k < 2 else 0)
        got.append((recs, words))
        pos += m
    m3 = track.chains(got)
    assert len(m3) == 1 and stripped(m3[0].rec) == stripped(r) and np.array_equal(m3[0].bits, whole[0].bits)


def test_a_level_changed_between_two_submits_slices_each_piece_with_its_own():
    z = A.nrz_row().reshape(-1)
    one = track.chains(A.submits(z, (1, 1), A.L_NRZ, A.ON // 2))[0]
    two = track.chains(A.submits(z, (1, 1), A.L_NRZ, None, levels=[A.ON // 2, A.ON + 40]))[0]
    assert stripped(two.rec)[:5] == stripped(one.rec)[:5]  # not a restart: the chain is one
    assert np.array_equal(two.bits[:2500], one.bits[:2500]) and one.bits[2500:].any() and not two.bits[2500:].any()


# ---- the generated rows of the GPU test's random set: the two forms, and the cut against the uncut rows
@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_generated_rows_and_cuts(seed):
    rows, lv, L, sizes = A.generated(seed)
    assert sizes != (3,) or seed == 4
    for s in range(len(rows)):
        whole = A.submits(rows[s], (3,), L, lv[s])
        slow = A.submits(rows[s], (3,), L, lv[s], brute=True)
        assert whole[0][0].tobytes() == slow[0][0].tobytes() and whole[0][1].tobytes() == slow[0][1].tobytes() and len(whole[0][0]) >= 1
        a, b = track.chains(A.submits(rows[s], sizes, L, lv[s])), track.chains(whole)
        assert len(a) == len(b)
        for x, y in zip(a, b):
            assert stripped(x.rec) == stripped(y.rec) and np.array_equal(x.bits, y.bits), (s, int(x["start_sample"]))


# ---- a pulse-width burst
PW_BITS = [1, 0, 0, 1, 1, 0, 1, 0, 1, 1, 1, 0, 0, 1]


def pw_chain(bits_in, brute=False):
    nb = -(-(500 + sum(A.pw_widths(bits_in)) + A.W) // B)
    ch = track.chains(A.submits(A.pw_row(bits_in, nb), (nb,), 16, A.ON // 2, brute=brute))
    assert len(ch) == 1
    return ch[0]


def test_the_pulse_widths_decode_to_the_bits_put_in():
    c = pw_chain(PW_BITS)
    w = track.pulses(c.bits[:int(c["last_over"]) + 1])
    assert len(w) == 2 * len(PW_BITS) - 1
    assert [int(x > A.PW_EDGE) for x in w[0::2]] == PW_BITS and [int(x > A.PW_EDGE) for x in w[1::2]] == PW_BITS[:-1]
    slow = pw_chain(PW_BITS, brute=True)
    assert track.pulses(slow.bits[:int(slow["last_over"]) + 1]) == w  # the exact widths, of both forms
    # what the smoothing does to them: 16 * level is 8 on-samples' worth, so an edge is seen with the 8th or the 9th of them, as the
    # noise decides: a pulse keeps its width but for a sample; the last pulse ends with the burst's last over sample, 7 or 8 short
    assert all(abs(x - y) <= 1 for x, y in zip(w[:-1], A.pw_widths(PW_BITS)[:-1])) and A.PW_LONG - w[-1] in (7, 8) and PW_BITS[-1] == 1
    assert track.pulses_line("f.iq", c) == "pulses f.iq %d %d %d %d %s" % (
        int(c["start_sample"]), int(c["n_samples"]), int(c["last_over"]) + 1, len(PW_BITS), ",".join("%d" % x for x in w))


def test_pulses_and_its_line():
    assert track.pulses([]) == [] and track.pulses([0, 0, 0]) == [] and track.pulses([1]) == [1]
    assert track.pulses([0, 1, 1, 0, 0, 0, 1, 0]) == [2, 3, 1] and track.pulses([1, 1, 0, 1]) == [2, 1, 1]
    rec = np.zeros((), dtype=track.TRACK_DTYPE)
    rec["start_sample"], rec["n_samples"], rec["last_over"] = 77, 40, 29
    none = track.Piece(rec.copy(), np.zeros(40, dtype=np.uint8))
    assert track.pulses_line("a", none) == "pulses a 77 40 30 0 -"  # a burst of zero pulses
    b = np.zeros(40, dtype=np.uint8)
    b[[3, 4, 9, 30]] = 1  # (the one at 30 lies behind last_over)
    assert track.pulses_line("a", track.Piece(rec.copy(), b)) == "pulses a 77 40 30 2 2,4,1"
    rec["last_over"] = -1
    assert track.pulses_line("a", track.Piece(rec.copy(), b)) == "pulses a 77 40 0 0 -"
    # the 64-pulse cap and its +
    for n, mark in ((64, ""), (65, "+"), (200, "+")):
        b = np.tile(np.array([1, 1, 0], dtype=np.uint8), n)
        rec["n_samples"], rec["last_over"] = len(b), len(b) - 1
        ln = track.pulses_line("a", track.Piece(rec.copy(), b)).split()
        assert ln[5] == "64" + mark and ln[6] == ",".join(["2", "1"] * 63 + ["2"])


# ---- tfrec_gpu's pulses: job.h in a stand-alone program
@pytest.fixture(scope="module")
def pulses_driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pulses") / "pulses_driver")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(parity.ROOT, "tests", "pulses_driver.cpp")])
    return exe


def test_the_host_prints_the_restatements_pulses(pulses_driver):
    pieces = [("nrz.iq", nrz_chain()[1]), ("pw.iq", pw_chain(PW_BITS))]
    rec = np.zeros((), dtype=track.TRACK_DTYPE)

    def hand(b, last, start=5):
        r = rec.copy()
        r["start_sample"], r["n_samples"], r["last_over"] = start, len(b), last
        return track.Piece(r, np.asarray(b, dtype=np.uint8))

    rng = A.lcg(99)
    noise = [next(rng) & 1 for _ in range(3000)]
    pieces += [("h.iq", hand([0] * 40, 29)), ("h.iq", hand([1] * 40, 39)), ("h.iq", hand([1] * 40, -1)), ("h.iq", hand([0, 1, 1, 0, 1, 0], 5)),
               ("h.iq", hand([0, 1, 1, 0, 1, 0], 3)), ("h.iq", hand([1, 1, 0] * 64, 191)), ("h.iq", hand([1, 1, 0] * 65, 194)),
               ("h.iq", hand(noise, 2998)), ("h.iq", hand([0, 1] * 17, 33)), ("h.iq", hand([1] + [0] * 31 + [1], 32))]
    lines, want = [], []
    for f, p in pieces:
        n = int(p["n_samples"])
        lines.append("track %s %d %d %d %s" % (f, int(p["start_sample"]), n, int(p["last_over"]), "".join("01"[b] for b in p.bits) or "-"))
        w = track.pulses(p.bits[:int(p["last_over"]) + 1])
        want += [track.pulses_line(f, p), " ".join(["widths", str(len(w))] + ["%d" % x for x in w])]
    out = subprocess.run([pulses_driver], input="".join(ln + "\n" for ln in lines), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.splitlines() == want
    assert any("+" in ln.split()[5] for ln in want[0::2]) and any(ln.endswith(" -") for ln in want[0::2])


# ---- the exports, the memory sums, the command line
def test_the_exports_and_the_memory_sums():
    names = ("tfrec_amd_enable_burst_track_amplitude", "tfrec_amd_set_burst_track_level")
    L = api.load_library()
    for sym in names:
        assert sym in api.EXPORTS
        getattr(L, sym)
    # no GPU is needed to be refused
    assert L.tfrec_amd_enable_burst_track_amplitude(None, 5) == api.E_INVAL
    assert L.tfrec_amd_set_burst_track_level(None, None, None, 0) == api.E_INVAL
    one = np.zeros(1, dtype=np.int32)
    assert L.tfrec_amd_set_burst_track_level(None, one.ctypes.data, one.ctypes.data, 1) == api.E_INVAL
    assert hasattr(api.Receiver, "enable_burst_track_amplitude") and hasattr(api.Receiver, "set_burst_track_level")
    # the memory sums are the frequency mode's: the staged int32 per stream carries the level instead of the centre's index
    assert track.device_bytes(3, 10, 65) == api.FIFO_DEPTH * (400 + 12 + 12) + 3 * 68 and track.pinned_bytes(3) == api.FIFO_DEPTH * 12
    src = open(os.path.join(parity.ROOT, "include", "tfrec_amd.h")).read()
    for sym in names:
        assert "int %s(tfrec_amd_ctx *ctx" % sym in src


def test_cli_amplitude_usage_errors(tmp_path):
    parity.build_cli()
    f = str(tmp_path / "missing.iq")
    for args in (["-O", "2000", "-L", f], ["-G", "4800", "-O", "65536", "-L", f], ["-G", "4800", "-O", "x", "-L", f],
                 ["-G", "4800", "-O", "-1", "-L", f], ["-G", "4800", "-O", "", "-L", f], ["-G", "2500,100", "-O", "5", "-L", f],
                 ["-O", "5", "-G", "2500,0", "-L", f], ["-O", "5", "-Y", "2dd4", "-L", f]):
        out = parity.run_cli(args)
        assert out.returncode == 1 and "bad -O" in out.stderr, args
    # refused wherever -G is, with -G's own messages
    for args in (["-G", "4800", "-O", "5", "-X", f], ["-G", "4800", "-O", "5", "-s", "50", "-L", f], ["-G", "4800", "-O", "5", "-A", "-L", f]):
        out = parity.run_cli(args)
        assert out.returncode == 1 and "-G reads" in out.stderr, args
    for k in ("-k", "-K"):
        out = parity.run_cli(["-G", "4800", "-O", "5", k, str(tmp_path / "keep"), "-L", f])
        assert out.returncode == 2 and "not with -G" in out.stderr, k
    out = parity.run_cli(["-h"])
    assert "-O level" in out.stderr and "[-O level]" in out.stderr and "pulses <file>" in out.stderr
    assert "-G r[,c]" in out.stderr and "[-G rate[,centre_hz]]" in out.stderr  # -G's own lines stay
    for args in (["-G", "4800", "-O", "2000", "-L", f], ["-O", "0", "-G", "96000", "-L", f], ["-G", "1000", "-O", "65535", "-L", f],
                 ["-G", "4800", "-O", "2000", "-Y", "2dd4,0,4", "-L", f], ["-G", "4800", "-O", "2000", "-M", "-Q", "-C", "-L", f],
                 ["-G", "4800", "-O", "2000", "-S", str(tmp_path / "cap"), "-n", "1", "-L", f], ["-G", "4800", "-O", "2000", "-d", "0", "-L", f]):
        out = parity.run_cli(args)  # accepted: the file is looked for
        assert out.returncode == 2 and "missing.iq" in out.stderr, args
    out = parity.run_cli(["-G", "4800", "-O", "2000", "-R", str(tmp_path / "nothing")])  # accepted with -R: the capture is looked for
    assert out.returncode == 2 and "-R replays" not in out.stderr and "bad -O" not in out.stderr
