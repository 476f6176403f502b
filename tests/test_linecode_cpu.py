"""The line code without a GPU (tfrec_amd_enable_burst_code, tfrec_gpu -G -U): the restatement tfrec_amd/linecode.py
against its per-sample form on crafted tracks and the five golden scenes, tracks whose decoded form is known by construction (a
single one, NRZI, G3RUH), INVERT, delta at its limits, the behaviour under cutting -- every block cut of the golden WHB and TFA_1
scenes, pieces of 1000, 500 and the rest, a first piece of 3 samples behind a stale history --, the figures the feature was
specified with (the golden WHB scene behind the descrambler, unrotated and under six carrier offsets, and the contrast on the raw
track), TFA_1's frames LSB-first, the byte order of sync.frames and sync.line, tfrec_gpu's host code (tfrec_amd/host/job.h,
compiled into a stand-alone program under the address and undefined-behaviour sanitizers), the declarations the C header makes,
the exports, the memory sums and what tfrec_gpu decides before it opens a device.

Everything is exact integers: there is no tolerance anywhere.  Nothing here is measured on real recordings."""
import ctypes as C
import functools
import itertools
import os
import subprocess

import numpy as np
import pytest

import linecode_rows as LR
import parity
import phase_rows as P
from linecode_rows import CONT, OPEN, code_submits, hand_track, held, pieces_of, scrambled, sync_submits
from recorder_rows import GOLDEN, RATE, golden_dec, rotated, stripped, submits
from tfrec_amd import api, linecode, sync, track

B = api.BLOCK_DEC


def both(trecs, twords, st, state=None, n_streams=1, max_samples=None):
    """The vectorised form's records, words and state, held to the per-sample one's."""
    a = linecode.codes(trecs, twords, st, state, n_streams, max_samples)
    b = linecode.codes_bruteforce(trecs, twords, st, state, n_streams, max_samples)
    assert a[0].dtype == b[0].dtype == track.TRACK_DTYPE and a[0].tobytes() == b[0].tobytes()
    assert a[1].dtype == b[1].dtype == np.dtype("<u4") and a[1].tobytes() == b[1].tobytes()
    assert len(a[2]["bits"]) == len(b[2]["bits"]) and all(np.array_equal(x, y) for x, y in zip(a[2]["bits"], b[2]["bits"]))
    for f in track.TRACK_DTYPE.names:  # the record is the track's, but for n_ones
        if f != "n_ones":
            assert np.array_equal(a[0][f], np.asarray(trecs)[f]), f
    return a


def both_submits(tsubs, st, n_streams=1):
    state, out = None, []
    for recs, words in tsubs:
        r, w, state = both(recs, words, st, state, n_streams)
        out.append((r, w))
    return out


def coded(bits, st, **kw):
    """The coded track of one run that stands alone."""
    r, w, _ = both(*hand_track(bits, **kw), st)
    return track.bits_of(r[0], w), r[0]


# ---- the restatement against its per-sample form
@pytest.mark.parametrize("name", list(LR.SETS))
def test_the_two_forms_agree_on_crafted_tracks(name):
    st = LR.settings(name)
    rng = np.random.default_rng(3)
    t = rng.integers(0, 2, 5000).astype(np.uint8)
    for sizes in ((), (1000, 500), (1, 1, 1), (2047, 1), (2500,)):
        both_submits(pieces_of(t, sizes), st)
    # several runs in one submit, two streams, packed back to back off word boundaries; a pool that does not hold the last run
    recs, off = [], 0
    for s, n, flags in ((0, 37, 0), (0, 730, 0), (0, 3, OPEN), (1, 100, 0), (1, 2100, OPEN)):
        recs.append(hand_track(np.zeros(n), flags, offset=off, stream=s, start=1000 * len(recs))[0])
        off += n
    recs = np.concatenate(recs)
    bits = rng.integers(0, 2, (off + 31) // 32 * 32).astype(np.uint8)
    words = np.packbits(bits.reshape(-1, 32), axis=1, bitorder="little").view("<u4").reshape(-1)
    a = both(recs, words, st, None, 2)
    assert [len(h) for h in a[2]["bits"]] == [3, 2047]
    cut = both(recs, words, st, None, 2, max_samples=off - 1)  # the last run does not fit: no bits, n_ones 0, no history
    assert cut[0][-1]["n_ones"] == 0 and cut[0][:-1].tobytes() == a[0][:-1].tobytes() and [len(h) for h in cut[2]["bits"]] == [3, 0]
    assert len(cut[1]) == (int(recs[-1]["bit_offset"]) + 31) // 32


@pytest.mark.parametrize("name", GOLDEN)
def test_the_two_forms_agree_on_the_golden_scenes(name):
    d = golden_dec(name)
    nb = len(d) // (2 * B)
    for st in (linecode.g3ruh(RATE[name]), linecode.nrzs(RATE[name])):
        for sizes in ((nb,), (1, nb - 1)):
            both_submits(submits(d, sizes, track.smooth_of(RATE[name])), st)


# ---- tracks whose decoded form is known by construction
def test_a_single_one_appears_at_itself_and_behind_every_tap():
    t = np.zeros(4000, dtype=np.uint8)
    t[100] = 1
    for name in ("nrzi", "g3ruh", "span2047"):
        st = LR.settings(name)
        u, rec = coded(t, st, offset=7)
        want = sorted({100} | {100 + d for d in st.delta})
        assert np.flatnonzero(u).tolist() == want and rec["n_ones"] == len(want), name
    assert LR.settings("g3ruh").delta == [768, 1088] and LR.settings("nrzi").delta == [10] and LR.settings("span2047").delta == [64, 2047]
    u, rec = coded(t[:150], LR.settings("g3ruh"))  # a run shorter than the smallest delta: the track itself
    assert np.array_equal(u, t[:150]) and rec["n_ones"] == 1


def test_nrzi_and_g3ruh_symbol_sequences_decode_to_their_data():
    rng = np.random.default_rng(8)
    data = rng.integers(0, 2, 300).tolist()
    line = np.cumsum(data) % 2  # NRZI: a 1 toggles the level
    u, _ = coded(held(line, 10), linecode.nrzi(38400))
    assert np.array_equal(u, held(data, 10))  # at every sample: the track is ideal, and ahead of the chain it reads 0
    u, _ = coded(held(1 - line, 10), linecode.nrzs(38400))  # NRZ-S on the complemented line: a 0 toggles
    assert np.array_equal(u[10:], held([1 - x for x in data], 10)[10:])
    s = scrambled(data, (12, 17))
    assert P.descrambled(s) == data
    u, rec = coded(held(s, 64), linecode.g3ruh(6000))
    assert np.array_equal(u, held(data, 64)) and rec["n_ones"] == 64 * sum(data)
    assert track.slice_bits(u, 6000) == data


def test_invert_complements_every_bit_and_what_lies_ahead_of_the_chain():
    rng = np.random.default_rng(9)
    t = rng.integers(0, 2, 3000).astype(np.uint8)
    for taps in (1, 0x10800):
        plain, _ = coded(t, linecode.Settings(6000, taps))
        inv, rec = coded(t, linecode.Settings(6000, taps, True))
        assert np.array_equal(inv, 1 - plain) and rec["n_ones"] == 3000 - int(plain.sum())
    zero, _ = coded(np.zeros(500, dtype=np.uint8), linecode.nrzs(6000))
    assert zero.all()  # the first 64 too: 0 ^ 0 ^ 1
    assert linecode.nrzs(6000).flags == linecode.INVERT == 1 and linecode.nrzi(6000).flags == 0


def test_delta_at_the_limits():
    assert [linecode.delta(6000, j) for j in (1, 12, 17)] == [64, 768, 1088] and linecode.delta(38400, 1) == 10
    # per highest tap the lowest rate it is accepted at: the span is exactly 2047 there and 2048 a bit/s below
    for j, rate in ((12, 2251), (17, 3189), (26, 4877), (32, 6002)):
        assert linecode.Settings(rate, 1 << (j - 1)).span == 2047 and linecode.delta(rate - 1, j) == 2048, j
        with pytest.raises(ValueError):
            linecode.Settings(rate - 1, 1 << (j - 1))
    assert [linecode.delta(r, 32) for r in (6004, 6003, 6002, 6001)] == [2047, 2047, 2047, 2048]  # 6001: the first refused
    assert linecode.Settings(1000, 0b11111).span == 1920 and linecode.delta(1000, 6) == 2304
    assert linecode.Settings(96000, 0xFFFFFFFF).span == 128 and linecode.Settings(96000, 0xFFFFFFFF).delays == list(range(1, 33))
    for bad in ((999, 1), (96001, 1), (6000, 0), (6000, 1 << 32), (6000, -1), (1000, 0b100000)):
        with pytest.raises(ValueError):
            linecode.Settings(*bad)
    assert (linecode.g3ruh(6000).taps, linecode.nrzi(6000).taps, linecode.nrzs(6000).taps, linecode.nrzs(6000).invert) == (0x10800, 1, 1, True)
    assert linecode.g3ruh(6000).delays == [12, 17] and linecode.HISTORY == sync.HISTORY == 2047


# ---- cutting
def compositions(n):
    return [c for k in range(1, n + 1) for c in itertools.product(range(1, n + 1), repeat=k) if sum(c) == n]


@pytest.mark.parametrize("name,drop", [("whb", 0), ("tfa_1", 0), ("tfa_1", 3000)])
def test_every_block_cut_merges_to_the_uncut_result(name, drop):
    """The scenes as they are -- TFA_1's bursts lie inside blocks --, and TFA_1 with its first 3000 samples taken away, so that its
    first burst lies across a block boundary."""
    rate, m, L = P.GOLDEN[name][:3]
    d = golden_dec(name)[2 * drop:]
    nb = len(d) // (2 * B)
    d = d[:2 * B * nb]
    st = linecode.g3ruh(rate)
    whole = linecode.chains(code_submits([s[1:] for s in P.submits(d, (nb,), L, m)], st))
    assert len(whole) == (1 if drop else len(P.GOLDEN[name][3])) and all(c.bits.any() for c in whole)  # (moved: the whole blocks hold the first burst)
    cuts = 0
    for sizes in compositions(nb):
        tsubs = [s[1:] for s in P.submits(d, sizes, L, m)]
        cuts += sum(1 for recs, _ in tsubs for r in recs if r["flags"] & CONT)
        got = linecode.chains(code_submits(tsubs, st))
        assert len(got) == len(whole)
        for a, b in zip(got, whole):
            assert stripped(a.rec) == stripped(b.rec) and np.array_equal(a.bits, b.bits), sizes
    assert (cuts >= 1) == (name == "whb" or drop > 0)


@pytest.mark.parametrize("name", list(LR.SETS))
def test_pieces_of_1000_500_and_the_rest_need_the_combined_history(name):
    st = LR.settings(name)
    t = np.random.default_rng(12).integers(0, 2, 6000).astype(np.uint8)
    whole = linecode.chains(both_submits([hand_track(t, start=7000)], st))[0]
    for sizes in ((1000, 500), (1000, 500, 40, 1, 700), (3, 2047), (2048,)):
        got = linecode.chains(both_submits(pieces_of(t, sizes), st))
        assert len(got) == 1 and np.array_equal(got[0].bits, whole.bits), sizes
        assert stripped(got[0].rec) == stripped(whole.rec)
    alone = [linecode.codes(*p, st)[:2] for p in pieces_of(t, (1000, 500))]  # without the history the pieces differ: the carry matters
    assert not np.array_equal(np.concatenate([track.bits_of(r[0], w) for r, w in alone]), whole.bits)


def test_a_first_piece_of_three_samples_behind_a_stale_history():
    """H = 3: the bits ahead of the chain read 0 whatever the stream held before."""
    st = LR.settings("g3ruh")
    rng = np.random.default_rng(13)
    old, t = rng.integers(0, 2, 4000).astype(np.uint8), rng.integers(0, 2, 3000).astype(np.uint8)
    whole, _ = coded(t, st)
    first = both(*hand_track(old, OPEN), st)  # an earlier chain leaves its last 2047 bits
    assert len(first[2]["bits"][0]) == 2047
    a = both(*hand_track(t[:3], OPEN, start=9000), st, first[2])  # a new chain: not CONTINUES, 3 samples, open
    assert len(a[2]["bits"][0]) == 3 and a[2]["bits"][0].tolist() == t[:3].tolist()
    b = both(*hand_track(t[3:], CONT, start=9003), st, a[2])
    assert np.array_equal(np.concatenate([track.bits_of(a[0][0], a[1]), track.bits_of(b[0][0], b[1])]), whole)
    # a piece that CONTINUES with no history left (the piece before did not fit the pool): everything ahead reads 0
    c = both(*hand_track(t[3:], CONT, start=9003), st, linecode.fresh_state(1))
    assert np.array_equal(track.bits_of(c[0][0], c[1]), coded(t[3:], st)[0])


# ---- the figures the feature was specified with
@functools.lru_cache(maxsize=None)
def whb(hz):
    """-> (the merged phase track, the merged coded track) of the golden WHB scene rotated by hz."""
    rate, m, L = P.GOLDEN["whb"][:3]
    d = rotated(golden_dec("whb"), hz) if hz else golden_dec("whb")
    tsubs = [s[1:] for s in P.submits(d, (len(d) // (2 * B),), L, m)]
    csubs = both_submits(tsubs, linecode.g3ruh(rate)) if hz == 0 else code_submits(tsubs, linecode.g3ruh(rate))
    return track.chains(tsubs), linecode.chains(csubs), csubs


@pytest.mark.parametrize("hz", (0,) + P.ROTATIONS)
def test_the_golden_whb_scene_frames_behind_the_descrambler(hz):
    tch, cch, csubs = whb(hz)
    assert len(cch) == 1 and int(cch[0]["last_over"]) == P.GOLDEN["whb"][3][0][2] == 27650 and int(cch[0]["n_ones"]) == LR.WHB_N_ONES
    for E, want in ((0, [LR.WHB_PLATEAU]), (1, [LR.WHB_PLATEAU]), (2, [LR.WHB_PLATEAU, LR.WHB_PLATEAU_E2])):
        st = sync.Settings(6000, LR.WORD, 16, E)
        sch = sync.chains(sync_submits(csubs, st))
        assert [sync.plateaus(s.bits) for s in sch] == [want], E
        fr = sync.frames(cch[0], sch[0], st, 26, lsb=True)
        assert fr[0][:3] == (14312, 0, "+") and len(fr[0][3]) == 208 and sync.hex_of(fr[0][3], True) == LR.WHB_FRAME
        assert sync.line("f", sch[0], fr[0]) == "frame f 10004 24316 0 + 208 " + LR.WHB_FRAME
    assert P.whb_event_bytes()[6:6 + 52] == LR.WHB_FRAME  # bytes 3 .. 28 of the golden event
    assert fr[0][3] == P.lsb_first(P.whb_event_bytes())[24:24 + 208]
    sl = track.slice_bits(cch[0].bits[:27651], 6000)
    assert len(sl) == LR.WHB_SLICED and sl == P.descrambled(P.sliced(tch[0], 6000))
    assert linecode.line("f", cch[0], 6000) == "code f 10004 28344 27651 432 " + track.hex_of(sl)
    # the contrast: the raw track has no b42b at E <= 1
    raw = sync.syncs(tch[0].rec.reshape(1), hand_track(tch[0].bits, offset=int(tch[0]["bit_offset"]))[1], sync.Settings(6000, LR.WORD, 16, 1), None, 1)[0]
    assert (int(raw[0]["best"]), int(raw[0]["n_hits"])) == (LR.WHB_RAW_BEST, 0)


def test_tfa_1s_two_frames_read_lsb_first_without_a_code():
    rate, m, L = P.GOLDEN["tfa_1"][:3]
    d = golden_dec("tfa_1")
    tsubs = [s[1:] for s in P.submits(d, (len(d) // (2 * B),), L, m)]
    st = sync.Settings(rate, LR.WORD, 16, 0)
    got = []
    for t, s in zip(track.chains(tsubs), sync.chains(sync_submits(tsubs, st))):
        fr = sync.frames(t, s, st, 9, lsb=True)
        assert len(fr) == 1 and fr[0][1:3] == (0, "+") and len(fr[0][3]) == 72
        got.append(sync.line("f", s, fr[0]).split()[-1])
    assert tuple(got) == LR.TFA_1_FRAMES == tuple(tel[4:] for tel in P.TFA_1_TELEGRAMS)


def test_frames_and_line_without_lsb_are_what_they_were():
    d = golden_dec("tfa_2")[:2 * 4 * B]
    tsubs = submits(d, (4,), 11)
    st = sync.Settings(17240, 0x2DD4, 16, 0)
    pairs = list(zip(track.chains(tsubs), sync.chains(sync_submits(tsubs, st))))
    lines = [sync.line("f", s, f) for t, s in pairs for f in sync.frames(t, s, st, 4)]
    assert lines == ["frame f 10003 10533 0 + 32 96070960", "frame f 25583 26113 0 + 32 98812225"]
    for t, s in pairs:
        a, b = sync.frames(t, s, st, 4), sync.frames(t, s, st, 4, lsb=True)
        assert type(a[0][3]) is list and a == [tuple(f[:3]) + (list(f[3]),) for f in b]  # the same bits, the same n_bits
        assert sync.line("f", s, a[0], lsb=True) == sync.line("f", s, b[0]) != sync.line("f", s, a[0])
    assert sync.line("f", pairs[0][1], sync.frames(*pairs[0], st, 4, lsb=True)[0]).split()[-1] == "69e09006"  # 96070960, every byte reversed
    # a last partial byte is zero-filled at the top, two digits a byte; the MSB-first form pads the last nibble
    assert sync.hex_of([1, 0, 0, 0, 0, 0, 0, 0, 1, 1, 0], True) == "0103" and sync.hex_of([1, 0, 0, 0, 0, 0, 0, 0, 1, 1, 0]) == "80c"
    assert sync.hex_of([1], True) == "01" and sync.hex_of([], True) == ""


# ---- the declarations, the exports, the memory sums
def test_the_header_the_exports_and_the_memory_sums(tmp_path):
    src = tmp_path / "code.c"
    src.write_text('#include <stddef.h>\n#include "tfrec_amd.h"\n'
                   "_Static_assert(sizeof(tfrec_amd_track) == 40 && offsetof(tfrec_amd_track, n_ones) == 36, \"the record is the track's\");\n"
                   "_Static_assert(TFREC_AMD_CODE_INVERT == %d, \"flag\");\n" % linecode.INVERT +
                   "int (*enable)(tfrec_amd_ctx *, int32_t, uint32_t, uint32_t) = tfrec_amd_enable_burst_code;\n"
                   "int (*read)(tfrec_amd_ctx *, tfrec_amd_track *, size_t, uint32_t *, uint32_t *, size_t, uint64_t *) = tfrec_amd_read_burst_codes;\n")
    subprocess.check_call(["cc", "-std=c11", "-fsyntax-only", "-I", os.path.join(parity.ROOT, "include"), str(src)])
    L = api.load_library()
    for sym in ("tfrec_amd_enable_burst_code", "tfrec_amd_read_burst_codes"):
        assert sym in api.EXPORTS
        getattr(L, sym)
    assert hasattr(api.Receiver, "enable_burst_code") and hasattr(api.Receiver, "read_burst_codes")
    # no GPU is needed to be refused
    assert L.tfrec_amd_enable_burst_code(None, 6000, 0x10800, 0) == api.E_INVAL
    n, w = C.c_uint32(7), C.c_uint64(9)
    assert L.tfrec_amd_read_burst_codes(None, None, 0, C.byref(n), None, 0, C.byref(w)) == api.E_INVAL and (n.value, w.value) == (7, 9)
    # the memory sums: the records and the bitmap per FIFO set; 260 bytes per stream; nothing page-locked
    assert linecode.device_bytes(3, 10, 65) == api.FIFO_DEPTH * (400 + 12) + 3 * 260 and linecode.pinned_bytes(3) == 0
    head = open(os.path.join(parity.ROOT, "include", "tfrec_amd.h")).read()
    text = head[head.index("Line code (tfrec_amd_enable_burst_code"):head.index("int tfrec_amd_enable_burst_code(tfrec_amd_ctx")]
    for words in ("floor((768000 j + R) / (2 R))", "<= 2047", "ahead of the chain's first sample", "TFREC_AMD_E_OVERFLOW", "tfrec_amd_save_streams",
                  "real recordings", "0x10800"):
        assert words in text, words


# ---- tfrec_gpu's own code: job.h in a stand-alone program
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("linecode") / "linecode_driver")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(parity.ROOT, "tests", "linecode_driver.cpp")])
    return exe


def run_driver(exe, lines):
    out = subprocess.run([exe], input="".join(ln + "\n" for ln in lines), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    return out.stdout.splitlines()


def test_the_hosts_argument_span_and_byte_order_are_the_restatements(driver):
    args = {"g3ruh": (0x10800, 0), "nrzi": (1, 0), "nrzs": (1, 1), "g3ruh,inv": (0x10800, 1), "nrzs,inv": (1, 0), "10800": (0x10800, 0),
            "1,inv": (1, 1), "FFFFFFFF": (0xFFFFFFFF, 0), "80000001,inv": (0x80000001, 1), "0010": (16, 0)}
    for name, (taps, inv) in linecode.NAMED.items():
        assert args[name] == (taps, int(inv))
    bad = ["0", "", "123456789", "g3ruh,", "g3ruh,x", "xyz", "1,inv,inv", "00000000", "G3RUH", "nrzi,", ",inv", "-1"]
    got = run_driver(driver, ["parse " + a for a in list(args) + bad])
    assert got == ["taps %x %d" % v for v in args.values()] + ["bad"] * len(bad)
    spans = [(0x10800, 6000), (1, 38400), (1 << 31, 6002), (1 << 31, 6001), (1 << 11, 2250), (0xFFFFFFFF, 96000), (0b100000, 1000), (1, 1000)]
    got = run_driver(driver, ["span %x %d" % s for s in spans])
    assert got == ["span %d" % linecode.delta(r, t.bit_length()) for t, r in spans]
    assert [int(g.split()[1]) <= 2047 for g in got] == [True, True, True, False, False, True, False, True]
    rng = np.random.default_rng(14)
    frames = [rng.integers(0, 2, n).tolist() for n in (0, 1, 7, 8, 9, 11, 16, 208, 2048)]
    piece = sync.Piece(np.zeros(1, dtype=sync.SYNC_DTYPE)[0], np.zeros(0))
    piece["start_sample"] = 1000
    lines, want = [], []
    for b in frames:
        for lsb in (0, 1):
            lines.append("frame %d %s" % (lsb, "".join("01"[x] for x in b) or "-"))
            want.append(sync.line("f", piece, (30, 0, "+", b), lsb=bool(lsb)))
    assert run_driver(driver, lines) == want and want[0] == "frame f 1000 1030 0 + 0 -" and want[3].endswith(" 1 0%d" % frames[1][0])


@pytest.mark.parametrize("name", ["g3ruh", "nrzs"])
def test_the_host_merges_coded_pieces_and_prints_the_restatements_line(driver, name):
    st = LR.settings(name)
    data = np.random.default_rng(15).integers(0, 2, 200).tolist()
    t = held(scrambled(data, (12, 17)), 64) if name == "g3ruh" else held(data, 10)
    lines, want = ["rate %d" % st.rate, "file 100"], []
    for sizes, start in (((1000, 500), 7000), ((3, 2047), 30000), ((), 60000)):
        csubs = code_submits(pieces_of(t, sizes, start=start), st)
        for recs, words in csubs:
            r = recs[0]
            lines.append("piece 1 %d %d %d %d %d %d %s" % (int(r["flags"]), int(r["start_sample"]), int(r["n_samples"]), int(r["bit_offset"]),
                                                            int(r["last_over"]), int(r["n_ones"]), " ".join("%x" % w for w in words)))
        # (pieces_of marks every piece's last sample over: the merged last_over is the chain's last sample)
        want += [linecode.line("f", c, st.rate) for c in linecode.chains(csubs)]
    assert run_driver(driver, lines) == want and len(want) == 3
    if name == "g3ruh":
        assert want[0].split()[5:] == ["200", track.hex_of(data)]


# ---- the command line
def test_cli_code_usage_errors_and_accepted_forms(tmp_path):
    parity.build_cli()
    f = str(tmp_path / "missing.iq")
    out = parity.run_cli(["-U", "g3ruh", "-L", f])
    assert out.returncode == 1 and "-U codes" in out.stderr  # without -G
    for bad in ("0", "", "123456789", "g3ruh,", "g3ruh,x", "xyz", "1,inv,inv", "G3RUH"):
        out = parity.run_cli(["-G", "6000", "-U", bad, "-L", f])
        assert out.returncode == 1 and "bad -U" in out.stderr, bad
    for rate, taps in (("6000", "g3ruh"), ("6001", "80000000"), ("2250", "800"), ("1000", "20")):  # 6000: no, 12 and 17 symbols fit; see below
        out = parity.run_cli(["-G", rate, "-U", taps, "-L", f])
        assert (out.returncode == 1 and "more than 2047" in out.stderr) == (taps != "g3ruh"), (rate, taps)
    for args in (["-X", f], ["-s", "50", "-L", f], ["-A", "-L", f]):  # whatever -G refuses
        out = parity.run_cli(["-G", "6000", "-U", "g3ruh"] + args)
        assert out.returncode == 1 and "-G reads" in out.stderr, args
    for k in ("-k", "-K"):
        out = parity.run_cli(["-G", "6000", "-U", "g3ruh", k, str(tmp_path / "keep"), "-L", f])
        assert out.returncode == 2 and "not with -G" in out.stderr
    for bad in ("b42b,0,4,0,2", "b42b,0,4,0,x", "b42b,0,4,0,", "b42b,0,4,0,1,1"):  # -Y's fifth field is the flag 1
        out = parity.run_cli(["-G", "6000", "-Y", bad, "-L", f])
        assert out.returncode == 1 and "bad -Y" in out.stderr, bad
    out = parity.run_cli(["-h"])
    assert "-U code[,inv]" in out.stderr and "[-U g3ruh|nrzi|nrzs|hextaps[,inv]]" in out.stderr and "-Y h,e,n,b,1" in out.stderr
    assert "-Y h[,e[,n[,b]]]" in out.stderr and "[-Y hex[,errors[,bytes[,both]]]]" in out.stderr  # the others' stay
    for args in (["-G", "6000,psk", "-U", "g3ruh"], ["-U", "nrzs", "-G", "38400,psk,10"], ["-G", "6002", "-U", "80000001,inv"],
                 ["-G", "6000,psk", "-U", "g3ruh", "-Y", "b42b,0,26,0,1"], ["-G", "17240", "-Y", "2dd4,0,4,0,1"], ["-G", "6000,auto", "-U", "nrzi"],
                 ["-G", "6000", "-O", "2000", "-U", "1"], ["-G", "6000", "-U", "g3ruh", "-M", "-Q", "-C"],
                 ["-G", "6000", "-U", "g3ruh", "-S", str(tmp_path / "cap"), "-n", "1"], ["-G", "6000", "-U", "g3ruh", "-d", "0"]):
        out = parity.run_cli(args + ["-L", f])  # accepted: the file is looked for
        assert out.returncode == 2 and "missing.iq" in out.stderr, args
    out = parity.run_cli(["-G", "6000,psk", "-U", "g3ruh", "-R", str(tmp_path / "nothing")])  # accepted with -R: the capture is looked for
    assert out.returncode == 2 and "-R replays" not in out.stderr and "bad -U" not in out.stderr
