"""The burst track without a GPU (tfrec_amd_enable_burst_track, tfrec_gpu -G): the restatement tfrec_amd/track.py
against its per-sample form, the bits of the golden scenes against the golden telegrams (also rotated, about the matching centre),
the centre's table index, the zero sum, the quarter-turn centres, the behaviour under cutting and the carried chain position, the
slicer's walk, tfrec_gpu's merge, slice and line (tfrec_amd/host/job.h, compiled into a stand-alone program under the address and
undefined-behaviour sanitizers), the struct and the exports, and what tfrec_gpu decides before it opens a device.

Everything is exact integers: there is no tolerance anywhere.  The golden TFA_1 and WHB scenes do not slice with this discriminator
(limits); nothing is asserted about their bits beyond the agreement of the two forms.  Nothing here is measured on
real recordings."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import parity
from recorder_rows import GOLDEN, RATE, TELEGRAMS, bit_string, golden_dec, pattern, rotated, stripped, submits
from tfrec_amd import api, capture, envelope, levels, track, tune
from meter_rows import crafted_dec

B = levels.BLOCK_DEC
CONT, OPEN = capture.RUN_CONTINUES, capture.RUN_OPEN


@functools.lru_cache(maxsize=None)
def golden_chains(name, hz=0):
    dec = golden_dec(name) if hz == 0 else rotated(golden_dec(name), hz)
    return track.chains(submits(dec, (len(dec) // (2 * B),), track.smooth_of(RATE[name]), hz))


def table(*rows):
    """A run table by hand: (start, n[, flags]) of stream 0, packed in order."""
    t = np.zeros(len(rows), dtype=capture.RUN_DTYPE)
    off = 0
    for k, r in enumerate(rows):
        t[k]["start_sample"], t[k]["n_samples"], t[k]["thresh"] = r[0], r[1], 500
        t[k]["flags"] = r[2] if len(r) > 2 else 0
        t[k]["pool_offset"] = off
        off += r[1]
    return t


def same(a, b):
    (ra, wa, sa), (rb, wb, sb) = a, b
    assert ra.dtype == rb.dtype == track.TRACK_DTYPE and ra.tobytes() == rb.tobytes()
    assert wa.dtype == wb.dtype == np.dtype("<u4") and wa.tobytes() == wb.tobytes()
    assert np.array_equal(sa["carry"], sb["carry"]) and np.array_equal(sa["prior"], sb["prior"])


def pairs(z):
    return np.asarray(z, dtype=np.int16).reshape(-1)


# ---- the restatement against its per-sample form
@pytest.mark.parametrize("L", [1, 5, 16])
def test_the_vectorised_form_equals_the_per_sample_one_on_crafted_samples(L):
    dec, _ = crafted_dec(max(levels.windows(0x2F)), 0x2F)
    dec = dec.reshape(-1)
    runs = capture.captures(dec, 0x2F, 500)[0]
    thr = envelope.thresholds(dec, 0x2F, 500)[0]
    assert len(runs) >= 1
    for hz in (0, 20000, -35000):
        same(track.tracks([dec], [thr], runs, L, [hz]), track.tracks_bruteforce([dec], [thr], runs, L, [hz]))
    # a table by hand on the same samples: neighbours that share a word, a run at sample 0, one to the last sample; and a state to
    # continue from
    M = len(dec) // 2
    t = table((0, 37, CONT), (40, 1), (41, 70), (5000, M - 5000, OPEN))
    st = track.fresh_state(1)
    st["carry"][0] = np.arange(32).reshape(16, 2) * 700 - 9000
    st["prior"][0] = 7
    a = track.tracks([dec], [thr], t, L, [0], st)
    same(a, track.tracks_bruteforce([dec], [thr], t, L, [0], st))
    assert a[2]["prior"][0] == 16 and a[0]["bit_offset"].tolist() == [0, 37, 38, 108]


@pytest.mark.parametrize("name", GOLDEN)
def test_the_vectorised_form_equals_the_per_sample_one_on_the_golden_scenes(name):
    dec = golden_dec(name)
    L = track.smooth_of(RATE[name])
    fast, slow = submits(dec, (len(dec) // (2 * B),), L), submits(dec, (len(dec) // (2 * B),), L, brute=True)
    assert len(fast[0][0]) >= 1
    assert fast[0][0].tobytes() == slow[0][0].tobytes() and fast[0][1].tobytes() == slow[0][1].tobytes()


# ---- what the bursts said
@pytest.mark.parametrize("hz", [0, 20000])
def test_the_golden_telegrams_first_six_bytes_are_read(hz):
    """MSB-first and in positive polarity, from the first last_over + 1 samples; after a rotation by +20 kHz about centre 20000."""
    for name, want in TELEGRAMS.items():
        got = golden_chains(name, hz)
        assert len(got) == 2 and track.smooth_of(RATE[name]) == (11 if name == "tfa_2" else 16)
        for c, tel in zip(got, want):
            length = int(c["last_over"]) + 1
            symbols = track.slice_bits(c.bits[:length], RATE[name])
            print(name, hz, length, len(symbols), track.hex_of(symbols))
            assert pattern(tel) in bit_string(symbols)
    if hz == 0:
        a, b = golden_chains("tfa_2")
        assert (int(a["last_over"]), int(b["last_over"])) == (1473, 1474)
        assert track.line("f.iq", a, 17240) == "bits f.iq 10003 2167 1474 66 aa2dd4960709605b4"
        assert track.line("f.iq", b, 17240) == "bits f.iq 25583 2168 1475 66 aa2dd498812225304"


def test_the_scenes_that_do_not_slice():
    """The stated limit: about centre 0 the TFA_1 scene's first run is all zeros and the WHB run all ones."""
    a = golden_chains("tfa_1")[0]
    assert not a.bits[:int(a["last_over"]) + 1].any() and track.line("f", a, 38400).endswith(" 336 " + "0" * 84)
    w = golden_chains("whb")[0]
    assert w.bits[1:int(w["last_over"]) + 1].all()


# ---- the centre
def test_index_of():
    assert track.index_of(0) == 0
    assert track.index_of(46) == 0 and track.index_of(47) == 1  # 4096 * 47 / 384000 = 0.501
    assert track.index_of(-46) == 0 and track.index_of(-47) == 4095
    assert track.index_of(192000) == 2048 and track.index_of(-192000) == 2048  # -2047.5 floors to -2048
    # a negative centre whose floor is not its truncation: (8192 * -141 + 384000) / 768000 = -1.004: -2, not -1
    assert track.index_of(-141) == 4094 and int((8192 * -141 + 384000) / 768000) == -1
    assert track.index_of(96000) == 1024 and track.index_of(-96000) == 3072
    for bad in (192001, -192001):
        with pytest.raises(ValueError):
            track.index_of(bad)


def test_a_zero_sum_gives_zero():
    # v = crs C[0] about centre 0: crs alternates +c, -c, so every sum over two products is exactly 0 and over one it is +-c
    z = np.zeros((64, 2), dtype=np.int16)
    z[0::4], z[1::4], z[2::4], z[3::4] = (1000, 0), (0, 1000), (1000, 0), (0, 1000)  # crs: +, -, +, - ...
    t = table((0, 64))
    th = [np.full(64, 500)]
    r1, w1, _ = track.tracks([pairs(z)], th, t, 1)
    r2, w2, _ = track.tracks([pairs(z)], th, t, 2)
    b1, b2 = track.bits_of(r1[0], w1), track.bits_of(r2[0], w2)
    assert b1.tolist() == [0] + [1, 0] * 31 + [1]  # the chain's first sample has no product
    assert b2.tolist() == [0, 1] + [0] * 62 and r2[0]["n_ones"] == 1  # k = 1: one term; then +c - c = 0: not greater than 0
    same(track.tracks([pairs(z)], th, t, 2), track.tracks_bruteforce([pairs(z)], th, t, 2))
    silent = np.zeros(128, dtype=np.int16)
    r0, w0, _ = track.tracks([silent], [np.full(64, 500)], t, 5)
    assert not w0.any() and r0[0]["n_ones"] == 0 and r0[0]["last_over"] == -1


def test_the_quarter_turn_centres():
    """r = 1024: C = 0, S = 32767, v = -32767 dot; r = 3072: v = +32767 dot.  A tone at +96 kHz has dot = 0: silence about both; one a
    little above it reads 1 about +96000, and about -96000 what its dot says."""
    c, s = tune.table()
    assert (c[1024], s[1024], c[3072], s[3072]) == (0, 32767, 0, -32767)
    n = np.arange(256)
    t = table((0, 256))
    th = [np.full(256, 500)]
    for f, about_plus, about_minus in ((110000, 1, 0), (82000, 0, 1)):
        ph = 2 * np.pi * f * n / 384000.0
        dec = pairs(np.stack([np.rint(8000 * np.cos(ph)), np.rint(8000 * np.sin(ph))], axis=1))
        for hz, want in ((96000, about_plus), (-96000, about_minus)):
            r, w, _ = track.tracks([dec], th, t, 4, [hz])
            same((r, w, _), track.tracks_bruteforce([dec], th, t, 4, [hz]))
            assert track.bits_of(r[0], w)[1:].tolist() == [want] * 255, (f, hz)


# ---- cutting
@pytest.mark.parametrize("name", ["tfa_2", "whb"])
def test_the_merged_chains_are_the_uncut_stream_for_every_block_cut(name):
    dec = golden_dec(name)
    dec = dec[:2 * B * min(8, len(dec) // (2 * B))]
    nb = len(dec) // (2 * B)
    L = track.smooth_of(RATE[name])
    key = lambda c: (int(c["stream"]), int(c["start_sample"]))  # noqa: E731
    whole = sorted(track.chains(submits(dec, (nb,), L)), key=key)
    assert len(whole) >= 1
    cuts = 0
    for sizes in [(1,) * nb] + [(k, nb - k) for k in range(1, nb)]:
        subs = submits(dec, sizes, L)
        cuts += sum(1 for recs, _ in subs for r in recs if r["flags"] & CONT)
        got = sorted(track.chains(subs), key=key)
        assert len(got) == len(whole)
        for a, b in zip(got, whole):
            assert stripped(a.rec) == stripped(b.rec) and np.array_equal(a.bits, b.bits), (sizes, key(a))
            assert track.line("f", a, RATE[name]) == track.line("f", b, RATE[name])
    assert cuts >= 1 or name != "whb"  # the WHB telegram spans blocks


@pytest.mark.parametrize("L", [1, 5, 16])
def test_a_chain_whose_first_piece_is_three_samples_at_a_submits_end(L):
    """prior is 3: the second piece's first samples sum over fewer than L products, and none of a sample ahead of the chain."""
    rng = np.random.default_rng(5)
    dec = rng.integers(-3000, 3000, 2 * 2 * B).astype(np.int16)
    thr = np.full(2 * B, 500)
    whole = track.tracks([dec], [thr], table((B - 3, 3 + 100)), L, [20000])
    a = track.tracks([dec[:2 * B]], [thr[:B]], table((B - 3, 3, OPEN)), L, [20000])
    assert a[2]["prior"][0] == 3
    t2 = table((0, 100, CONT))
    t2["start_sample"] = B
    b = track.tracks([dec[2 * B:]], [thr[B:]], t2, L, [20000], a[2], base=[B])
    same(b, track.tracks_bruteforce([dec[2 * B:]], [thr[B:]], t2, L, [20000], a[2], base=[B]))
    m = track.chains([(a[0], a[1]), (b[0], b[1])])
    assert len(m) == 1 and stripped(m[0].rec) == stripped(whole[0][0])
    assert np.array_equal(m[0].bits, track.bits_of(whole[0][0], whole[1]))
    # the samples ahead of the chain do not matter: other samples there, the same track
    other = dec.copy()
    other[:2 * (B - 3)] = rng.integers(-3000, 3000, 2 * (B - 3))
    a2 = track.tracks([other[:2 * B]], [thr[:B]], table((B - 3, 3, OPEN)), L, [20000])
    b2 = track.tracks([other[2 * B:]], [thr[B:]], t2, L, [20000], a2[2], base=[B])
    assert a2[1].tobytes() == a[1].tobytes() and b2[1].tobytes() == b[1].tobytes()
    # a chain longer than 16 holds prior at 16, and a piece that is not OPEN leaves 0
    assert track.tracks([dec[:2 * B]], [thr[:B]], table((B - 40, 40, OPEN)), L)[2]["prior"][0] == 16
    assert track.tracks([dec[:2 * B]], [thr[:B]], table((B - 40, 39)), L)[2]["prior"][0] == 0
    assert b[2]["prior"][0] == 0


def test_merge_takes_the_ends_flags_and_the_last_over_of_the_last_piece_that_has_one():
    p = np.zeros(3, dtype=track.TRACK_DTYPE)
    p["flags"], p["n_samples"], p["n_ones"], p["last_over"] = (OPEN, CONT | OPEN, CONT), (5, 8, 3), (2, 3, 1), (4, 6, -1)
    p["start_sample"], p["thresh"], p["bit_offset"] = (3192, 8192, 16384), (500, 600, 700), (64, 0, 0)
    bits = [np.array(b, dtype=np.uint8) for b in ([1, 0, 0, 0, 1], [1, 1, 1, 0, 0, 0, 0, 0], [0, 1, 0])]
    m = track.merge([track.Piece(r, b) for r, b in zip(p, bits)])
    assert [int(m[f]) for f in track.TRACK_DTYPE.names] == [0, 0, 3192, 16, 500, 64, 11, 6]
    assert m.bits.tolist() == sum((b.tolist() for b in bits), [])
    assert track.merge([track.Piece(p[0], bits[0]), track.Piece(p[1], bits[1])])["flags"] == OPEN
    none = p.copy()
    none["last_over"] = -1
    assert track.merge([track.Piece(r, b) for r, b in zip(none, bits)])["last_over"] == -1


# ---- the slicer
def runs_of(*lens, first=0):
    return np.concatenate([np.full(m, (first + k) % 2, dtype=np.uint8) for k, m in enumerate(lens)])


def test_the_slicers_walk():
    R = 17240  # 22.27 samples a symbol: sym(m) = 0 for m <= 11, 1 for 12 .. 33, 2 for 34 .. 55
    assert [track.sym(m, R) for m in (11, 12, 33, 34, 55, 56)] == [0, 1, 1, 2, 2, 3]
    assert track.slice_bits([], R) == [] and track.slice_bits(runs_of(11), R) == []
    assert track.slice_bits(runs_of(22, 22, 45, 22), R) == [0, 1, 0, 0, 1]
    assert track.slice_bits(runs_of(5, 3, 22, 22), R) == [0, 1]  # leading glitches are dropped: the first kept run is the 22 zeros
    assert track.slice_bits(runs_of(5, 22, 22), R) == [1, 0]  # ... whatever their value
    assert track.slice_bits(runs_of(20, 4, 20, 22), R) == [0, 0, 1]  # a glitch inside a run joins it: 44 samples, two symbols
    assert track.slice_bits(runs_of(22, 3, 2, 3, 22), R) == [0, 0]  # glitches in a row, then the same value again: 52 samples
    assert track.slice_bits(runs_of(22, 3, 2, 17, 22), R) == [0, 1, 0]  # ... then the other value: the 27 samples are one symbol
    assert track.slice_bits(runs_of(22, 22, 6), R) == [0, 1]  # a trailing glitch joins the last run (28 samples: one symbol)
    assert track.slice_bits(runs_of(22, 16, 6), R) == [0, 1]  # 16 + 6: still one
    assert track.slice_bits(runs_of(22, 100), R) == [0] + [1] * 4  # a trailing run is emitted at the end
    assert track.hex_of([1, 0, 1, 0, 1]) == "a8" and track.hex_of([]) == ""
    p = track.Piece(np.zeros((), dtype=track.TRACK_DTYPE), runs_of(22, 22, 45, 22))
    p.rec["n_samples"], p.rec["last_over"], p.rec["start_sample"] = 111, 110, 7
    assert track.line("a.iq", p, R) == "bits a.iq 7 111 111 5 48"
    p.rec["last_over"] = 43  # the slice takes the first last_over + 1 samples only
    assert track.line("a.iq", p, R) == "bits a.iq 7 111 44 2 4"
    p.rec["last_over"] = -1
    assert track.line("a.iq", p, R) == "bits a.iq 7 111 0 0 -"


def long_chain():
    """9 pieces of 2^17 samples whose track flips every 22 samples: longer than the 2^20 that are kept."""
    n = 1 << 17
    t = ((np.arange(9 * n) // 22) % 2).astype(np.uint8)
    recs = np.zeros(9, dtype=track.TRACK_DTYPE)
    recs["n_samples"], recs["last_over"], recs["thresh"] = n, n - 1, 500
    recs["flags"] = [OPEN] + [CONT | OPEN] * 7 + [CONT]
    recs["start_sample"] = n * np.arange(9)
    recs["n_ones"] = [int(t[n * k:n * (k + 1)].sum()) for k in range(9)]
    return recs, [t[n * k:n * (k + 1)] for k in range(9)]


def test_the_cap_of_two_to_the_twenty_samples():
    recs, bits = long_chain()
    m = track.merge([track.Piece(r, b) for r, b in zip(recs, bits)])
    assert m["n_samples"] == 9 << 17 and m["last_over"] == (9 << 17) - 1
    ln = track.line("a.iq", m, 17240).split()
    n_sym = (1 << 20) // 22 + 1  # every whole run of 22 is a symbol, and so are the 2^20 mod 22 = 14 samples left
    assert ln[:6] == ["bits", "a.iq", "0", str(9 << 17), str(9 << 17), "%d+" % n_sym] and len(ln[6]) == (n_sym + 3) // 4
    assert ln[6].startswith("5555")


# ---- tfrec_gpu's merge, slice and line: job.h in a stand-alone program
@pytest.fixture(scope="module")
def merge_driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("track_merge") / "track_merge_driver")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(parity.ROOT, "tests", "merge_driver.cpp")])
    return exe


def batch_lines(nb, slots, recs, words, f, keep=None):
    out = ["batch %d %s" % (nb, " ".join("%d" % s for s in slots)), "words " + " ".join("%x" % w for w in words)]
    for i, r in enumerate(recs):
        v = [f] + [int(r[k]) for k in ("flags", "start_sample", "n_samples", "thresh", "bit_offset", "last_over", "n_ones")]
        out.append("rec " + " ".join("%d" % x for x in v + [int(r["n_samples"]) if keep is None else keep[i]]))
    return out


def hand_batch(bits, f, start, flags=0, last_over=None, keep=None):
    """One batch of one record whose track is `bits`, at bit offset 5 of its bitmap."""
    r = np.zeros(1, dtype=track.TRACK_DTYPE)
    r["n_samples"], r["start_sample"], r["flags"], r["bit_offset"], r["n_ones"] = len(bits), start, flags, 5, int(np.sum(bits))
    r["last_over"] = len(bits) - 1 if last_over is None else last_over
    flat = np.zeros((5 + len(bits) + 31) // 32 * 32, dtype=np.uint8)
    flat[5:5 + len(bits)] = bits
    words = np.packbits(flat.reshape(-1, 32), axis=1, bitorder="little").view("<u4").reshape(-1)
    assert np.array_equal(track.bits_of(r[0], words), bits)
    return r, words, batch_lines(1, [f], r, words, f, keep)


def test_the_host_merge_prints_the_restatements_lines(merge_driver):
    """Two files through one slot, batches of 1 block: the golden WHB scene's first 6 blocks, whose telegram spans four of them, and
    the golden TFA_2 scene; then a file of hand-made records: the slicer's cases, a record that the file's end cuts, one without an
    over sample, and the chain that is longer than what is kept."""
    R = 17240
    files = [("a.iq", golden_dec("whb")[:2 * 6 * B], 16), ("b.iq", golden_dec("tfa_2")[:2 * 4 * B], 11)]
    lines = ["rate %d" % R] + ["file %s %d" % (name, len(dec) // (2 * B)) for name, dec, _ in files] + ["file c.iq 4096"]
    want = []
    for f, (name, dec, L) in enumerate(files):
        subs = submits(dec, (1,) * (len(dec) // (2 * B)), L)
        for recs, words in subs:
            lines += batch_lines(1, [f], recs, words, f)
        assert f or any(r["flags"] & CONT for recs, _ in subs for r in recs)
        want += [track.line(name, c, R) for c in track.chains(subs)]
    assert want[-2:] == ["bits b.iq 10003 2167 1474 66 aa2dd4960709605b4", "bits b.iq 25583 2168 1475 66 aa2dd498812225304"]
    cases = [runs_of(22, 22, 45, 22), runs_of(5, 3, 22, 22), runs_of(5, 22, 22), runs_of(20, 4, 20, 22), runs_of(22, 3, 2, 17, 22),
             runs_of(22, 22, 6), runs_of(22, 100), runs_of(11), runs_of(22, 22, first=1)]
    for k, bits in enumerate(cases):
        r, _, ls = hand_batch(bits, 2, 8192 * k)
        lines += ls
        want.append(track.line("c.iq", track.Piece(r[0], bits), R))
    assert want[-9].endswith(" 5 48") and want[-2].endswith(" 0 -") and want[-1].endswith(" 2 8")
    bits = runs_of(22, 22, 45, 22)
    r, _, ls = hand_batch(bits, 2, 8192 * 20, last_over=-1)  # no over sample: nothing to slice
    lines += ls
    want.append("bits c.iq %d 111 0 0 -" % (8192 * 20))
    # the file's end cuts a record: 50 of its 111 samples are kept, it is OPEN, its ones are counted again; the piece that would
    # continue it lies behind the file's end and never comes
    r, _, ls = hand_batch(bits, 2, 8192 * 4096 - 50, keep=[50])
    lines += ls
    cut = r[0].copy()
    cut["n_samples"], cut["last_over"], cut["flags"] = 50, 49, OPEN
    want.append(track.line("c.iq", track.Piece(cut, bits[:50]), R))
    assert want[-1] == "bits c.iq %d 50 50 2 4" % (8192 * 4096 - 50)
    out = subprocess.run([merge_driver, "track"], input="".join(ln + "\n" for ln in lines), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.splitlines() == want


def test_the_host_keeps_two_to_the_twenty_samples_of_a_chain(merge_driver):
    recs, bits = long_chain()
    lines = ["rate 17240", "file a.iq 144"]
    for r, b in zip(recs, bits):
        words = np.packbits(b.reshape(-1, 32), axis=1, bitorder="little").view("<u4").reshape(-1)
        lines += batch_lines(16, [0], [r], words, 0)
    out = subprocess.run([merge_driver, "track"], input="".join(ln + "\n" for ln in lines), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    want = track.line("a.iq", track.merge([track.Piece(r, b) for r, b in zip(recs, bits)]), 17240)
    assert out.stdout.splitlines() == [want] and "+" in want.split()[5]


# ---- the struct, the exports, the command line
def test_the_struct_and_the_exports(tmp_path):
    D = track.TRACK_DTYPE
    assert D.itemsize == 40 and api.TRACK_DTYPE is D
    offs = [("stream", 0), ("flags", 4), ("start_sample", 8), ("n_samples", 16), ("thresh", 20), ("bit_offset", 24), ("last_over", 32),
            ("n_ones", 36)]
    assert [(f, D.fields[f][1]) for f in D.names] == offs
    src = tmp_path / "track.c"
    src.write_text('#include <stddef.h>\n#include "tfrec_amd.h"\n'
                   "_Static_assert(sizeof(tfrec_amd_track) == 40, \"size\");\n" +
                   "".join("_Static_assert(offsetof(tfrec_amd_track, %s) == %d, \"%s\");\n" % (f, o, f) for f, o in offs) +
                   "_Static_assert(offsetof(tfrec_amd_run, pool_offset) == offsetof(tfrec_amd_track, bit_offset), \"the entry's\");\n")
    subprocess.check_call(["cc", "-std=c11", "-fsyntax-only", "-I", os.path.join(parity.ROOT, "include"), str(src)])
    names = ("tfrec_amd_enable_burst_track", "tfrec_amd_set_burst_track_centre", "tfrec_amd_read_burst_tracks")
    L = api.load_library()
    for sym in names:
        assert sym in api.EXPORTS
        getattr(L, sym)
    # no GPU is needed to be refused
    assert L.tfrec_amd_enable_burst_track(None, 5) == api.E_INVAL
    assert L.tfrec_amd_set_burst_track_centre(None, None, None, 0) == api.E_INVAL
    n, w = C.c_uint32(7), C.c_uint64(9)
    assert L.tfrec_amd_read_burst_tracks(None, None, 0, C.byref(n), None, 0, C.byref(w)) == api.E_INVAL and (n.value, w.value) == (7, 9)
    # the memory sums: the records, the bitmap and the centre indices per FIFO set; 68 bytes per stream; the indices' source
    assert track.device_bytes(3, 10, 65) == api.FIFO_DEPTH * (400 + 12 + 12) + 3 * 68 and track.pinned_bytes(3) == api.FIFO_DEPTH * 12
    assert [track.smooth_of(r) for r in (1000, 6000, 9600, 17240, 38400, 96000)] == [16, 16, 16, 11, 5, 2]


def test_cli_track_usage_errors(tmp_path):
    parity.build_cli()
    f = str(tmp_path / "missing.iq")

    for args in (["-G", "17240", "-X", f], ["-G", "17240", "-s", "50", "-L", f], ["-G", "17240", "-A", "-L", f]):
        out = parity.run_cli(args)
        assert out.returncode == 1 and "-G reads" in out.stderr, args
    out = parity.run_cli(["-M", "-G", "17240", "-X", f])  # -M's own refusal comes first and is what it was
    assert out.returncode == 1 and "-M measures" in out.stderr
    for bad in ("999", "96001", "abc", "17240,192001", "17240,-192001", "17240,", ",5"):
        out = parity.run_cli(["-G", bad, "-L", f])
        assert out.returncode == 1 and "bad -G" in out.stderr, bad
    out = parity.run_cli(["-h"])
    assert "-G r[,c]" in out.stderr and "[-G rate[,centre_hz]]" in out.stderr
    for args in (["-G", "17240", "-k", str(tmp_path / "keep"), "-L", f], ["-G", "17240", "-K", str(tmp_path / "keep"), "-L", f]):
        out = parity.run_cli(args)
        assert out.returncode == 2 and "not with -G" in out.stderr, args
    for args in (["-G", "17240", "-L", f], ["-G", "96000,-192000", "-L", f], ["-G", "1000,192000", "-M", "-Q", "-C", "-L", f],
                 ["-G", "17240", "-S", str(tmp_path / "cap"), "-n", "1", "-L", f], ["-G", "17240", "-d", "0", "-L", f]):
        out = parity.run_cli(args)  # accepted: the file is looked for
        assert out.returncode == 2 and "missing.iq" in out.stderr, args
    out = parity.run_cli(["-G", "17240", "-R", str(tmp_path / "nothing")])  # accepted with -R: the capture is looked for
    assert out.returncode == 2 and "-R replays" not in out.stderr
