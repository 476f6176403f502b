"""The burst sync without a GPU (tfrec_amd_enable_burst_sync, tfrec_gpu -G -Y): the restatement tfrec_amd/sync.py
against its per-sample form, the plateaus and payloads of the golden scenes (also rotated, about the matching centre; with a longer
word; with more errors allowed; the scenes that do not slice), the complemented word, delta at its limits, the first defined
sample, the behaviour under cutting -- every block cut, and pieces of 1000, 500 and the rest, which need the carried history
combined --, tfrec_gpu's merge, framing and line (tfrec_amd/host/job.h, compiled into a stand-alone program under the address and
undefined-behaviour sanitizers), the struct and the exports, and what tfrec_gpu decides before it opens a device.

Everything is exact integers: there is no tolerance anywhere.  Nothing here is measured on real recordings."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import parity
from recorder_rows import (GOLDEN, PAYLOADS, PLATEAUS, RATE, WORD, frame_symbols, golden_dec, rotated, submits, word_bits,
                           sync_stripped as stripped)
from tfrec_amd import api, capture, levels, sync, track
from meter_rows import crafted_dec

B = levels.BLOCK_DEC
CONT, OPEN = capture.RUN_CONTINUES, capture.RUN_OPEN


def sync_submits(tsubs, st, brute=False, n_streams=1):
    """Track submits [(records, words)] -> the sync's [(records, words)], the state carried from one to the next."""
    state, out = None, []
    for recs, words in tsubs:
        r, w, state = (sync.syncs_bruteforce if brute else sync.syncs)(recs, words, st, state, n_streams)
        out.append((r, w))
    return out


@functools.lru_cache(maxsize=None)
def golden_tracks(name, hz=0):
    dec = golden_dec(name) if hz == 0 else rotated(golden_dec(name), hz)
    return submits(dec, (len(dec) // (2 * B),), track.smooth_of(RATE[name]), hz)


def golden(name, st, hz=0):
    """-> [(the merged track piece, the merged sync piece)] of the scene's bursts."""
    tsubs = golden_tracks(name, hz)
    return list(zip(track.chains(tsubs), sync.chains(sync_submits(tsubs, st))))


def same(a, b):
    (ra, wa, sa), (rb, wb, sb) = a, b
    assert ra.dtype == rb.dtype == sync.SYNC_DTYPE and ra.tobytes() == rb.tobytes()
    assert wa.dtype == wb.dtype == np.dtype("<u4") and wa.tobytes() == wb.tobytes()
    assert len(sa["bits"]) == len(sb["bits"]) and all(np.array_equal(x, y) for x, y in zip(sa["bits"], sb["bits"]))


def hand_track(bits, flags=0, offset=0, stream=0, start=0, last_over=None):
    """A track record and bitmap by hand: the track `bits` at bit `offset`."""
    bits = np.asarray(bits, dtype=np.uint8)
    r = np.zeros(1, dtype=track.TRACK_DTYPE)
    r["stream"], r["flags"], r["start_sample"], r["n_samples"], r["thresh"] = stream, flags, start, len(bits), 500
    r["bit_offset"], r["n_ones"] = offset, int(bits.sum())
    r["last_over"] = len(bits) - 1 if last_over is None else last_over
    flat = np.zeros((offset + len(bits) + 31) // 32 * 32, dtype=np.uint8)
    flat[offset:offset + len(bits)] = bits
    return r, np.packbits(flat.reshape(-1, 32), axis=1, bitorder="little").view("<u4").reshape(-1)


def symbols_track(symbols, rate, lead=0):
    """An ideal track: symbol i holds from floor(384000 i / rate) on, behind `lead` zeros."""
    n = -(-384000 * len(symbols) // rate)
    idx = np.minimum(np.arange(n) * rate // 384000, len(symbols) - 1)
    return np.concatenate([np.zeros(lead, dtype=np.uint8), np.asarray(symbols, dtype=np.uint8)[idx]])


# ---- the restatement against its per-sample form
def test_the_vectorised_form_equals_the_per_sample_one_on_crafted_samples():
    dec, _ = crafted_dec(max(levels.windows(0x2F)), 0x2F)
    tsubs = submits(dec.reshape(-1), (len(dec.reshape(-1)) // (2 * B),), 5)
    assert len(tsubs[0][0]) >= 1
    for args in ((38400, 0xA5, 8, 0), (38400, 0xA5, 8, 3, True), (17240, WORD, 16, 2), (96000, 0x123456789ABCDEF0, 64, 20, True)):
        st = sync.Settings(*args)
        same(sync.syncs(*tsubs[0], st), sync.syncs_bruteforce(*tsubs[0], st))
    # tracks by hand: neighbours that share a word, a state to continue from, a run that does not fit the pool
    rng = np.random.default_rng(3)
    t = rng.integers(0, 2, 900).astype(np.uint8)
    recs = np.concatenate([hand_track(t[:37], CONT, 0)[0], hand_track(t[37:38], 0, 37, start=40)[0], hand_track(t[38:500], 0, 38, start=41)[0],
                           hand_track(t[500:], OPEN, 500, start=5000)[0]])
    words = hand_track(t)[1]
    st = sync.Settings(38400, 0x5A, 8, 1, True)
    state = {"bits": [rng.integers(0, 2, 300).astype(np.uint8)]}
    a = sync.syncs(recs, words, st, state)
    same(a, sync.syncs_bruteforce(recs, words, st, state))
    assert a[0]["best"][1] == sync.NONE and a[0]["best"][0] != sync.NONE and len(a[2]["bits"][0]) == 400
    b = sync.syncs(recs, words, st, state, max_samples=600)  # the last run does not fit: no bits, no history behind it
    same(b, sync.syncs_bruteforce(recs, words, st, state, max_samples=600))
    assert b[0]["best"][3] == sync.NONE and b[0]["n_hits"][3] == 0 and len(b[2]["bits"][0]) == 0 and len(b[1]) == 16
    assert b[0][:3].tobytes() == a[0][:3].tobytes() and a[0]["best"][3] != sync.NONE


@pytest.mark.parametrize("name", GOLDEN)
def test_the_vectorised_form_equals_the_per_sample_one_on_the_golden_scenes(name):
    st = sync.Settings(RATE[name], WORD, 16, 2, name in ("tfa_1", "whb"))
    tsubs = golden_tracks(name)
    fast, slow = sync_submits(tsubs, st), sync_submits(tsubs, st, brute=True)
    assert len(fast[0][0]) >= 1
    assert fast[0][0].tobytes() == slow[0][0].tobytes() and fast[0][1].tobytes() == slow[0][1].tobytes()


# ---- what DESIGN.md 6u's table states
@pytest.mark.parametrize("hz", [0, 20000])
@pytest.mark.parametrize("E", [0, 1])
def test_the_golden_plateaus_and_payloads(hz, E):
    for name in PLATEAUS:
        got = golden(name, sync.Settings(RATE[name], WORD, 16, E), hz)
        assert len(got) == 2
        for run, (t, s) in enumerate(got):
            want = PLATEAUS[name][run]
            if (name, run, hz) == ("tx22", 1, 20000):
                want = (1359, 1398)  # the only change under the rotation
            assert sync.plateaus(s.bits) == [want], (name, run)
            fr = sync.frames(t, s, sync.Settings(RATE[name], WORD, 16, E), 4)
            assert len(fr) == 1 and fr[0][0] == (want[0] + want[1]) >> 1 and fr[0][1:3] == (0, "+")
            assert track.hex_of(fr[0][3]) == PAYLOADS[name][run] and len(fr[0][3]) == 32
            assert int(s["n_hits"]) == want[1] - want[0] + 1 and (int(s["best"]), int(s["best_at"])) == (0, want[0])
    a, b = golden("tfa_2", sync.Settings(17240, WORD, 16, E), hz)
    st = sync.Settings(17240, WORD, 16, E)
    assert sync.line("f.iq", a[1], sync.frames(a[0], a[1], st, 4)[0]) == "frame f.iq 10003 10533 0 + 32 96070960"
    assert sync.line("f.iq", b[1], sync.frames(b[0], b[1], st, 4)[0]) == "frame f.iq 25583 26113 0 + 32 98812225"


def test_a_longer_word_gives_tfa_2_the_same_plateaus():
    for E in (0, 1):
        st = sync.Settings(17240, 0xAA2DD4, 24, E)
        got = golden("tfa_2", st)
        assert [sync.plateaus(s.bits) for _, s in got] == [[p] for p in PLATEAUS["tfa_2"]]
        assert [track.hex_of(sync.frames(t, s, st, 4)[0][3]) for t, s in got] == list(PAYLOADS["tfa_2"])


def test_false_plateaus_in_the_noise_tail_are_in_m_and_not_in_the_frames():
    st = sync.Settings(9600, WORD, 16, 2)
    t, s = golden("tfa_3", st)[1]
    assert sync.plateaus(s.bits) == [(1570, 1609), (3707, 3708), (3721, 3724)] and int(t["last_over"]) == 3283
    fr = sync.frames(t, s, st, 4)
    assert [f[0] for f in fr] == [1589] and track.hex_of(fr[0][3]) == "96846244"
    assert int(s["n_hits"]) == 40 + 2 + 4


def test_the_scenes_that_do_not_slice_give_no_frame():
    for name in ("tfa_1", "whb"):
        for E in (0, 1):
            st = sync.Settings(RATE[name], WORD, 16, E)
            for t, s in golden(name, st):
                assert not s.bits.any() and sync.frames(t, s, st) == [] and int(s["best"]) >= 2


def test_both_finds_the_complemented_word_with_the_complemented_payload():
    for name in PLATEAUS:
        st = sync.Settings(RATE[name], WORD ^ 0xFFFF, 16, 0, both=True)  # (E = 1 adds matches of either polarity in the noise tails)
        one = sync.Settings(RATE[name], WORD ^ 0xFFFF, 16, 0)
        for run, (t, s) in enumerate(golden(name, st)):
            assert sync.plateaus(s.bits) == [PLATEAUS[name][run]]
            fr = sync.frames(t, s, st, 4)
            assert len(fr) == 1 and fr[0][1:3] == (0, "-") and track.hex_of(fr[0][3]) == "%08x" % (int(PAYLOADS[name][run], 16) ^ 0xFFFFFFFF)
            assert (int(s["best"]), int(s["best_at"])) == (0, PLATEAUS[name][run][0])
        assert all(not s.bits.any() and int(s["best"]) >= 1 for _, s in golden(name, one))  # without BOTH: nothing


# ---- delta and the first defined sample
def test_deltas_at_the_limits():
    assert sync.deltas(17240, 4) == [0, 22, 45, 67] and sync.deltas(96000, 3) == [0, 4, 8] and sync.deltas(1000, 3) == [0, 384, 768]
    assert sync.Settings(4315, 0xAA2DD4, 24).span == 2047  # (768000 * 23 + 4315) // 8630
    with pytest.raises(ValueError):
        sync.Settings(4315, 0x1AA2DD4, 25)  # 2136 samples
    assert sync.Settings(12000, 0, 64).span == 2016 and sync.Settings(96000, 0, 64).span == 252
    for bad in ((999, 0, 8), (96001, 0, 8), (17240, 0, 7), (17240, 0, 65), (17240, 0, 16, 8), (17240, 0, 16, -1), (17240, 0, 9, 5)):
        with pytest.raises(ValueError):
            sync.Settings(*bad)
    assert sync.Settings(17240, 0, 16, 7).E == 7 and sync.Settings(17240, 0, 9, 4).E == 4
    assert sync.Settings(17240, 0x12DD4, 16).pattern == 0x2DD4  # the low P bits


def test_the_first_defined_sample():
    """k + H = span - 1 gives no bit, k + H = span may: an ideal track that is the word from its first sample on."""
    rate = 17240
    st = sync.Settings(rate, WORD, 16)
    t = symbols_track(word_bits(WORD, 16) + [0, 1] * 4, rate)[11:]  # (half of the first symbol: sample 334 is the last one's centre)
    recs, words = hand_track(t)
    r, w, _ = sync.syncs(recs, words, st)
    m = sync.bits_of(r[0], w)
    assert st.span == 334 and not m[:334].any() and m[334] == 1 and int(r[0]["best_at"]) == 334
    # the same track with its first h samples carried: defined from span - h on
    for h in (1, 100, 333, 334, 335):
        recs2, words2 = hand_track(t[h:], CONT)
        got = sync.syncs(recs2, words2, st, {"bits": [t[:h]]})
        same(got, sync.syncs_bruteforce(recs2, words2, st, {"bits": [t[:h]]}))
        m2 = sync.bits_of(got[0][0], got[1])
        assert np.array_equal(m2, m[h:]) and (h > 334 or (not m2[:334 - h].any() and m2[334 - h] == 1))
    short = sync.syncs(*hand_track(t[:334]), st)  # a run shorter than the span: nothing is defined
    assert short[0][0]["best"] == sync.NONE and short[0][0]["best_at"] == 0 and short[0][0]["n_hits"] == 0


# ---- cutting
@pytest.mark.parametrize("name,drop", [("tfa_2", 0), ("tfa_3", 0), ("tfa_2", 2000), ("tfa_3", 3000)])
def test_the_merged_chains_are_the_uncut_stream_for_every_block_cut(name, drop):
    """The scenes as they are -- their bursts lie inside blocks --, and with their first `drop` samples taken away, so that the first
    burst's sync word lies across a block boundary."""
    dec = golden_dec(name)[2 * drop:]
    dec = dec[:2 * B * min(8, len(dec) // (2 * B))]
    nb = len(dec) // (2 * B)
    L = track.smooth_of(RATE[name])
    st = sync.Settings(RATE[name], WORD, 16, 2)
    key = lambda c: (int(c["stream"]), int(c["start_sample"]))  # noqa: E731
    whole = sorted(sync.chains(sync_submits(submits(dec, (nb,), L), st)), key=key)
    assert len(whole) >= 2 and any(c.bits.any() for c in whole)
    cuts = 0
    for sizes in [(1,) * nb] + [(k, nb - k) for k in range(1, nb)]:
        tsubs = submits(dec, sizes, L)
        cuts += sum(1 for recs, _ in tsubs for r in recs if r["flags"] & CONT)
        got = sorted(sync.chains(sync_submits(tsubs, st)), key=key)
        assert len(got) == len(whole)
        for a, b in zip(got, whole):
            assert stripped(a.rec) == stripped(b.rec) and np.array_equal(a.bits, b.bits), (sizes, key(a))
    assert (cuts >= 1) == (drop > 0)
    if drop:  # ... and the cut lies inside the word: the plateau's first sample needs track bits of the block before
        first = whole[0]
        at = int(first["start_sample"]) + sync.plateaus(first.bits)[0][0]
        assert int(first["start_sample"]) < B and at - st.span < B <= at


def pieces_of(t, sizes, start=7000):
    """A track cut into pieces of `sizes` samples (the last takes the rest), one submit each."""
    out, pos = [], 0
    sizes = list(sizes) + [len(t) - sum(sizes)]
    for i, n in enumerate(sizes):
        flags = (CONT if i else 0) | (OPEN if i + 1 < len(sizes) else 0)
        out.append(hand_track(t[pos:pos + n], flags, offset=5 * i, start=start + pos))
        pos += n
    return out


@pytest.mark.parametrize("args", [(17240, WORD, 16, 0), (4315, 0xAA2DD4, 24, 1), (12000, 0x5A0FF0A5C3963C69, 64, 3, True)])
def test_pieces_of_1000_500_and_the_rest_need_the_combined_history(args):
    st = sync.Settings(*args)
    symbols = [i & 1 for i in range(6000 * st.rate // 384000 + st.P)]
    ends = [1150, 1650, 4000] if st.span < 450 else [2300, 5000]  # the samples near which a word ends: across a cut, or across both
    for e in ends:
        i = e * st.rate // 384000
        symbols[i - st.P + 1:i + 1] = word_bits(st.pattern, st.P)
    t = symbols_track(symbols, st.rate)
    whole = sync.chains(sync_submits([hand_track(t, start=7000)], st))[0]
    for e in ends:
        hit = np.flatnonzero(whole.bits[e - 60:e + 60]) + e - 60
        assert len(hit) and (e > 3000 or any(k - st.span < cut <= k for k in hit for cut in (1000, 1500)))
    for sizes in ((1000, 500), (1000, 500, 40, 1, 700), (3, 2047), (2048,)):
        subs = sync_submits(pieces_of(t, sizes), st)
        slow = sync_submits(pieces_of(t, sizes), st, brute=True)
        assert all(a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() for a, b in zip(subs, slow))
        got = sync.chains(subs)
        assert len(got) == 1 and np.array_equal(got[0].bits, whole.bits), sizes
        want = stripped(whole.rec)
        assert stripped(got[0].rec) == want
    # without the history every piece's first span samples are undefined: the carry matters
    alone = [sync.syncs(*p, st)[:2] for p in pieces_of(t, (1000, 500))]
    assert sum(int(r[0]["n_hits"]) for r, _ in alone) < int(whole["n_hits"])


def test_merge_takes_the_smaller_best_and_on_a_tie_the_earlier_piece():
    p = np.zeros(3, dtype=sync.SYNC_DTYPE)
    p["flags"], p["n_samples"], p["n_hits"] = (OPEN, CONT | OPEN, CONT), (5, 8, 3), (0, 2, 1)
    p["best"], p["best_at"] = (sync.NONE, 1, 1), (0, 6, 2)
    p["start_sample"], p["thresh"], p["bit_offset"] = (3192, 8192, 16384), (500, 600, 700), (64, 0, 0)
    bits = [np.array(b, dtype=np.uint8) for b in ([0] * 5, [0, 0, 0, 0, 0, 0, 1, 1], [0, 0, 1])]
    m = sync.merge([sync.Piece(r, b) for r, b in zip(p, bits)])
    assert [int(m[f]) for f in sync.SYNC_DTYPE.names] == [0, 0, 3192, 16, 500, 64, 3, 1, 11, 0]
    assert m.bits.tolist() == sum((b.tolist() for b in bits), [])
    p["best"], p["best_at"] = (2, 1, 0), (4, 6, 2)
    assert [int(sync.merge([sync.Piece(r, b) for r, b in zip(p, bits)])[f]) for f in ("best", "best_at")] == [0, 15]
    assert sync.merge([sync.Piece(p[0], bits[0]), sync.Piece(p[1], bits[1])])["flags"] == OPEN


# ---- tfrec_gpu's merge, framing and line: job.h in a stand-alone program
@pytest.fixture(scope="module")
def merge_driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sync_merge") / "sync_merge_driver")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(parity.ROOT, "tests", "merge_driver.cpp")])
    return exe


def batch_lines(nb, slots, trecs, twords, srecs, swords, f, keep=None):
    out = ["batch %d %s" % (nb, " ".join("%d" % s for s in slots)), "words " + " ".join("%x" % w for w in twords),
           "match " + " ".join("%x" % w for w in swords)]
    for i, (r, s) in enumerate(zip(trecs, srecs)):
        v = [f] + [int(r[k]) for k in ("flags", "start_sample", "n_samples", "thresh", "bit_offset", "last_over", "n_ones")]
        v += [int(s[k]) for k in ("n_hits", "best", "best_at")]
        out.append("rec " + " ".join("%d" % x for x in v + [int(r["n_samples"]) if keep is None else keep[i]]))
    return out


def expected_lines(name, tsubs, ssubs, st, n_bytes):
    want = []
    for t, s in zip(track.chains(tsubs), sync.chains(ssubs)):
        want.append(track.line(name, t, st.rate))
        want.append("sync %s %d %d %d %d %d %d" % ((name,) + tuple(int(s[k]) for k in ("start_sample", "n_samples", "flags", "n_hits", "best", "best_at"))))
        want += [sync.line(name, s, f) for f in sync.frames(t, s, st, n_bytes)]
    return want


def run_driver(exe, st, n_bytes, lines):
    head = ["sync %d %x %d %d %d %d" % (st.rate, st.pattern, st.P, st.E, n_bytes, st.both)]
    out = subprocess.run([exe, "sync"], input="".join(ln + "\n" for ln in head + lines), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    return out.stdout.splitlines()


def test_the_host_merge_prints_the_restatements_lines(merge_driver):
    """The golden TFA_2 scene in batches of 1 block (E = 0, 4 bytes) beside a file of hand-made tracks: a chain cut in three whose
    plateau straddles a cut, a frame whose payload the burst's end cuts, a match behind last_over, and the complemented word."""
    st = sync.Settings(17240, WORD, 16, 0, both=True)
    dec = golden_dec("tfa_2")[:2 * 4 * B]
    tsubs = submits(dec, (1,) * 4, 11)
    ssubs = sync_submits(tsubs, st)
    lines = ["file b.iq 4", "file c.iq 4096"]
    for (tr, tw), (sr, sw) in zip(tsubs, ssubs):
        lines += batch_lines(1, [0], tr, tw, sr, sw, 0)
    want = expected_lines("b.iq", tsubs, ssubs, st, 4)
    assert [w for w in want if w.startswith("frame")] == ["frame b.iq 10003 10533 0 + 32 96070960", "frame b.iq 25583 26113 0 + 32 98812225"]
    inv = symbols_track(frame_symbols(WORD, 16, 5, pre=8, pay=40, invert=True) + frame_symbols(WORD, 16, 6, pre=8, pay=12), 17240, lead=50)
    plain = sync.chains(sync_submits([hand_track(inv)], st))[0]
    a, b = sync.plateaus(plain.bits)[0]
    cut = (a + b) // 2  # the first plateau straddles the first cut
    pieces = pieces_of(inv, (cut, 700), start=8192 * 3 - cut)
    hs = sync_submits(pieces, st)
    for k, ((tr, tw), (sr, sw)) in enumerate(zip(pieces, hs)):
        lines += batch_lines(1, [1], tr, tw, sr, sw, 1)
    hw = expected_lines("c.iq", pieces, hs, st, 4)
    frames = [w.split() for w in hw if w.startswith("frame")]
    assert [f[5] for f in frames] == ["-", "+"] and frames[0][6] == "32" and 0 < int(frames[1][6]) < 32  # the second payload is cut
    want += hw
    t2, w2 = hand_track(inv, start=8192 * 9, last_over=b + 30)  # the burst ends ahead of the second plateau: one frame, a short payload
    s2 = sync.syncs(t2, w2, st)
    lines += batch_lines(1, [1], t2, w2, s2[0], s2[1], 1)
    h2 = expected_lines("c.iq", [(t2, w2)], [(s2[0], s2[1])], st, 4)
    assert len([w for w in h2 if w.startswith("frame")]) == 1 and h2[-1].split()[6] == "1"
    want += h2
    assert run_driver(merge_driver, st, 4, lines) == want


def test_the_host_cuts_a_piece_at_its_files_end(merge_driver):
    st = sync.Settings(17240, WORD, 16, 1)
    t = symbols_track(frame_symbols(WORD, 16, 7, pre=8, pay=40), 17240, lead=20)
    tr, tw = hand_track(t, start=8192 * 2 - 700)
    s = sync.syncs(tr, tw, st)
    assert s[0][0]["n_hits"] > 0
    lines = ["file a.iq 2"] + batch_lines(2, [0], tr, tw, s[0], s[1], 0, keep=[700])
    kept = hand_track(t[:700], OPEN, start=8192 * 2 - 700)
    ks = sync.syncs(*kept, st)
    want = expected_lines("a.iq", [kept], [(ks[0], ks[1])], st, 8)
    assert run_driver(merge_driver, st, 8, lines) == want and any(w.startswith("frame") for w in want)


# ---- the struct, the exports, the command line
def test_the_struct_and_the_exports(tmp_path):
    D = sync.SYNC_DTYPE
    assert D.itemsize == 48 and api.SYNC_DTYPE is D
    offs = [("stream", 0), ("flags", 4), ("start_sample", 8), ("n_samples", 16), ("thresh", 20), ("bit_offset", 24), ("n_hits", 32),
            ("best", 36), ("best_at", 40), ("reserved", 44)]
    assert [(f, D.fields[f][1]) for f in D.names] == offs
    src = tmp_path / "sync.c"
    src.write_text('#include <stddef.h>\n#include "tfrec_amd.h"\n'
                   "_Static_assert(sizeof(tfrec_amd_burst_sync) == 48, \"size\");\n" +
                   "".join("_Static_assert(offsetof(tfrec_amd_burst_sync, %s) == %d, \"%s\");\n" % (f, o, f) for f, o in offs) +
                   "_Static_assert(TFREC_AMD_SYNC_BOTH == %d, \"flag\");\n" % sync.BOTH)
    subprocess.check_call(["cc", "-std=c11", "-fsyntax-only", "-I", os.path.join(parity.ROOT, "include"), str(src)])
    L = api.load_library()
    for sym in ("tfrec_amd_enable_burst_sync", "tfrec_amd_read_burst_syncs"):
        assert sym in api.EXPORTS
        getattr(L, sym)
    # no GPU is needed to be refused
    assert L.tfrec_amd_enable_burst_sync(None, 17240, WORD, 16, 0, 0) == api.E_INVAL
    n, w = C.c_uint32(7), C.c_uint64(9)
    assert L.tfrec_amd_read_burst_syncs(None, None, 0, C.byref(n), None, 0, C.byref(w)) == api.E_INVAL and (n.value, w.value) == (7, 9)
    # the memory sums: the records and the bitmap per FIFO set; 260 bytes per stream; nothing page-locked
    assert sync.device_bytes(3, 10, 65) == api.FIFO_DEPTH * (480 + 12) + 3 * 260 and sync.pinned_bytes(3) == 0


def test_cli_sync_usage_errors(tmp_path):
    parity.build_cli()
    f = str(tmp_path / "missing.iq")

    out = parity.run_cli(["-Y", "2dd4", "-L", f])
    assert out.returncode == 1 and "-Y finds" in out.stderr  # without -G
    for bad in ("2", "2dd4a5920189acdb0", "2dx4", "", "2dd4,8", "2dd4,-1", "2dd4,0,0", "2dd4,0,257", "2dd4,0,4,2", "2dd4,0,4,1,0", "2dd4,"):
        out = parity.run_cli(["-G", "17240", "-Y", bad, "-L", f])
        assert out.returncode == 1 and "bad -Y" in out.stderr, bad
    out = parity.run_cli(["-G", "4315", "-Y", "1aa2dd4", "-L", f])  # 28 bits at 4315 bit/s: 2403 samples
    assert out.returncode == 1 and "more than 2047" in out.stderr
    for args in (["-X", f], ["-s", "50", "-L", f], ["-A", "-L", f]):
        out = parity.run_cli(["-G", "17240", "-Y", "2dd4"] + args)
        assert out.returncode == 1 and "-G reads" in out.stderr, args
    for k in ("-k", "-K"):
        out = parity.run_cli(["-G", "17240", "-Y", "2dd4", k, str(tmp_path / "keep"), "-L", f])
        assert out.returncode == 2 and "not with -G" in out.stderr
    out = parity.run_cli(["-h"])
    assert "-Y h[,e[,n[,b]]]" in out.stderr and "[-Y hex[,errors[,bytes[,both]]]]" in out.stderr
    for args in (["-G", "17240", "-Y", "2dd4"], ["-G", "17240", "-Y", "2DD4,7,256,1"], ["-G", "4315", "-Y", "aa2dd4,11"],
                 ["-G", "96000", "-Y", "0123456789abcdef,31,1,0", "-M", "-Q", "-C"], ["-Y", "d4,3", "-G", "17240,20000"]):
        out = parity.run_cli(args + ["-L", f])  # accepted: the file is looked for
        assert out.returncode == 2 and "missing.iq" in out.stderr, args
