"""The frame check without a GPU (tfrec_amd_enable_burst_crc, tfrec_gpu -G -Y -V): the restatement tfrec_amd/crc.py
against its per-sample form on crafted tracks and the golden scenes, the figures the feature was specified with -- every golden
frame's verdict at v[c + D], TX22's two lengths both ways, WHB's n_ok and first_at --, frames planted by construction and one
flipped payload bit, LSB against MSB, INVERT and skip, the first defined sample, the behaviour under cutting -- every block cut of
the golden WHB and TFA_2 scenes, pieces of 1000, 500 and the rest, a first piece of 3 samples behind a stale history --, merge's
first_at, the table builder (tfrec_amd/csrc/crc_table.h) and tfrec_gpu's host code (tfrec_amd/host/job.h), compiled into a
stand-alone program under the address and undefined-behaviour sanitizers, the declarations the C header makes, the exports, the
memory sums and what tfrec_gpu decides before it opens a device.

Everything is exact integers: there is no tolerance anywhere.  Nothing here is measured on real recordings."""
import ctypes as C
import functools
import itertools
import os
import subprocess

import numpy as np
import pytest

import crc_rows as CR
import linecode_rows as LR
import parity
from linecode_rows import CONT, OPEN, hand_track, pieces_of
from recorder_rows import RATE, golden_dec
from tfrec_amd import api, crc, sync, track

B = api.BLOCK_DEC
FIELDS = [f for f in crc.CRC_DTYPE.names if f != "bit_offset"]  # (a piece's place in its own submit's pool)


def stripped(rec):
    return [int(rec[f]) for f in FIELDS]


def both(trecs, twords, st, state=None, n_streams=1, max_samples=None):
    """The vectorised form's records, words and state, held to the per-sample one's."""
    a = crc.crcs(trecs, twords, st, state, n_streams, max_samples)
    b = crc.crcs_bruteforce(trecs, twords, st, state, n_streams, max_samples)
    assert a[0].dtype == b[0].dtype == crc.CRC_DTYPE and a[0].tobytes() == b[0].tobytes()
    assert a[1].dtype == b[1].dtype == np.dtype("<u4") and a[1].tobytes() == b[1].tobytes()
    assert len(a[2]["bits"]) == len(b[2]["bits"]) and all(np.array_equal(x, y) for x, y in zip(a[2]["bits"], b[2]["bits"]))
    for f in ("stream", "flags", "start_sample", "n_samples", "thresh", "bit_offset"):  # the entry's fields are the input record's
        assert np.array_equal(a[0][f], np.asarray(trecs)[f]), f
    for r in a[0]:  # the record's sums are the bitmap's
        v = crc.bits_of(r, a[1]) if crc._fits(r, max_samples) else np.zeros(0, dtype=np.uint8)
        ok = np.flatnonzero(v)
        assert int(r["n_ok"]) == len(ok) and int(r["first_at"]) == (int(ok[0]) if len(ok) else crc.NONE)
    return a


def both_submits(tsubs, st, n_streams=1):
    state, out = None, []
    for recs, words in tsubs:
        r, w, state = both(recs, words, st, state, n_streams)
        out.append((r, w))
    return out


def checked(bits, st, **kw):
    """The check track of one run that stands alone."""
    r, w, _ = both(*hand_track(bits, **kw), st)
    return crc.bits_of(r[0], w), r[0]


# ---- the settings and the table
def test_the_settings_limits_and_the_reach():
    assert {k: CR.settings(k).D for k in CR.SETS} == CR.REACH
    assert crc.delta(6001, 256) == 16381 and crc.delta(6000, 256) == 16384 and crc.HISTORY == 16383
    with pytest.raises(ValueError):
        crc.Settings(6000, 32, 8, 0x07)  # D = 16384
    # per N the lowest rate it is accepted at: D <= 16383 there and above it a bit/s below
    for N, rate in ((32, 6001), (64, 12001), (128, 24001), (256, 48002)):
        assert crc.Settings(rate, N, 8, 0x31).D <= 16383 < crc.delta(rate - 1, 8 * N), N
        with pytest.raises(ValueError):
            crc.Settings(rate - 1, N, 8, 0x31)
    assert crc.Settings(96000, 256, 32, 1, skip=251).D == 8192 and crc.Settings(1000, 5, 8, 1).D == 15360
    bad = [(999, 5, 8, 0x31), (96001, 5, 8, 0x31), (6000, 0, 8, 0x31), (48002, 257, 8, 0x31), (6000, 5, 12, 0x31), (6000, 5, 0, 0x31),
           (6000, 5, 40, 0x31), (6000, 5, 8, 0), (6000, 5, 8, 0x131), (6000, 5, 8, 0x31, 0x100), (6000, 5, 8, 0x31, 0, 0x100),
           (6000, 5, 8, 0x31, 0, 0, -1), (6000, 5, 8, 0x31, 0, 0, 4), (6000, 5, 32, 0x04C11DB7, 0, 0, 1), (6000, 1, 8, 0x31),
           (6000, 5, 16, 0x11021), (6000, 5, 32, 1 << 32), (6000, 5, 8, -1), (1000, 6, 8, 0x31)]
    for args in bad:
        with pytest.raises(ValueError):
            crc.Settings(*args)
    crc.Settings(6000, 5, 8, 0x31, 0, 0, 3)  # one covered byte
    crc.Settings(6000, 5, 32, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF)
    assert crc.Settings(6000, 5, 8, 0x31, lsb=True, invert=True).flags == crc.LSB | crc.INVERT == 3 and (crc.LSB, crc.INVERT) == (1, 2)


@pytest.mark.parametrize("name", list(CR.SETS))
def test_the_table_is_the_crcs_affine_form(name):
    """residue(b) = r0 ^ XOR of the columns of the set bits, on random frames; the skipped bytes have no term."""
    st = CR.settings(name)
    table = st.table()
    offs = [o for o, _ in table]
    covered = 8 * (st.N - st.S)
    assert len(table) == covered and offs == st.offs[8 * st.S:] and all(0 <= o < st.D for o in offs) and offs[-1] == 0
    assert all(0 < c < 1 << st.W for _, c in table)
    rng = np.random.default_rng(5)
    for k in range(20):
        frame = bytes(rng.integers(0, 256, st.N).tolist()) if k else CR.random_frame(st, 3)
        bits = CR.frame_bits(st, frame)  # as they stand on the track
        res = st.r0
        for b, (_, col) in zip(bits[8 * st.S:], table):
            res ^= col if b else 0
        assert (res == 0) == st.check(frame), k
    assert st.check(CR.random_frame(st, 3))


# ---- the restatement against its per-sample form
@pytest.mark.parametrize("name", ["crc8", "ccitt", "crc24"])
def test_the_two_forms_agree_on_crafted_tracks(name):
    st = CR.settings(name)
    rng = np.random.default_rng(3)
    t = np.concatenate([CR.planted(st, s)[0] for s in (1, 2)])[:3 * st.D + 1500]
    for sizes in ((), (1000, 500), (1, 1, 1), (st.D, 1), (st.D + 700,)):
        both_submits(pieces_of(t, sizes), st)
    # several runs in one submit, two streams, packed back to back off word boundaries -- neighbours that share a bitmap word --; a
    # state to continue from; a pool that does not hold the last run
    recs, off = [], 0
    for s, n, flags in ((0, 37, 0), (0, st.D + 230, 0), (0, 3, OPEN), (1, 100, CONT), (1, st.D + 600, OPEN)):
        recs.append(hand_track(np.zeros(n), flags, offset=off, stream=s, start=1000 * len(recs))[0])
        off += n
    recs = np.concatenate(recs)
    bits = np.resize(np.concatenate([t, rng.integers(0, 2, 40).astype(np.uint8)]), (off + 31) // 32 * 32)
    words = np.packbits(bits.reshape(-1, 32), axis=1, bitorder="little").view("<u4").reshape(-1)
    state = {"bits": [np.zeros(0, dtype=np.uint8), t[:st.D - 50].copy()]}
    a = both(recs, words, st, state, 2)
    assert [len(h) for h in a[2]["bits"]] == [3, min(crc.HISTORY, st.D + 600)]
    assert int(a[0][3]["n_samples"]) + st.D - 50 >= st.D  # stream 1's run of 100 has defined samples only through what it continues
    fresh = both(recs, words, st, None, 2)
    assert fresh[0][3]["n_ok"] == 0 and fresh[0][3]["first_at"] == crc.NONE  # without it: a run shorter than D has none
    cut = both(recs, words, st, state, 2, max_samples=off - 1)  # the last run does not fit: no bits, n_ok 0, no history
    assert cut[0][-1]["n_ok"] == 0 and cut[0][-1]["first_at"] == crc.NONE and cut[0][:-1].tobytes() == a[0][:-1].tobytes()
    assert [len(h) for h in cut[2]["bits"]] == [3, 0] and len(cut[1]) == (int(recs[-1]["bit_offset"]) + 31) // 32


@pytest.mark.parametrize("name", list(CR.GOLDEN))
def test_the_two_forms_agree_on_the_golden_scenes(name):
    """Uncut, but for the two scenes with the longest frames, which are cut once: the brute force is a Python loop per sample."""
    nb = len(golden_dec(name)) // (2 * B)
    for N, _, _ in CR.GOLDEN[name][3]:
        both_submits(CR.golden_tracks(name, (1, nb - 1) if name in ("whb", "tx22") else (nb,)), CR.golden_settings(name, N))


# ---- the figures the feature was specified with
@functools.lru_cache(maxsize=None)
def golden(name, N):
    """-> (the sync's settings, the check's, the merged input tracks, sync chains and check chains) of a golden scene, uncut."""
    _, word, lsb, _ = CR.GOLDEN[name]
    tsubs = CR.golden_tracks(name)
    sst = sync.Settings(RATE[name], word, 16, 0)
    st = CR.golden_settings(name, N)
    return sst, st, track.chains(tsubs), sync.chains(LR.sync_submits(tsubs, sst)), crc.chains(CR.crc_submits(tsubs, st))


@pytest.mark.parametrize("name", list(CR.GOLDEN))
def test_the_issues_table_figure_for_figure(name):
    _, word, lsb, rows = CR.GOLDEN[name]
    for N, centres, holds in rows:
        sst, st, tch, sch, vch = golden(name, N)
        assert st.D == CR.GOLDEN_D[(name, N)] and len(tch) == len(sch) == len(vch) == len(centres)
        for i, (t, s, v) in enumerate(zip(tch, sch, vch)):
            fr = sync.frames(t, s, sst, N, lsb=lsb)
            assert len(fr) == 1 and fr[0][:3] == (centres[i], 0, "+")
            verdict = crc.verdicts(fr, v, st)
            k = centres[i] + st.D
            if len(fr[0][3]) == 8 * N:  # all of the frame lies inside the burst
                assert sync.hex_of(fr[0][3], lsb).startswith(CR.GOLDEN_FRAMES[name][i][:2 * N]) and k <= int(t["last_over"])
                assert verdict == ["ok" if holds[i] else "bad"] and bool(v.bits[k]) == holds[i], (name, N, i)
                assert st.check(bytes.fromhex(sync.hex_of(fr[0][3], lsb))) == holds[i]
                if holds[i]:
                    assert sync.hex_of(fr[0][3], lsb) == CR.GOLDEN_FRAMES[name][i]
                    assert crc.line("f", v, st).split()[1:4] == ["f", str(int(v["start_sample"])), str(int(v["n_samples"]))]
            else:  # TX22's 7-byte telegram read as 9 bytes: the burst ends first, no verdict, and nothing there checks
                assert (name, N, i) == ("tx22", 9, 0) and not holds[i] and verdict == ["-"] and (k >= len(v.bits) or not v.bits[k])
    if name == "whb":
        v = vch[0]
        assert (int(v["n_ok"]), int(v["first_at"])) == (CR.WHB_N_OK, CR.WHB_FIRST_AT) and CR.WHB_FIRST_AT - st.D == LR.WHB_PLATEAU[0]
        assert np.flatnonzero(v.bits).tolist() == list(range(CR.WHB_FIRST_AT, CR.WHB_FIRST_AT + 64))  # the sync's plateau, D on
        assert crc.line("f", v, st) == "crc f 10004 28344 64 %d" % (10004 + LR.WHB_PLATEAU[0])
        assert sync.hex_of(fr[0][3], True) == LR.WHB_FRAME[:46]
    if name == "tfa_1":  # init 0, xorout 0: the burst's constant stretches check too
        assert all(1200 <= int(v["n_ok"]) <= 1400 and int(v["n_samples"]) == 4056 for v in vch)


# ---- frames planted by construction
@pytest.mark.parametrize("name", list(CR.SETS))
def test_a_planted_frame_checks_about_its_last_bits_centre_and_a_flipped_bit_does_not(name):
    st = CR.settings(name)
    spb = 384000 / st.rate
    for seed in (1, 2, 3):
        t, frame, c = CR.planted(st, seed)
        assert st.check(frame)
        form = checked if st.D < 4000 else (lambda bits, s: (lambda r: (crc.bits_of(r[0][0], r[1]), r[0][0]))(crc.crcs(*hand_track(bits), s)))
        v, rec = form(t, st)
        k = c + st.D
        got = CR.stretch(v, k)
        assert got is not None and got[0] <= k <= got[1], (name, seed)  # the symbol's centre is in it
        assert spb / 2 <= got[1] - got[0] + 1 <= spb + 1, (name, seed, got)  # ... and it is roughly a symbol wide
        assert int(rec["n_ok"]) >= got[1] - got[0] + 1 and int(rec["first_at"]) <= got[0] and v[:st.D].sum() == 0
        for flip in (1, 8 * st.S + 1, 8 * st.S + 3, 8 * (st.N - st.W // 8), 8 * (st.N - st.W // 8) + 1, 8 * st.N):
            w, _ = form(CR.planted(st, seed, flip=flip)[0], st)
            if flip <= 8 * st.S:  # a skipped byte is not covered
                assert np.array_equal(w[got[0]:got[1] + 1], v[got[0]:got[1] + 1]) and st.S
            else:  # one flipped payload bit: bad, at every sample of the stretch
                assert not w[got[0]:got[1] + 1].any(), (name, seed, flip)


def test_lsb_against_msb_invert_and_skip():
    base = dict(rate=38400, n_bytes=6, width=16, poly=0x1021, init=0x1D0F)
    plain = crc.Settings(**base)
    t, frame, c = CR.planted(plain, 7)
    k = c + plain.D
    v, _ = checked(t, plain)
    assert v[k]
    # the same symbols read LSB-first are other bytes: that frame does not check, its bit-reversed bytes' frame does
    lsb = crc.Settings(lsb=True, **base)
    assert not checked(t, lsb)[0][k] and not lsb.check(bytes(int("{:08b}".format(x)[::-1], 2) for x in frame))
    tl, fl, _ = CR.planted(lsb, 7)
    assert checked(tl, lsb)[0][k] and fl == frame and not np.array_equal(tl, t)  # the same bytes, other symbols
    # INVERT: the complemented track checks, the track itself does not
    inv = crc.Settings(invert=True, **base)
    assert np.array_equal(checked(1 - t, inv)[0], v) and not checked(t, inv)[0][k]
    assert np.array_equal(CR.planted(inv, 7)[0][10 * 40:10 * 88], 1 - t[10 * 40:10 * 88])
    # skip: a 7-byte frame whose first byte is anything
    skip = crc.Settings(38400, 7, 16, 0x1021, 0x1D0F, skip=1)
    for first in (0x00, 0xA5):
        bits = CR.frame_bits(skip, bytes([first]) + frame)
        sym = [0, 1] * 20 + bits + [1, 0] * 6
        ts = np.repeat(np.asarray(sym, dtype=np.uint8), 10)
        assert checked(ts, skip)[0][10 * 39 + 5 + skip.D] and skip.check(bytes([first]) + frame)
    assert not crc.Settings(38400, 7, 16, 0x1021, 0x1D0F).check(bytes([0xA5]) + frame)
    assert len(skip.table()) == 48 and len(crc.Settings(38400, 7, 16, 0x1021, 0x1D0F).table()) == 56


def test_the_first_defined_sample():
    st = CR.settings("ccitt")  # D = 320; INVERT, init ffff, xorout ffff
    t, frame, c = CR.planted(st, 4, pre=1)
    t, c = t[c:], 0  # the sync word's last symbol would have had its centre at the track's first sample
    v, rec = checked(t, st)
    assert v[:st.D].sum() == 0  # samples ahead of D are undefined and read 0 ...
    assert v[st.D] and int(rec["first_at"]) == st.D  # ... the first defined one checks: the frame is read from sample 0 on
    # behind a history of H samples the first defined sample is D - H
    r1, w1, state = both(*hand_track(t[:100], OPEN), st)
    assert r1[0]["n_ok"] == 0 and len(state["bits"][0]) == 100
    r2, w2, _ = both(*hand_track(t[100:], CONT, start=100), st, state)
    assert np.array_equal(crc.bits_of(r2[0], w2), v[100:]) and int(r2[0]["first_at"]) == st.D - 100
    # all zeros with init 0 and xorout 0: every defined sample checks
    z = crc.Settings(38400, 4, 8, 0x31)
    vz, rz = checked(np.zeros(1000, dtype=np.uint8), z)
    assert vz[:z.D].sum() == 0 and vz[z.D:].all() and (int(rz["n_ok"]), int(rz["first_at"])) == (1000 - z.D, z.D)
    assert checked(np.zeros(z.D, dtype=np.uint8), z)[1]["first_at"] == crc.NONE  # a run of D samples has none


# ---- cutting
def compositions(n):
    return [c for k in range(1, n + 1) for c in itertools.product(range(1, n + 1), repeat=k) if sum(c) == n]


@pytest.mark.parametrize("name", ["whb", "tfa_2"])
def test_every_block_cut_merges_to_the_uncut_result(name):
    N = CR.GOLDEN[name][3][0][0]
    st = CR.golden_settings(name, N)
    whole = golden(name, N)[4]
    nb = len(golden_dec(name)) // (2 * B)
    cuts = 0
    for sizes in compositions(nb):
        tsubs = CR.golden_tracks(name, sizes)
        cuts += sum(1 for recs, _ in tsubs for r in recs if r["flags"] & CONT)
        got = crc.chains(CR.crc_submits(tsubs, st))
        assert len(got) == len(whole)
        for a, b in zip(got, whole):
            assert stripped(a.rec) == stripped(b.rec) and np.array_equal(a.bits, b.bits), sizes
    assert (cuts >= 1) == (name == "whb")  # WHB's burst lies across block boundaries, and D = 11776 is above a block


@pytest.mark.parametrize("name", ["crc8", "whb", "ccitt", "crc24"])
def test_pieces_of_1000_500_and_the_rest_need_the_combined_history(name):
    st = CR.settings(name)
    t, frame, c = CR.planted(st, 9, pre=1200 * st.rate // 384000 + 1)  # the frame begins in the second piece and ends in the third
    k = c + st.D
    assert 1000 < c < 1500 < k
    one = crc.crcs if st.D > 4000 else both
    subs = lambda pieces: [one(r, w, st, s)[:2] for (r, w), s in zip(pieces, states(pieces, st))]  # noqa: E731
    whole = crc.chains([one(*hand_track(t, start=7000), st)[:2]])[0]
    assert whole.bits[k] and len(t) > k + 20
    for sizes in ((1000, 500), (1000, 500, 40, 1, 700), (3, k - 500), (k - 1,), (k, 1)):
        got = crc.chains(subs(pieces_of(t, sizes)))
        assert len(got) == 1 and np.array_equal(got[0].bits, whole.bits), sizes
        assert stripped(got[0].rec) == stripped(whole.rec)
    alone = [crc.crcs(*p, st)[:2] for p in pieces_of(t, (1000, 500))]  # without the history the frame is not seen: the carry matters
    assert not np.concatenate([crc.bits_of(r[0], w) for r, w in alone])[k]


def states(pieces, st):
    """The state ahead of every piece of a chain."""
    out, state = [], None
    for r, w in pieces:
        out.append(state)
        state = crc.crcs(r, w, st, state, 1)[2]
    return out


def test_a_first_piece_of_three_samples_behind_a_stale_history():
    """H = 3: nothing ahead of the chain is used, whatever the stream held before."""
    st = CR.settings("crc8")
    rng = np.random.default_rng(13)
    t, frame, c = CR.planted(st, 5)
    old = np.concatenate([rng.integers(0, 2, 20000).astype(np.uint8), t[-2000:]])  # an earlier chain that ends in frame-like bits
    whole, _ = checked(t, st)
    first = both(*hand_track(old, OPEN), st)
    assert len(first[2]["bits"][0]) == crc.HISTORY
    a = both(*hand_track(t[:3], OPEN, start=90000), st, first[2])  # a new chain: not CONTINUES, 3 samples, open
    assert len(a[2]["bits"][0]) == 3 and a[2]["bits"][0].tolist() == t[:3].tolist() and a[0][0]["n_ok"] == 0
    b = both(*hand_track(t[3:], CONT, start=90003), st, a[2])
    assert np.array_equal(np.concatenate([crc.bits_of(a[0][0], a[1]), crc.bits_of(b[0][0], b[1])]), whole)
    assert int(b[0][0]["first_at"]) >= st.D - 3
    # a piece that CONTINUES with no history left (the piece before did not fit the pool): a chain's first
    cc = both(*hand_track(t[3:], CONT, start=90003), st, crc.fresh_state(1))
    assert np.array_equal(crc.bits_of(cc[0][0], cc[1]), checked(t[3:], st)[0])


def test_merges_first_at_is_the_first_pieces_that_has_one():
    def piece(n, ok, flags):
        r = np.zeros((), dtype=crc.CRC_DTYPE)
        bits = np.zeros(n, dtype=np.uint8)
        bits[list(ok)] = 1
        r["flags"], r["n_samples"], r["n_ok"], r["first_at"], r["start_sample"] = flags, n, len(ok), min(ok, default=crc.NONE), 500
        return crc.Piece(r, bits)

    m = crc.merge([piece(100, [], OPEN), piece(50, [7, 9], CONT | OPEN), piece(30, [0], CONT)])
    assert (int(m["n_samples"]), int(m["n_ok"]), int(m["first_at"]), int(m["flags"])) == (180, 3, 107, 0)
    assert np.flatnonzero(m.bits).tolist() == [107, 109, 150]
    m = crc.merge([piece(100, [40], CONT | OPEN), piece(50, [7], CONT | OPEN)])
    assert (int(m["n_ok"]), int(m["first_at"]), int(m["flags"])) == (2, 40, CONT | OPEN)
    m = crc.merge([piece(100, [], OPEN), piece(50, [], CONT)])
    assert (int(m["n_ok"]), int(m["first_at"])) == (0, crc.NONE)
    st = CR.settings("crc8")
    assert crc.line("f", m, st) == "crc f 500 150 0 -"
    assert crc.line("f", crc.merge([piece(2000, [1000], 0)]), st) == "crc f 500 2000 1 %d" % (500 + 1000 - 891)
    # the verdict: polarity + and all 8 N bits
    v = piece(2000, [1000], 0)
    frames = [(1000 - 891, 0, "+", [0] * 40), (1001 - 891, 0, "+", [0] * 40), (1000 - 891, 0, "-", [0] * 40), (1000 - 891, 0, "+", [0] * 39)]
    assert crc.verdicts(frames, v, st) == ["ok", "bad", "-", "-"]


# ---- the declarations, the exports, the memory sums
def test_the_header_the_exports_and_the_memory_sums(tmp_path):
    src = tmp_path / "crc.c"
    src.write_text('#include <stddef.h>\n#include "tfrec_amd.h"\n'
                   "_Static_assert(sizeof(tfrec_amd_burst_crc) == 40 && offsetof(tfrec_amd_burst_crc, bit_offset) == 24 && "
                   "offsetof(tfrec_amd_burst_crc, n_ok) == 32 && offsetof(tfrec_amd_burst_crc, first_at) == 36, \"the record\");\n"
                   "_Static_assert(TFREC_AMD_CRC_LSB == %d && TFREC_AMD_CRC_INVERT == %d, \"flags\");\n" % (crc.LSB, crc.INVERT) +
                   "int (*enable)(tfrec_amd_ctx *, int32_t, int32_t, int32_t, int32_t, uint32_t, uint32_t, uint32_t, uint32_t) = tfrec_amd_enable_burst_crc;\n"
                   "int (*read)(tfrec_amd_ctx *, tfrec_amd_burst_crc *, size_t, uint32_t *, uint32_t *, size_t, uint64_t *) = tfrec_amd_read_burst_crcs;\n")
    subprocess.check_call(["cc", "-std=c11", "-fsyntax-only", "-I", os.path.join(parity.ROOT, "include"), str(src)])
    assert [(n, crc.CRC_DTYPE.fields[n][1]) for n in ("bit_offset", "n_ok", "first_at")] == [("bit_offset", 24), ("n_ok", 32), ("first_at", 36)]
    L = api.load_library()
    for sym in ("tfrec_amd_enable_burst_crc", "tfrec_amd_read_burst_crcs"):
        assert sym in api.EXPORTS
        getattr(L, sym)
    assert hasattr(api.Receiver, "enable_burst_crc") and hasattr(api.Receiver, "read_burst_crcs")
    # no GPU is needed to be refused
    assert L.tfrec_amd_enable_burst_crc(None, 17240, 5, 0, 8, 0x31, 0, 0, 0) == api.E_INVAL
    n, w = C.c_uint32(7), C.c_uint64(9)
    assert L.tfrec_amd_read_burst_crcs(None, None, 0, C.byref(n), None, 0, C.byref(w)) == api.E_INVAL and (n.value, w.value) == (7, 9)
    # the memory sums: the records and the bitmap per FIFO set; 2052 bytes per stream; the table; nothing page-locked
    assert crc.device_bytes(3, 10, 65, 23) == api.FIFO_DEPTH * (400 + 12) + 3 * 2052 + 23 * 64 and crc.pinned_bytes(3) == 0
    head = open(os.path.join(parity.ROOT, "include", "tfrec_amd.h")).read()
    text = head[head.index("Frame check (tfrec_amd_enable_burst_crc"):head.index("int tfrec_amd_enable_burst_crc(tfrec_amd_ctx")]
    for words in ("floor((768000 i + R) / (2 R))", "<= 16383", "k + H >= D", "TFREC_AMD_E_OVERFLOW", "tfrec_amd_save_streams", "real recordings",
                  "one N per context", "Reflected CRCs", "all-zero frame", "v[c + D]", "2052 bytes", "16381"):
        assert " ".join(words.split()) in " ".join(text.replace(" *", " ").split()) or words in text, words


# ---- the builder and tfrec_gpu's own code in a stand-alone program
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("crc") / "crc_driver")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(parity.ROOT, "tests", "crc_driver.cpp")])
    return exe


def run_driver(exe, lines):
    out = subprocess.run([exe], input="".join(ln + "\n" for ln in lines), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    return out.stdout.splitlines()


def table_line(st):
    return "table %d %x " % (st.D, st.r0) + " ".join("%d:%x" % t for t in st.table())


def test_the_builder_and_the_argument_are_the_restatements(driver):
    sets = [crc.Settings(*a) for a in CR.SETS.values()]
    sets += [crc.Settings(48002, 256, 32, 0x04C11DB7, 0xFFFFFFFF, 0xFFFFFFFF, 7, True, True), crc.Settings(96000, 2, 8, 0xFF, 0xFF),
             crc.Settings(1000, 5, 24, 1, 0, 0xFFFFFF, 1), crc.Settings(17240, 9, 16, 0x8005, invert=True)]
    refused = ["6000 32 0 8 7 0 0 0", "999 5 0 8 31 0 0 0", "6000 5 0 12 31 0 0 0", "6000 5 4 8 31 0 0 0", "6000 5 0 8 0 0 0 0",
               "6000 5 0 8 131 0 0 0", "6000 5 0 8 31 0 0 4", "6000 0 0 8 31 0 0 0", "6000 257 0 8 31 0 0 0", "6000 5 -1 8 31 0 0 0",
               "6000 5 0 16 1021 10000 0 0", "6000 5 2 32 4c11db7 0 0 0"]
    got = run_driver(driver, ["table %d %d %d %d %x %x %x %d" % st.args() for st in sets] + ["table " + r for r in refused])
    assert got == [table_line(st) for st in sets] + ["refused"] * len(refused)
    args = {"8,31": (8, 0x31, 0, 0, 0, 0), "32,04c11db7,f59c5a1e,0,1": (32, 0x04C11DB7, 0xF59C5A1E, 0, 1, 0), "16,1021,FFFF,ffff,0,1": (16, 0x1021, 0xFFFF, 0xFFFF, 0, 1),
            "24,864cfb,b704ce": (24, 0x864CFB, 0xB704CE, 0, 0, 0), "12,1": (12, 1, 0, 0, 0, 0), "8,0,0,0,200,0": (8, 0, 0, 0, 200, 0)}
    bad = ["", "8", "8,", ",31", "8,31,", "8,xy", "x,31", "8,31,0,0,0,2", "8,31,0,0,0,inv", "8,31,0,0,0,1,0", "8,123456789", "0,31", "8,31,0,0,-1",
           "8,31,0,0,1000", "-8,31"]
    got = run_driver(driver, ["parse " + a for a in list(args) + bad])
    assert got == ["crc %d %x %x %x %d %d" % v for v in args.values()] + ["bad"] * len(bad)


@pytest.mark.parametrize("name", ["crc8", "whb"])
def test_the_host_merges_check_pieces_and_prints_the_restatements_line_and_verdicts(driver, name):
    st = CR.settings(name)
    t, frame, c = CR.planted(st, 11, pre=60)
    k = c + st.D
    lines, want = ["reach %d" % st.D, "file 100"], []
    for sizes, start in (((1000, 500), 7000), ((3, k - 500), 300000), ((), 600000)):
        pieces = pieces_of(t, sizes, start=start)
        vsubs = [crc.crcs(r, w, st, s)[:2] for (r, w), s in zip(pieces, states(pieces, st))]
        for recs, words in vsubs:
            r = recs[0]
            lines.append("piece 1 %d %d %d %d %d %d %d %s" % (int(r["flags"]), int(r["start_sample"]), int(r["n_samples"]), int(r["n_samples"]),
                                                              int(r["bit_offset"]), int(r["n_ok"]), int(r["first_at"]), " ".join("%x" % w for w in words)))
        merged = crc.chains(vsubs)
        want += [crc.line("f", m, st) for m in merged]
        frames = [(c, 0, "+", [0] * (8 * st.N)), (c + 200, 0, "+", [0] * (8 * st.N)), (c, 0, "-", [0] * (8 * st.N)), (c, 0, "+", [0] * (8 * st.N - 1))]
        lines += ["verdict %d %d %d %d" % (f[0], f[2] == "+", len(f[3]), st.N) for f in frames]
        want += crc.verdicts(frames, merged[0], st)
        assert want[-4:] == ["ok", "bad", "-", "-"]
    assert run_driver(driver, lines) == want and len(want) == 15
    # a piece the file's end cuts: n_ok and first_at are counted again on what is kept
    recs, words, _ = crc.crcs(*hand_track(t, start=0), st)
    r = recs[0]
    for keep in (k + 1, k - 40):
        got = run_driver(driver, ["reach %d" % st.D, "file 1", "piece 1 %d 0 %d %d %d %d %d %s" % (
            OPEN, int(r["n_samples"]), keep, int(r["bit_offset"]), int(r["n_ok"]), int(r["first_at"]), " ".join("%x" % w for w in words))])
        v = crc.bits_of(r, words)[:keep]
        ok = np.flatnonzero(v)
        assert got == ["crc f 0 %d %d %s" % (keep, len(ok), ok[0] - st.D if len(ok) else "-")]


# ---- the command line
def test_cli_crc_usage_errors_and_accepted_forms(tmp_path):
    parity.build_cli()
    f = str(tmp_path / "missing.iq")
    for args in (["-V", "8,31"], ["-G", "17240", "-V", "8,31"], ["-Y", "2dd4,0,5", "-V", "8,31"]):  # without -Y, without -G
        out = parity.run_cli(args + ["-L", f])
        assert out.returncode == 1 and ("-V checks the frames of -Y" in out.stderr or "-Y finds" in out.stderr), args
    out = parity.run_cli(["-G", "17240", "-Y", "2dd4,0,5,1", "-V", "8,31", "-L", f])  # -Y's both
    assert out.returncode == 1 and "not with -Y's both" in out.stderr
    for bad in ("", "8", "8,", "8,xy", "8,31,0,0,0,2", "8,31,0,0,0,1,0", "8,123456789", "0,31"):
        out = parity.run_cli(["-G", "17240", "-Y", "2dd4,0,5", "-V", bad, "-L", f])
        assert out.returncode == 1 and "bad -V" in out.stderr, bad
    refused = [("17240", "2dd4,0,5", "12,31", "width"), ("17240", "2dd4,0,5", "8,131", "poly"), ("17240", "2dd4,0,5", "8,0", "poly"),
               ("17240", "2dd4,0,5", "8,31,100", "init"), ("17240", "2dd4,0,5", "8,31,0,0,4", "at least one byte"),
               ("17240", "2dd4,0,4", "32,04c11db7", "at least one byte"), ("6000", "2dd4,0,32", "8,31", "16383"), ("12000", "2dd4,0,64", "8,31", "16383")]
    for rate, y, v, why in refused:  # a width, range or length the enable call refuses
        out = parity.run_cli(["-G", rate, "-Y", y, "-V", v, "-L", f])
        assert out.returncode == 1 and "-V: " in out.stderr and why in out.stderr, (rate, y, v)
    for args in (["-X", f], ["-s", "50", "-L", f], ["-A", "-L", f]):  # whatever -G refuses
        out = parity.run_cli(["-G", "17240", "-Y", "2dd4,0,5", "-V", "8,31"] + args)
        assert out.returncode == 1 and "-G reads" in out.stderr, args
    out = parity.run_cli(["-h"])
    assert "-V w,p[,i[,x[,s[,v]]]]" in out.stderr and "[-V width,poly[,init[,xorout[,skip[,inv]]]]]" in out.stderr
    assert "-U code[,inv]" in out.stderr and "-Y h[,e[,n[,b]]]" in out.stderr  # the others' stay
    for args in (["-G", "17240", "-Y", "2dd4,0,5", "-V", "8,31"], ["-G", "6001", "-Y", "2dd4,0,32", "-V", "8,7"],
                 ["-G", "6000,psk", "-U", "g3ruh", "-Y", "b42b,0,23,0,1", "-V", "32,04c11db7,f59c5a1e,0,1"],
                 ["-V", "16,1021,ffff,ffff,0,1", "-Y", "2dd4,1,4", "-G", "38400,psk,10"], ["-G", "9600,auto", "-Y", "2dd4,0,6,0,1", "-V", "24,864cfb,b704ce,0,1"],
                 ["-G", "6000", "-O", "2000", "-Y", "2dd4,0,5", "-V", "8,31"], ["-G", "17240", "-Y", "2dd4,0,5", "-V", "8,31", "-M", "-Q", "-C"],
                 ["-G", "17240", "-Y", "2dd4,0,5", "-V", "8,31", "-S", str(tmp_path / "cap"), "-n", "1"]):
        out = parity.run_cli(args + ["-L", f])  # accepted: the file is looked for
        assert out.returncode == 2 and "missing.iq" in out.stderr, args
    out = parity.run_cli(["-G", "17240", "-Y", "2dd4,0,5", "-V", "8,31", "-R", str(tmp_path / "nothing")])  # accepted with -R: the capture is looked for
    assert out.returncode == 2 and "-R replays" not in out.stderr and "bad -V" not in out.stderr
