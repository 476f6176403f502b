"""The inputs the amplitude track's tests share (tests/test_amplitude_cpu.py, tests/test_amplitude_gpu.py), none of which
needs a GPU: a fixed integer generator, an NRZ on-off keyed frame and a pulse-width (FS20-like) burst at the channel rate, the
hand-made rows of the GPU tests, and the restatement run submit by submit.  Imported as a plain module (`import amplitude_rows`)."""
import functools

import numpy as np

from tfrec_amd import api, capture, envelope, track

B = api.BLOCK_DEC
T = 100  # the rows' trigger threshold: their floor stays below it (|I| + |Q| <= 40)
W = 694  # the largest window of -T 2f
CONT, OPEN = capture.RUN_CONTINUES, capture.RUN_OPEN

RATE = 4800  # the NRZ burst: 80 samples a bit
SPB = 384000 // RATE
ON = 4000  # its on-amplitude; the level: half of it
WORD = 0x2DD4
PAYLOAD = "965ac369"  # no more than four equal bits in a row, and the last one a 1: the burst's last sample is over
FRAME = "aaaa2dd4" + PAYLOAD
L_NRZ = track.smooth_of(RATE)  # 16

PW_SHORT, PW_LONG, PW_EDGE = 154, 230, 192  # the pulse-width burst: 400 and 600 us, told apart at 500


def lcg(seed):
    """The fixed integer generator: x' = (1103515245 x + 12345) mod 2^31, its bits 16 .. 30."""
    x = int(seed)
    while True:
        x = (1103515245 * x + 12345) % (1 << 31)
        yield x >> 16


def floor(n, seed, amp=20):
    """n pairs of small deterministic noise, each component within +-amp -> int16 [n, 2]."""
    g = lcg(seed)
    return np.array([next(g) % (2 * amp + 1) - amp for _ in range(2 * n)], dtype=np.int16).reshape(n, 2)


def hex_bits(h):
    return [(int(c, 16) >> (3 - i)) & 1 for c in h for i in range(4)]  # MSB first


def keyed(widths, first, seed, on=ON):
    """Stretches of `widths` samples, alternately on (from `first`) and off: on is (on, 0) plus the floor's noise -> int16 [n, 2]."""
    z = floor(sum(widths), seed)
    pos, v = 0, first
    for w in widths:
        if v:
            z[pos:pos + w, 0] += on
        pos, v = pos + w, not v
    return z


def nrz(symbols, seed=7, spb=SPB, on=ON):
    """The symbols, spb samples each, on for a 1 -> int16 [spb n, 2]."""
    s = np.asarray(symbols)
    edges = np.flatnonzero(np.diff(s)) + 1
    runs = np.diff(np.concatenate([[0], edges, [len(s)]]))
    return keyed((runs * spb).tolist(), bool(s[0]), seed, on)


def row_with(burst, nb, at, seed=3):
    """nb blocks of floor with the burst from sample `at` on -> int16 [nb B, 2]."""
    z = floor(nb * B, seed)
    z[at:at + len(burst)] = burst
    return z


@functools.lru_cache(maxsize=None)
def nrz_row(nb=2, at=B - 2500):
    """The frame aaaa 2dd4 and four payload bytes as an NRZ on-off keyed burst of 64 * 80 samples across the first block boundary."""
    z = row_with(nrz(hex_bits(FRAME)), nb, at)
    z.setflags(write=False)
    return z


def pw_widths(bits):
    """FS20-like: a bit is a pulse and a gap of the same width, 154 samples for a 0 and 230 for a 1; the last gap is left out."""
    w = []
    for b in bits:
        w += [PW_LONG if b else PW_SHORT] * 2
    return w[:-1]


def pw_row(bits, nb, at=500, seed=11):
    return row_with(keyed(pw_widths(bits), True, seed), nb, at)


def submits(dec, sizes, L, level, thresh=T, types=0x2F, brute=False, levels=None):
    """One stream's samples (int16 [2 M]) cut into submits of `sizes` blocks -> the amplitude track's [(records, words)], the
    recorder's, the thresholds' and the track's state carried from one to the next.  levels: a level per submit instead."""
    cst = est = tst = None
    pos, out = 0, []
    form = track.amplitude_tracks_bruteforce if brute else track.amplitude_tracks
    for i, nb in enumerate(sizes):
        part = np.ascontiguousarray(dec).reshape(-1)[2 * pos * B:2 * (pos + nb) * B]
        runs, _, cst = capture.captures(part, types, thresh, cst)
        thr, est = envelope.thresholds(part, types, thresh, est)
        recs, words, tst = form([part], [thr], runs, L, [levels[i] if levels else level], tst, base=[pos * B])
        out.append((recs, words))
        pos += nb
    return out


# ---- the GPU tests' hand-made rows
LEVELS = [1500, 65533]


@functools.lru_cache(maxsize=None)
def hand_rows():
    """int16 [2, 2 B, 2] on a floor of +-20.  An over sample keeps the trigger up for W - 1 samples behind it.
    Stream 0 (level 1500): on-off keyed at amplitude 3000, 10 samples a stretch, from the submit's first sample to 37, the last 7 on
    (the run is 36 + W long, so every later run of the pool starts off a word boundary); 300 samples of (1500, 0) -- every full sum is exactly
    L * level: 0 -- and 300 of (1000, -501), a sum of L * level + L: 1; keyed, 22 a stretch, from B - 3 across the block boundary
    (cut there, its first piece is 3 samples); keyed to the input's last sample, where the run stays open.
    Stream 1 (level 65533): one over sample; 40 pairs (-32768, -32768), which a channel-rate context clamps to -32767: p = 65534, a
    bit 1; a run that ends a sample ahead of block 0's last one; one from block 1's first sample: all zeros at that level."""
    rows = np.stack([floor(2 * B, 21), floor(2 * B, 22)])
    k10 = keyed([10] * (2 * B // 10 + 1), True, 5, on=3000)[:2 * B]
    k22 = keyed([22] * (2 * B // 22 + 1), True, 6, on=3000)[:2 * B]
    for a, b, src in ((0, 37, k10), (B - 3, B + 2000, k22), (2 * B - 1500, 2 * B, k10)):
        rows[0, a:b] = src[a:b]
    rows[0, 30:37] = (3000, 0)
    rows[0, 2000:2300] = (1500, 0)
    rows[0, 2300:2600] = (1000, -501)
    rows[1, 1000] = (-2500, 2600)
    rows[1, 3001:3041] = (-32768, -32768)
    for a, b, src in ((B - W - 50, B - W, k10), (B, B + 500, k22)):
        rows[1, a:b] = src[a:b]
    rows[1, B - W - 7:B - W] = (3000, 0)  # (its last sample is over: the run ends W - 1 behind it)
    rows.setflags(write=False)
    return rows


# ---- a short fixed-seed random set
def generated(seed):
    """-> (rows int16 [n, 3 B, 2], a level per stream, L, the cut into submits): 2 .. 4 streams of floor, each with a few keyed
    bursts of its own amplitude, some across a block boundary or up to the row's end; levels at half the amplitude, at it, at 0
    and above it."""
    g = lcg(1000 + seed)
    n, nb = 2 + next(g) % 3, 3
    L = (1, 2, 7, 16)[next(g) % 4]
    sizes = ((3,), (1, 2), (2, 1), (1, 1, 1))[seed % 4]
    rows = np.stack([floor(nb * B, 50 * seed + s) for s in range(n)])
    lv = []
    for s in range(n):
        on = 500 + next(g) % 20000
        lv.append((on // 2, on, 0, on + 100)[next(g) % 4])
        for _ in range(1 + next(g) % 4):
            w = [1 + next(g) % 60 for _ in range(20 + next(g) % 200)]
            at = (next(g) * 7 + next(g)) % (nb * B)
            if next(g) % 3 == 0:
                at = (1 + next(g) % (nb - 1)) * B - sum(w) // 2
            k = keyed(w, True, next(g), on=on)[:nb * B - at]
            rows[s, at:at + len(k)] = k
    return rows, lv, L, sizes


# ---- tfrec_gpu -G -O -Y
@functools.lru_cache(maxsize=None)
def cli_scene():
    """The NRZ frame as a u8 recording at 1.536 MS/s (320 samples a bit, the carrier at full scale on I) in 6 blocks, placed so that
    -b 2 makes three batches and the burst lies across the first batch boundary -> (its bytes, the level: half the largest power of
    the reference front end's decimated samples, the lines the restatements expect of tfrec_gpu -G 4800 -O level -Y 2dd4,0,4 on a
    file named %s)."""
    import parity
    from tfrec_amd import sync

    n = 6 * api.BLOCK_BYTES
    x = (127 + np.arange(n) * 7919 % 3).astype(np.uint8)
    at = 4 * (2 * B - 2500)
    for i, s in enumerate(hex_bits(FRAME)):
        if s:
            x[2 * (at + 4 * SPB * i):2 * (at + 4 * SPB * (i + 1)):2] = 228
    dec = parity.fresh_oracle(x, 0x2F, 500, keep_dec=True).dec().reshape(-1, 2)
    level = int(np.abs(dec.astype(np.int64)).sum(axis=1).max()) // 2
    tsubs = submits(dec, (2, 2, 2), L_NRZ, level, thresh=500)
    assert any(r["flags"] & CONT for r in tsubs[1][0]), "the burst is not cut by the batches"
    st, state, ssubs = sync.Settings(RATE, WORD, 16, 0), None, []
    for recs, words in tsubs:
        srecs, swords, state = sync.syncs(recs, words, st, state, 1)
        ssubs.append((srecs, swords))
    want = []
    for t, s in zip(track.chains(tsubs), sync.chains(ssubs)):
        want += [track.line("%s", t, RATE), track.pulses_line("%s", t)] + [sync.line("%s", s, f) for f in sync.frames(t, s, st, 4)]
    return x, level, want
