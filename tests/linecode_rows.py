"""The inputs the line code's tests share (tests/test_linecode_cpu.py, tests/test_linecode_gpu.py), none of which needs
a GPU: tracks and their records by hand, a track cut into pieces, the restatement run submit by submit, the tap sets the GPU
tests run, and the figures the feature was specified with.  Imported as a plain module (`import linecode_rows`)."""
import numpy as np

import recorder_rows as RR
from tfrec_amd import api, capture, linecode, sync, track

B = api.BLOCK_DEC

CONT, OPEN = capture.RUN_CONTINUES, capture.RUN_OPEN
WORD = 0xB42B  # 2dd4 as the TFA_1 and WHB transmitters send it: every byte LSB-first
# the tap sets of the GPU tests: (rate, taps, invert); delta(32) at 6002 bit/s is 2047, the largest span there is (6001: 2048)
SETS = {"nrzi": (38400, 1, False), "nrzs": (38400, 1, True), "g3ruh": (6000, 0x10800, False), "span2047": (6002, (1 << 31) | 1, False)}
# the golden WHB scene behind G3RUH at 6000 bit/s (phase track: m = 64, L = 16, K = 1024), word b42b, P = 16
WHB_PLATEAU = (14281, 14344)
WHB_PLATEAU_E2 = (19337, 19400)  # the second one, at E = 2 only
WHB_FRAME = "2b1603a290d9d3cf962a73e1ec2a34c87390cc8e5308a0ffffff"  # 208 bits, LSB-first per byte: bytes 3 .. 28 of the event
WHB_N_ONES = 20625
WHB_SLICED = 432
WHB_RAW_BEST = 3  # the raw track's best distance to b42b: no match at E <= 1
TFA_1_FRAMES = ("3dc488941c6010566e", "7fd682573a60d05660")  # the nine bytes behind b42b, LSB-first per byte


def settings(name):
    rate, taps, inv = SETS[name]
    return linecode.Settings(rate, taps, inv)


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


def pieces_of(t, sizes, start=7000):
    """A track cut into pieces of `sizes` samples (the last takes the rest), one submit each."""
    out, pos = [], 0
    sizes = list(sizes) + [len(t) - sum(sizes)]
    for i, n in enumerate(sizes):
        flags = (CONT if i else 0) | (OPEN if i + 1 < len(sizes) else 0)
        out.append(hand_track(t[pos:pos + n], flags, offset=5 * i, start=start + pos))
        pos += n
    return out


def held(symbols, spb):
    """An ideal track: every symbol held for spb samples."""
    return np.repeat(np.asarray(symbols, dtype=np.uint8), spb)


def code_submits(tsubs, st, brute=False, n_streams=1, state=None):
    """Track submits [(records, words)] -> the code's [(records, words)], the state carried from one to the next."""
    out = []
    for recs, words in tsubs:
        r, w, state = (linecode.codes_bruteforce if brute else linecode.codes)(recs, words, st, state, n_streams)
        out.append((r, w))
    return out


def sync_submits(csubs, st, n_streams=1):
    """Coded submits -> the sync's [(records, words)] on them."""
    state, out = None, []
    for recs, words in csubs:
        r, w, state = sync.syncs(recs, words, st, state, n_streams)
        out.append((r, w))
    return out


def scrambled(bits, delays):
    """A self-synchronising scrambler's output: s[i] = b[i] ^ XOR of s[i - j] over the delays (nothing ahead of the first: 0)."""
    s = []
    for i, b in enumerate(bits):
        v = int(b)
        for j in delays:
            v ^= s[i - j] if i >= j else 0
        s.append(v)
    return s


# ---- hand-made rows for the GPU tests (channel-rate contexts; threshold 100, the floor stays below it)
def fsk_rows():
    """int16 [2, 2 B, 2], phase_rows.hand_rows' FSK sibling at 17240 bit/s.
    Stream 0: 37 tone samples from the submit's first sample (a run at index 0, so every later run of the pool starts off a word
    boundary); a frame from B - 3 across the block boundary (cut there, its first piece is 3 samples); a run open at the input's
    last sample, 100 samples.
    Stream 1: a frame inside block 0; one from B - 500 across the block boundary; one over sample at 2 B - 2: a run of 2 samples,
    open, shorter than every delta.
    Block 1 holds fewer captured samples than block 0: a pool sized on the first of two submits of a block holds the second."""
    rng = np.random.default_rng(21)
    rows = np.stack([RR.quiet(2, 51), RR.quiet(2, 52)])
    rows[0, :37] = RR.fsk([1, 0], 17240)[:37]
    rows[0, B - 3:B - 3 + 800] = RR.fsk(rng.integers(0, 2, 120).tolist(), 17240)[:800]
    rows[0, 2 * B - 100:] = RR.fsk([1, 0] * 50, 17240)[:100]
    rows[1, 300:300 + 1500] = RR.fsk(rng.integers(0, 2, 90).tolist(), 17240)[:1500]
    rows[1, B - 500:B - 500 + 1200] = RR.fsk(rng.integers(0, 2, 150).tolist(), 17240)[:1200]
    rows[1, 2 * B - 2] = (3000, -3000)
    rows.setflags(write=False)
    return rows


def long_rows():
    """int16 [2, 3 B, 2]: FSK transmissions of fixed pseudo-random symbols from B - 1000 (stream 0) and B - 1500 (stream 1) to
    2 B + 3000: in submits of one block a chain of three pieces, 1000 (1500) samples, a whole block and the rest."""
    rows = np.stack([RR.quiet(3, 53), RR.quiet(3, 54)])
    for s, at in ((0, B - 1000), (1, B - 1500)):
        n = 2 * B + 3000 - at
        rows[s, at:at + n] = RR.fsk(np.random.default_rng(60 + s).integers(0, 2, n * 17240 // 384000 + 2).tolist(), 17240)[:n]
    rows.setflags(write=False)
    return rows


# ---- tfrec_gpu -G 6000,psk -U g3ruh -Y b42b,0,26,0,1
CLI_RATE = 6000
CLI_SHIFT = 9000


def cli_scene():
    """The golden WHB scene as a u8 recording, moved 9000 decimated samples on inside 8 blocks of silence, so that -b 2 makes four
    batches and the sync word (the 960 samples up to the scene's 24316) lies across the boundary at 32768 -> (its bytes, the lines
    the restatements expect of tfrec_gpu -G 6000,psk -U g3ruh -Y b42b,0,26,0,1 on a file named %s: per burst its centre line, its
    bits line, its code line and its frame lines)."""
    import parity
    import phase_rows as P
    x = np.full(8 * api.BLOCK_BYTES, 128, dtype=np.uint8)
    scene = RR.golden_iq("whb", 6)[0]
    x[8 * CLI_SHIFT:8 * CLI_SHIFT + len(scene)] = scene
    # the restatement: the oracle's front end (the context's, bit for bit), then capture.py, envelope.py's thresholds and track.py
    # submit by submit (2 + 2 + 2 + 2), linecode.py on those tracks and sync.py on the coded ones
    dec = parity.fresh_oracle(x, 0x2F, 500, keep_dec=True).dec().reshape(-1)
    subs = P.submits(dec, (2, 2, 2, 2), track.smooth_of(CLI_RATE), track.lag_of(CLI_RATE))
    assert any(c["flags"] & CONT for c in subs[2][0]), "no burst is cut by the batches"
    st = sync.Settings(CLI_RATE, WORD, 16, 0)
    csubs = code_submits([s[1:] for s in subs], linecode.g3ruh(CLI_RATE))
    ssubs = sync_submits(csubs, st)
    cen, trk = P.chains(subs)
    want = []
    for c, t, u, s in zip(cen, trk, linecode.chains(csubs), sync.chains(ssubs)):
        a = int(s["start_sample"])
        for p in sync.plateaus(s.bits[:int(t["last_over"]) + 1]):
            assert a + p[1] - st.span < 4 * B <= a + p[1], "the sync word does not lie across the batch boundary"
        want += [track.centre_line("%s", c), track.line("%s", t, CLI_RATE), linecode.line("%s", u, CLI_RATE)]
        want += [sync.line("%s", s, f) for f in sync.frames(u, s, st, 26, lsb=True)]
    return x, want
