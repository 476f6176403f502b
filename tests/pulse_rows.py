"""The inputs the pulse slicer's tests share (tests/test_pulsecode_cpu.py, tests/test_pulsecode_gpu.py), none of which
needs a GPU: track records made by hand from bit lists, the restatement run submit by submit, the hand-made rows of the GPU tests and
tfrec_gpu -J's scene.  Imported as a plain module (`import pulse_rows`)."""
import functools

import numpy as np

import amplitude_rows as A
from tfrec_amd import api, pulsecode, track

B, CONT, OPEN = A.B, A.CONT, A.OPEN
FS20 = (100, 192, 300)  # lo, mid, hi at 384 kS/s: 400 us against 600 us
LEVEL = 1500  # the hand-made rows' level: ON samples read 1, HELD samples 0 and keep the trigger up
ON, HELD = (3000, 0), (500, 0)


def stretches(*widths, first=1):
    """Stretches of `widths` samples, alternately 1 and 0 from `first` on -> a list of bits."""
    out, v = [], first
    for w in widths:
        out += [v] * w
        v ^= 1
    return out


def submit_of(runs):
    """runs: [(stream, flags, start_sample, bits)] in table order -> (track records, track words) of one submit."""
    recs, off = np.zeros(len(runs), dtype=track.TRACK_DTYPE), 0
    for o, (s, flags, start, bits) in zip(recs, runs):
        o["stream"], o["flags"], o["start_sample"], o["n_samples"], o["bit_offset"], o["n_ones"] = s, flags, start, len(bits), off, sum(bits)
        off += len(bits)
    return recs, track._pack(recs, [np.array(b, dtype=np.uint8) for _, _, _, b in runs], None)


def cut_chain(bits, sizes):
    """One run of stream 0 from sample 0 on, cut into submits of `sizes` blocks -> [(track records, track words)]."""
    ends = np.cumsum(sizes) * B
    return [submit_of([(0, (CONT if a else 0) | (OPEN if e < len(bits) else 0), int(a), bits[a:e])]) for a, e in zip(ends - np.array(sizes) * B, ends)]


def restated(tsubs, st, n_streams=1, max_samples=None):
    """The restatement submit by submit -> [(records, bits words, marks words)]."""
    state, out = None, []
    for trecs, twords in tsubs:
        recs, bits, marks, state = pulsecode.symbols_bruteforce(trecs, twords, st, state, n_streams, max_samples)
        out.append((recs, bits, marks))
    return out


@functools.lru_cache(maxsize=None)
def hand_rows():
    """int16 [2, 2 B, 2] on a floor of +-20, for an amplitude track with L = 1 at LEVEL; a HELD sample reads 0 inside a run.
    Stream 0: samples alternating from 64 to 264 (16 symbols a word at lo = 1); a pulse of 40 across the word boundary at 320; one of
    100 across sample 2048, where a wave ends; a gap of 100 across 4096; alternating from B - 1700 (100 falls ahead of block 1: no
    multiple of 32), then 2500 samples of pulse across the block boundary, a gap of 40, a pulse of 5; a run of the last 3 samples.
    Stream 1: pulses of 30 and 140 around a gap of 30; a pulse of 100, a gap of 2400, a pulse of 70, a gap of 60 across the block
    boundary, a pulse of 50.  Its first run's bits follow the 3-sample run's in the pool: they share a word."""
    rows = np.stack([A.floor(2 * B, 31), A.floor(2 * B, 32)])

    def put(s, a, e, v, step=1):
        rows[s, a:e:step] = v

    put(0, 64, 264, HELD), put(0, 64, 264, ON, 2)
    put(0, 300, 340, ON), put(0, 340, 400, HELD), put(0, 400, 420, ON)
    put(0, 2000, 2100, ON), put(0, 4000, 4050, ON), put(0, 4050, 4150, HELD), put(0, 4150, 4160, ON)
    put(0, B - 1700, B - 1500, HELD), put(0, B - 1700, B - 1500, ON, 2)
    put(0, B - 1500, B + 1000, ON), put(0, B + 1000, B + 1040, HELD), put(0, B + 1040, B + 1045, ON)
    put(0, 2 * B - 3, 2 * B, ON), put(0, 2 * B - 2, 2 * B - 1, HELD)
    put(1, 200, 230, ON), put(1, 230, 260, HELD), put(1, 260, 400, ON)
    put(1, B - 2600, B - 2500, ON), put(1, B - 2500, B - 100, HELD), put(1, B - 100, B - 30, ON), put(1, B - 30, B + 30, HELD), put(1, B + 30, B + 80, ON)
    rows.setflags(write=False)
    return rows


CLI_BITS = [0, 1, 1, 0, 1, 0, 0, 1, 1, 1, 0, 0]


@functools.lru_cache(maxsize=None)
def cli_scene():
    """The FS20-like burst of CLI_BITS as a u8 recording at 1.536 MS/s in 6 blocks, across the first boundary of -b 2's batches ->
    (its bytes, the level, the lines the restatements expect of tfrec_gpu -G 2500 -O level -J width,100,192,300 on a file %s)."""
    import parity

    x = (127 + np.arange(6 * api.BLOCK_BYTES) * 7919 % 3).astype(np.uint8)
    pos, on = 4 * (2 * B - 1500), True
    for w in A.pw_widths(CLI_BITS):
        if on:
            x[2 * pos:2 * (pos + 4 * w):2] = 228
        pos, on = pos + 4 * w, not on
    dec = parity.fresh_oracle(x, 0x2F, 500, keep_dec=True).dec().reshape(-1, 2)
    level = int(np.abs(dec.astype(np.int64)).sum(axis=1).max()) // 2
    tsubs = A.submits(dec, (2, 2, 2), track.smooth_of(2500), level, thresh=500)
    assert any(r["flags"] & CONT for r in tsubs[1][0]), "the burst is not cut by the batches"
    want = []
    for t, s in zip(track.chains(tsubs), pulsecode.chains(restated(tsubs, pulsecode.Settings(pulsecode.WIDTH, *FS20)))):
        want += [track.line("%s", t, 2500), track.pulses_line("%s", t), pulsecode.line("%s", s)]
    return x, level, want
