"""The inputs the phase track's tests share (tests/test_phase_cpu.py, tests/test_phase_gpu.py), none of which needs a
GPU: phase-keyed frames about a carrier offset at the channel rate, the hand-made rows of the GPU tests with what each of their
runs is there for, the restatement run submit by submit, the G3RUH descrambler and the byte order the two golden scenes need,
and tfrec_gpu's scene.  Imported as a plain module (`import phase_rows`)."""
import functools
import json
import os

import numpy as np

import parity
import recorder_rows as RR
from tfrec_amd import api, capture, envelope, sync, track

B = api.BLOCK_DEC
T = 100  # the rows' trigger threshold: RR.quiet stays below it (|I| + |Q| <= 80)
W = 694  # the largest window of -T 2f
CONT, OPEN = capture.RUN_CONTINUES, capture.RUN_OPEN
M, F, I = track.MEASURED, track.FALLBACK, track.INHERITED
ROTATIONS = (20000, -35000, 60000, -90000, 120000, -141000)
WORD = 0xB42B  # 2dd4 as the TFA_1 and WHB transmitters send it: every byte LSB-first
SPB = 10  # the hand-made frames' samples per symbol: 38400 bit/s
RATE = 38400
SETS = ((1, 1, 1024), (5, 10, 1024), (16, 64, 1024), (5, 10, 64), (5, 10, 4096))  # (L, m, K)
FALLBACK = [24000, -7000]

# the issue's table: at -t 500, types 0x2f, K = 1024; per scene (rate, m, L, [(start, n_samples, last_over, n_counted, index)], the
# indices under ROTATIONS, the sliced bits per run)
GOLDEN = {"tfa_1": (38400, 10, 5, [(10004, 4056, 3362, 975, 4031), (28315, 4056, 3362, 819, 37)],
                    [(149, 250), (3658, 3760), (575, 677), (3071, 3173), (1215, 1317), (2527, 2629)], 336),
          "whb": (6000, 64, 16, [(10004, 28344, 27650, 1007, 32)], [(246,), (3755,), (672,), (3168,), (1312,), (2624,)], 432)}
TFA_1_TELEGRAMS = ("2dd43dc488941c6010566e", "2dd47fd682573a60d05660")
TFA_1_PLATEAUS = ((2153, 2162), (2154, 2162))
TFA_1_PAYLOADS = ("bc231129", "fe6b41ea")
FROM_BIT = 200  # where both scenes' telegrams begin in the sliced bits


def psk(symbols, hz, spb=SPB, amp=6000, phase=0.3):
    """An NRZ-S phase-keyed burst: a carrier at hz whose sign toggles at the start of every 0 symbol, spb samples a symbol, the
    envelope unshaped -> int16 [len(symbols) spb, 2].  A detector at a lag of spb samples reads symbol i >= 1 at every sample of it."""
    sign = np.cumprod(np.where(np.asarray(symbols) != 0, 1.0, -1.0))
    k = np.arange(len(symbols) * spb)
    z = amp * sign[k // spb] * np.exp(1j * (phase + 2 * np.pi * hz * k / 384000.0))
    return np.stack([np.rint(z.real), np.rint(z.imag)], axis=1).astype(np.int16)


def symbols(n, seed, word_at=None):
    """n fixed pseudo-random symbols; word_at: WORD's 16 bits from there on, behind alternating symbols."""
    s = np.random.default_rng(seed).integers(0, 2, n).tolist()
    if word_at is not None:
        s[:word_at] = [k % 2 for k in range(word_at)]
        s[word_at:word_at + 16] = RR.word_bits(WORD, 16)
    return s


def quarter_turns(n):
    """n samples whose one-sample products alternate +90 and -90 degrees: dot = 0 and crs = +-3000^2; an even count sums to (0, 0)."""
    z = np.zeros((n, 2), dtype=np.int16)
    z[0::2, 0], z[1::2, 1] = 3000, 3000
    return z


# (stream, start, hz, symbols): the frames of hand_rows
FRAMES = ((0, 0, 30000, symbols(60, 1)), (0, 2000, -52000, symbols(150, 2, word_at=20)), (0, B - 3, 12000, symbols(120, 3, word_at=30)),
          (0, 2 * B - 1500, -77000, symbols(150, 4)), (1, 2500, 100000, symbols(80, 5, word_at=16)), (1, B - 500, 48000, symbols(200, 6, word_at=24)))
ZERO_SUMS = (1, 3350, 3500)  # stream 1: (0, 0) pairs inside the window behind the frame at 2500


@functools.lru_cache(maxsize=None)
def hand_rows():
    """int16 [2, 2 B, 2] on RR.quiet.  An over sample keeps the trigger up for W - 1 samples behind it.
    Stream 0: a frame at +30 kHz from the submit's first sample (a run at index 0); one at -52 kHz that holds WORD; one at +12 kHz
    from B - 3 across the block boundary (cut there, its first piece is 3 samples: shorter than m = 10 and 64, the fallback);
    one at -77 kHz to the input's last sample, where the run stays open.
    Stream 1: 201 samples of quarter turns (200 products that sum to (0, 0): the fallback whatever K); a frame at +100 kHz and,
    inside the window behind it, 150 pairs that are (0, 0) -- every product and every sum there is exactly 0, the bits are 0 --; a
    frame at +48 kHz from B - 500 across the block boundary; one over sample; one over sample at 2 B - 2: a run of 2 samples,
    open, shorter than every m but 1.
    The runs lie back to back in the pool and none but by chance is a multiple of 32 long: neighbours share a bitmap word."""
    rows = np.stack([RR.quiet(2, 31), RR.quiet(2, 32)])
    for s, at, hz, sym in FRAMES:
        z = psk(sym, hz)
        rows[s, at:at + len(z)] = z
    rows[1, 1000:1201] = quarter_turns(201)
    rows[ZERO_SUMS[0], ZERO_SUMS[1]:ZERO_SUMS[2]] = 0
    rows[1, B + 3000] = (3000, -3000)
    rows[1, 2 * B - 2] = (3000, -3000)
    rows.setflags(write=False)
    return rows


# (stream, start) of every run of hand_rows, in the table's order
HAND_RUNS = [(0, 0), (0, 2000), (0, B - 3), (0, 2 * B - 1500), (1, 1000), (1, 2500), (1, B - 500), (1, B + 3000), (1, 2 * B - 2)]


def submits(dec, sizes, L, m, K=1024, fallback=0, thresh=500, types=0x2F, brute=False):
    """One stream's samples (int16 [2 M]) cut into submits of `sizes` blocks -> [(carrier records, track records, words)], the
    recorder's, the thresholds' and the track's states carried from one to the next."""
    cst = est = st = None
    pos, out = 0, []
    form = track.phase_tracks_bruteforce if brute else track.phase_tracks
    for nb in sizes:
        part = np.ascontiguousarray(dec).reshape(-1)[2 * pos * B:2 * (pos + nb) * B]
        runs, _, cst = capture.captures(part, types, thresh, cst)
        thr, est = envelope.thresholds(part, types, thresh, est)
        cen, recs, words, st = form([part], [thr], runs, L, m, K, [fallback], st, base=[pos * B])
        out.append((cen, recs, words))
        pos += nb
    return out


def chains(subs, restarts=None):
    """-> (the merged carrier records, the merged tracks), both in burst.chains' order."""
    return track.centre_chains([s[0] for s in subs], restarts), track.chains([(s[1], s[2]) for s in subs], restarts)


def sliced(piece, rate):
    """The symbols of the merged track's first last_over + 1 samples."""
    return track.slice_bits(piece.bits[:int(piece["last_over"]) + 1], rate)


def descrambled(bits):
    """G3RUH: out = x ^ lfsr bit 16 ^ lfsr bit 11, lfsr = (lfsr << 1) | x."""
    lfsr, out = 0, []
    for x in bits:
        out.append(x ^ ((lfsr >> 16) & 1) ^ ((lfsr >> 11) & 1))
        lfsr = ((lfsr << 1) | x) & 0xFFFFFFFF
    return out


def lsb_first(hexbytes):
    """A telegram's bytes -> its bits in the order of transmission: every byte LSB-first."""
    return [(b >> i) & 1 for b in bytes.fromhex(hexbytes) for i in range(8)]


@functools.lru_cache(maxsize=None)
def whb_event_bytes():
    """The golden WHB scene's telegram as its event records it (the type-4 event's bytes)."""
    meta = json.loads(str(np.load(os.path.join(parity.ROOT, "tests", "golden", "iq_whb.npz"))["meta"]))
    ev = [e for e in meta["events"] if e[0] == 4]
    assert len(ev) == 1 and ev[0][5].startswith("4b2dd42b1603a2")
    return ev[0][5]


def figures(c):
    return (int(c["start_sample"]), int(c["n_samples"]), int(c["n_counted"]), int(c["index"]))


# ---- tfrec_gpu -G 38400,psk -Y b42b
@functools.lru_cache(maxsize=None)
def cli_scene():
    """The golden TFA_1 scene as a u8 recording, moved 5500 decimated samples back inside 6 blocks of silence, so that -b 2 makes
    three batches and the first telegram lies across a batch boundary -> (its bytes, the lines the restatements expect of tfrec_gpu
    -G 38400,psk -Y b42b,0,4 on a file named %s: per burst its centre line, its bits line and its frame lines)."""
    x = np.full(6 * api.BLOCK_BYTES, 128, dtype=np.uint8)
    scene = RR.golden_iq("tfa_1")[0]
    x[8 * 5500:8 * 5500 + len(scene)] = scene
    # the restatement: the oracle's front end (the context's, bit for bit), then capture.py, envelope.py's thresholds and track.py
    # submit by submit (2 + 2 + 2)
    dec = parity.fresh_oracle(x, 0x2F, 500, keep_dec=True).dec().reshape(-1)
    subs = submits(dec, (2, 2, 2), track.smooth_of(RATE), track.lag_of(RATE))
    assert any(c["flags"] & CONT for c in subs[1][0]), "no burst is cut by the batches"
    st, state, ssubs = sync.Settings(RATE, WORD, 16, 0), None, []
    for _, recs, words in subs:
        srecs, swords, state = sync.syncs(recs, words, st, state, 1)
        ssubs.append((srecs, swords))
    cen, trk = chains(subs)
    want = []
    for c, t, s in zip(cen, trk, sync.chains(ssubs)):
        want += [track.centre_line("%s", c), track.line("%s", t, RATE)] + [sync.line("%s", s, f) for f in sync.frames(t, s, st, 4)]
    return x, want
