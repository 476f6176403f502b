"""The inputs the auto-centre track's tests share (tests/test_centre_cpu.py, tests/test_centre_gpu.py), none of which
needs a GPU: tones and FSK bursts about a carrier offset at the channel rate, the hand-made rows of the GPU tests with what each
of their runs is there for, the restatement run submit by submit, the mixed TFA_2 stream and tfrec_gpu's scene.  Imported as a
plain module (`import centre_rows`)."""
import functools

import numpy as np

import recorder_rows as RR
from tfrec_amd import api, capture, envelope, track

B = api.BLOCK_DEC
T = 100  # the rows' trigger threshold: their floor stays below it (|I| + |Q| <= 40)
W = 694  # the largest window of -T 2f
CONT, OPEN = capture.RUN_CONTINUES, capture.RUN_OPEN
M, F, I = track.MEASURED, track.FALLBACK, track.INHERITED
ROTATIONS = (0, 20000, -35000, 60000, -90000, 120000, -141000)
# the issue's table: per scene and rotation the (centre_hz, deviation_hz) of both runs at -t 500, types 0x2f, K = 1024
FIGURES = {("tfa_2", 0): ((3000, 33000), (6000, 54000)), ("tfa_3", 0): ((9000, 45000), (-3000, 45000)),
           ("tx22", 0): ((3000, 51000), (3000, 51000)), ("tfa_2", 20000): ((21000, 33000), (27000, 51000)),
           ("tfa_3", 20000): ((24000, 48000), (15000, 45000)), ("tx22", 20000): ((24000, 48000), (24000, 54000))}
MIXED_CUT = 18000  # the mixed stream: +40 kHz up to this decimated sample, -40 kHz from it on
MIXED_FIGURES = ((39000, 33000), (-33000, 51000))


def floor(n, seed, amp=20):
    """n pairs of small deterministic noise, each component within +-amp -> int16 [n, 2]."""
    x = np.arange(2 * n, dtype=np.int64) * 2654435761 + 40503 * seed
    return ((x >> 7) % (2 * amp + 1) - amp).astype(np.int16).reshape(n, 2)


def tone(freqs, amp=6000, phase=0.0):
    """A phase-continuous signal whose sample k turns by freqs[k] Hz from sample k - 1 -> int16 [n, 2].  The product of samples k
    and k - 1 points along freqs[k] but for the rounding (under 2e-4 rad at this amplitude): at a bin's centre it is in the bin."""
    ph = phase + 2 * np.pi * np.cumsum(np.asarray(freqs, dtype=np.float64)) / 384000.0
    return np.stack([np.rint(amp * np.cos(ph)), np.rint(amp * np.sin(ph))], axis=1).astype(np.int16)


def fsk(n, centre, dev=30000, spb=40, seed=1, amp=6000):
    """n samples of two-tone FSK about `centre`: alternating symbols first, then fixed pseudo-random ones, spb samples each."""
    sym = np.array([(k % 2) if k < 16 else (k * k * 7 + seed * 13 + k // 3) % 2 for k in range(n // spb + 1)])
    return tone(centre + dev * (2 * sym[np.arange(n) // spb] - 1), amp, phase=0.1 * seed)


# ---- the GPU tests' hand-made rows (the CPU tests use them too)
FALLBACK = [24000, -7000]  # (neither is a centre one of the rows' bursts measures)
EXACT_P = 160  # the exact-occupancy pair: 161 over samples; a bin needs (160 + 15) // 16 = 10 products


def exact_pair(n_other):
    """161 samples: a tone at +30 kHz (bin 5) with n_other products at -48 kHz (bin -8) in its middle."""
    f = np.full(EXACT_P + 1, 30000)
    f[50:50 + n_other] = -48000
    return tone(f)


@functools.lru_cache(maxsize=None)
def hand_rows():
    """int16 [2, 2 B, 2] on a floor of +-20.  An over sample keeps the trigger up for W - 1 samples behind it.
    Every FSK burst's two tones lie 30 kHz from its centre, at bin centres (the centre is a multiple of 6 kHz): the head holds
    both, so lo and hi are their bins, the centre is the burst's and the deviation 30000.
    Stream 0: FSK about +18 kHz from the submit's first sample, 300 samples (a run at index 0, shorter than 1024); FSK about
    +42 kHz and about -42 kHz, 1500 samples each; FSK about +12 kHz from B - 3 across the block boundary (cut there, its first piece
    is 3 samples); FSK about -60 kHz to the input's last sample, where the run stays open.
    Stream 1: a tone at 18 kHz of 64 samples (63 products) and one of 65 (64); the exact-occupancy pair; 1000 samples of FSK about
    -18 kHz with three samples under the threshold inside (a pair and a single one: 3 + 2 products less); FSK about +48 kHz from
    B - 500 across the block boundary; one over sample."""
    rows = np.stack([floor(2 * B, 21), floor(2 * B, 22)])
    for at, z in ((0, fsk(300, 18000, seed=2)), (2000, fsk(1500, 42000, seed=3)), (5000, fsk(1500, -42000, seed=4)),
                  (B - 3, fsk(1203, 12000, seed=5)), (2 * B - 1500, fsk(1500, -60000, seed=6))):
        rows[0, at:at + len(z)] = z
    for at, z in ((1000, tone([18000] * 64)), (2000, tone([18000] * 65)), (3000, exact_pair(10)), (4200, exact_pair(9)),
                  (5500, fsk(1000, -18000, seed=7)), (B - 500, fsk(2000, 48000, seed=8)), (B + 3000, tone([0], amp=3000))):
        rows[1, at:at + len(z)] = z
    rows[1, [5600, 5601, 5700]] = 0
    rows.setflags(write=False)
    return rows


# (stream, start): what head_centres gives at K = 1024 with the fallbacks above -- (n_counted, source, centre_hz, deviation_hz)
HAND_1024 = {(0, 0): (299, M, 18000, 30000), (0, 2000): (1023, M, 42000, 30000), (0, 5000): (1023, M, -42000, 30000),
             (0, B - 3): (1023, M, 12000, 30000), (0, 2 * B - 1500): (1023, M, -60000, 30000),
             (1, 1000): (63, F, -7000, 0), (1, 2000): (64, M, 18000, 0), (1, 3000): (160, M, -9000, 39000),
             (1, 4200): (160, M, 30000, 0), (1, 5500): (994, M, -18000, 30000), (1, B - 500): (1023, M, 48000, 30000),
             (1, B + 3000): (0, F, -7000, 0)}


def submits(dec, sizes, L, K, fallback=0, thresh=500, types=0x2F, brute=False, restarts=()):
    """One stream's samples (int16 [2 M]) cut into submits of `sizes` blocks -> [(centre records, track records, words)], the
    recorder's, the thresholds' and the track's states carried from one to the next; restarts: the submits the stream restarts
    with."""
    cst = est = st = None
    pos, out = 0, []
    for i, nb in enumerate(sizes):
        if i in restarts:
            cst = est = st = None
            pos = 0
        part = np.ascontiguousarray(dec).reshape(-1)[2 * sum(sizes[:i]) * B:2 * (sum(sizes[:i]) + nb) * B]
        runs, _, cst = capture.captures(part, types, thresh, cst)
        thr, est = envelope.thresholds(part, types, thresh, est)
        cen, recs, words, st = track.auto_tracks([part], [thr], runs, L, K, [fallback], st, base=[pos * B], brute=brute)
        out.append((cen, recs, words))
        pos += nb
    return out


def chains(subs, restarts=None):
    """-> (the merged centre records, the merged tracks), both in burst.chains' order."""
    return track.centre_chains([s[0] for s in subs], restarts), track.chains([(s[1], s[2]) for s in subs], restarts)


def reads(piece, rate, telegram):
    """The slice of the merged track's first last_over + 1 samples holds the telegram's 48 bits, in positive polarity."""
    return RR.pattern(telegram) in RR.bit_string(track.slice_bits(piece.bits[:int(piece["last_over"]) + 1], rate))


def fixed(dec, L, centre, thresh=500):
    """The frequency track about one centre, uncut -> its merged chains."""
    return track.chains(RR.submits(dec, (len(dec) // (2 * B),), L, centre, thresh=thresh))


@functools.lru_cache(maxsize=None)
def mixed_dec():
    """The golden TFA_2 scene rotated +40 kHz up to decimated sample MIXED_CUT -- behind its first burst -- and -40 kHz after it."""
    d = RR.golden_dec("tfa_2")
    x = np.concatenate([RR.rotated(d, 40000)[:2 * MIXED_CUT], RR.rotated(d, -40000)[2 * MIXED_CUT:]])
    x.setflags(write=False)
    return x


# ---- tfrec_gpu -G rate,auto -Y
@functools.lru_cache(maxsize=None)
def cli_scene():
    """The golden TFA_2 scene as a u8 recording at 1.536 MS/s, turned by +40 kHz up to its raw sample 4 MIXED_CUT and by -40 kHz
    after it, moved 5500 decimated samples back inside 6 blocks of silence, so that -b 2 makes three batches and both bursts lie
    across a batch boundary -> (its bytes, the lines the restatements expect of tfrec_gpu -G 17240,auto -Y 2dd4,0,4 on a file
    named %s: per burst its centre line, its bits line and its frame lines)."""
    import parity
    from tfrec_amd import sync

    scene = RR.golden_iq()[0].astype(np.float64)
    z = (scene[0::2] - 127.5) + 1j * (scene[1::2] - 127.5)
    hz = np.where(np.arange(len(z)) < 4 * MIXED_CUT, 40000.0, -40000.0)
    y = z * np.exp(2j * np.pi * np.cumsum(hz) / 1536000.0)
    x = np.full(6 * api.BLOCK_BYTES, 128, dtype=np.uint8)
    x[8 * 5500:8 * 5500 + 2 * len(y):2] = np.clip(np.rint(y.real + 127.5), 0, 255).astype(np.uint8)
    x[8 * 5500 + 1:8 * 5500 + 2 * len(y):2] = np.clip(np.rint(y.imag + 127.5), 0, 255).astype(np.uint8)
    # the restatement: the oracle's front end (the context's, bit for bit), then capture.py, envelope.py's thresholds and track.py
    # submit by submit (2 + 2 + 2)
    dec = parity.fresh_oracle(x, 0x2F, 500, keep_dec=True).dec().reshape(-1)
    rate = RR.RATE["tfa_2"]
    subs = submits(dec, (2, 2, 2), track.smooth_of(rate), 1024)
    assert any(c["flags"] & CONT for c in subs[1][0]) and any(c["flags"] & CONT for c in subs[2][0]), "a burst is not cut by the batches"
    st, state, ssubs = sync.Settings(rate, RR.WORD, 16, 0), None, []
    for _, recs, words in subs:
        srecs, swords, state = sync.syncs(recs, words, st, state, 1)
        ssubs.append((srecs, swords))
    cen, trk = chains(subs)
    want = []
    for c, t, s in zip(cen, trk, sync.chains(ssubs)):
        want += [track.centre_line("%s", c), track.line("%s", t, rate)] + [sync.line("%s", s, f) for f in sync.frames(t, s, st, 4)]
    return x, want
