"""The inputs and expectations the recorder family's tests share, none of which needs a GPU: hand-made channel-rate rows (a quiet
floor, keyed tones, FSK frames, silent and full-scale segments), the golden scenes with what their bursts must read, the aimed u8
scene of the squelched recorder, and the small forms the comparisons of chains use.  The family: the recorder, the channel-rate
input and the five measurements on the run table -- meter, envelope, clock, track, sync (tests/test_{capture,decin,burst,envelope,
clock,track,sync}_{cpu,gpu}.py, tests/test_stream_counts_*.py, tests/recorder_campaign.py).  tests/recorder.py holds what touches
a receiver.  Imported as a plain module (`import recorder_rows`).

recorder_campaign's plan digests (tests/test_recorder_campaign_cpu.py) pin the bytes quiet() and keyed() make."""
import functools
import os

import numpy as np

import parity
from oracle import oracle as O
from tfrec_amd import api, capture, clock, envelope, sync, track

B = api.BLOCK_DEC
SEG = clock.SEG
GOLDEN = ("tfa_1", "tfa_2", "tfa_3", "tx22", "whb")
RATE = dict(tfa_1=38400, tfa_2=17240, tfa_3=9600, tx22=8842, whb=6000)
# the first six bytes of each run's golden telegram (tx22: slot 3's events)
TELEGRAMS = dict(tfa_2=("2dd496070960", "2dd498812225"), tfa_3=("2dd49144363d", "2dd496846244"), tx22=("2dd4a5920189", "2dd4acdb0681"))
WORD = 0x2DD4
# DESIGN.md 6u's table: per scene and run the plateau at E = 0 and E = 1 and the 32 bits read behind the sync word
PLATEAUS = dict(tfa_2=((520, 541), (521, 540)), tfa_3=((1571, 1606), (1570, 1609)), tx22=((1357, 1397), (1358, 1397)))
PAYLOADS = dict(tfa_2=("96070960", "98812225"), tfa_3=("9144363d", "96846244"), tx22=("a5920189", "acdb0681"))


# ---- hand-made rows for a channel-rate context
def quiet(nb, seed):
    return np.random.default_rng(seed).integers(-40, 41, size=(nb * B, 2)).astype(np.int16)


def loud(row, where, v=(3000, -3000)):
    for p in where:
        row[p] = v


def gap_ladder(start):
    """Over samples with gaps of 1, 63, 64 and 65 not-over samples between them."""
    out = [start]
    for g in (1, 63, 64, 65):
        out.append(out[-1] + g + 1)
    return out


def keyed(n_blocks, period, seed=1, amp=3000):
    """A two-tone signal whose frequency flips every `period` samples, with a little noise -> int16 [2 M]."""
    n = np.arange(n_blocks * B)
    f = np.where((n // period) % 2 == 0, 1.0, -1.0) * 0.12
    ph = np.cumsum(f)
    rng = np.random.default_rng(seed)
    z = amp * np.exp(2j * np.pi * ph) + rng.normal(0, 20, len(n)) + 1j * rng.normal(0, 20, len(n))
    return np.stack([np.rint(z.real), np.rint(z.imag)], axis=1).astype(np.int16).reshape(-1)


def silent_rows(n_blocks=1):
    """Every other sample (0, 0) with a large pair between: the trigger stays up while every product is zero."""
    z = np.zeros((n_blocks * B, 2), dtype=np.int16)
    z[1::2] = (3000, -2000)
    return z.reshape(-1)


def mx_rows():
    """Segments whose largest product is 2^15 - 1, 2^15, 2^16 - 1, 2^16 and 2^31, the two constants of the issue (dot = 32761 and
    33124), and the one sequence whose four factors are all -2^15: every product -65535 (1 + i), mx = 2^16 - 1."""
    z = np.zeros((B, 2), dtype=np.int16)

    def alternate(k, a, b):
        z[SEG * k:SEG * (k + 1):2], z[SEG * k + 1:SEG * (k + 1):2] = a, b

    alternate(0, (217, 0), (151, 0))  # 217 * 151 = 2^15 - 1
    alternate(1, (128, 128), (128, 128))  # 2 * 128^2 = 2^15
    alternate(2, (255, 0), (257, 0))  # 2^16 - 1
    alternate(3, (256, 0), (256, 0))  # 2^16
    alternate(4, (-32768, -32768), (-32768, -32768))  # 2^31
    alternate(5, (181, 0), (181, 0))
    alternate(6, (182, 0), (182, 0))
    w = complex(-257, 0)
    for m in range(SEG):  # z[m+1] conj(z[m]) = -65535 (1 + i)
        z[SEG * 7 + m] = (round(w.real), round(w.imag))
        w = -65535 * (1 + 1j) * w / abs(w) ** 2
    return z.reshape(-1)


def word_bits(word, n_bits):
    return [(word >> (n_bits - 1 - i)) & 1 for i in range(n_bits)]  # MSB first


def fsk(symbols, rate, amp=6000, dev=40000, phase=0.0):
    """A phase-continuous two-tone signal, +dev Hz for a 1, at `rate` bit/s -> int16 [n, 2]."""
    n = -(-384000 * len(symbols) // rate)
    idx = np.minimum(np.arange(n) * rate // 384000, len(symbols) - 1)
    f = np.where(np.asarray(symbols)[idx] != 0, dev, -dev)
    ph = phase + 2 * np.pi * np.cumsum(f) / 384000.0
    return np.stack([np.rint(amp * np.cos(ph)), np.rint(amp * np.sin(ph))], axis=1).astype(np.int16)


def frame_symbols(word, n_bits, seed, pre=16, pay=32, invert=False):
    rng = np.random.default_rng(seed)
    s = [1, 0] * (pre // 2) + word_bits(word, n_bits) + rng.integers(0, 2, pay).tolist()
    return [1 - x for x in s] if invert else s


# ---- the golden scenes
def golden_iq(name="tfa_2", nb=4):
    return np.load(os.path.join(parity.ROOT, "tests", "golden", "iq_%s.npz" % name))["iq"][None, :nb * api.BLOCK_BYTES]


@functools.lru_cache(maxsize=None)
def golden_dec(name):
    d = np.load(os.path.join(parity.ROOT, "tests", "golden", "iq_%s.npz" % name))["dec"]
    d.setflags(write=False)
    return d


def rotated(dec, hz):
    """The scene shifted by hz, rounded to int16.  The rounding adds 0.29 LSB rms to samples that stand above the threshold of 500:
    under 1e-3 of a product, so a reading moves by a Hz or two at most and quality_c by well under 1 per cent."""
    z = dec.reshape(-1, 2).astype(np.float64)
    y = (z[:, 0] + 1j * z[:, 1]) * np.exp(2j * np.pi * hz * np.arange(len(z)) / 384000.0)
    return np.clip(np.stack([np.rint(y.real), np.rint(y.imag)], axis=1), -32768, 32767).astype(np.int16).reshape(-1)


def submits(dec, sizes, L, centre=0, types=0x2F, thresh=500, brute=False):
    """The stream cut into submits of `sizes` blocks -> the track's [(records, words)], the recorder's, the thresholds' and the
    track's state carried from one to the next."""
    cst = est = tst = None
    pos, out = 0, []
    for nb in sizes:
        part = dec[2 * pos * B:2 * (pos + nb) * B]
        runs, _, cst = capture.captures(part, types, thresh, cst)
        thr, est = envelope.thresholds(part, types, thresh, est)
        form = track.tracks_bruteforce if brute else track.tracks
        recs, words, tst = form([part], [thr], runs, L, [centre], tst, base=[pos * B])
        out.append((recs, words))
        pos += nb
    return out


def bit_string(symbols):
    return "".join("01"[s] for s in symbols)


def pattern(hex48):
    return bin(int(hex48, 16))[2:].zfill(48)


@functools.lru_cache(maxsize=None)
def shifted_tfa_2():
    """The golden TFA_2 scene moved 5500 decimated samples back inside 6 blocks of silence, so that -b 2 makes three batches and
    both telegrams lie across a batch boundary -> (its bytes, the lines track.py expects of tfrec_gpu -G 17240 on a file named %s)."""
    x = np.full(6 * api.BLOCK_BYTES, 128, dtype=np.uint8)
    scene = golden_iq()[0]
    x[8 * 5500:8 * 5500 + len(scene)] = scene
    # the restatement: the oracle's front end (the context's, bit for bit), capture.py, envelope.py's thresholds and track.py submit
    # by submit (2 + 2 + 2)
    dec = parity.fresh_oracle(x, 0x2F, 500, keep_dec=True).dec().reshape(-1, 2)
    subs, cst, est, tst = [], None, None, None
    for a, b in ((0, 2), (2, 4), (4, 6)):
        part = dec[a * B:b * B].reshape(-1)
        runs, _, cst = capture.captures(part, 0x2F, 500, cst)
        thr, est = envelope.thresholds(part, 0x2F, 500, est)
        recs, words, tst = track.tracks([part], [thr], runs, 11, [0], tst, base=[a * B])
        subs.append((recs, words))
    cont = capture.RUN_CONTINUES
    assert any(c["flags"] & cont for c in subs[1][0]) and any(c["flags"] & cont for c in subs[2][0]), "a burst is not cut by the batches"
    chains = track.chains(subs)
    for c, tel in zip(chains, TELEGRAMS["tfa_2"]):
        assert pattern(tel) in bit_string(track.slice_bits(c.bits[:int(c["last_over"]) + 1], 17240)), "telegram %s is not in the slice" % tel
    return x, [track.line("%s", c, 17240) for c in chains]


# ---- what a comparison of chains, or of a record with the host's merge, is made on
def stripped(rec):
    return [int(rec[f]) for f in track.TRACK_DTYPE.names if f != "bit_offset"]  # (a piece's place in its own submit's pool)


def sync_stripped(rec):
    return [int(rec[f]) for f in sync.SYNC_DTYPE.names if f != "bit_offset"]  # (a piece's place in its own submit's pool)


def rec_line(f, r):
    """An envelope record as tests/merge_driver.cpp reads it."""
    v = [f] + [int(r[k]) for k in ("flags", "start_sample", "n_samples", "thresh", "n_over", "last_over", "energy_head", "energy_tail",
                                   "n_gaps", "max_gap", "lead_not_over", "nprod_head", "dot_head", "crs_head", "dot_tail", "crs_tail",
                                   "nprod_tail")]
    return "rec " + " ".join("%d" % x for x in v)


# ---- the aimed u8 scene of the squelched recorder (tests/test_capture_gpu.py lists what its eight streams hold)
NB = 4
M = NB * B
N = 8
TYPES = [0x2F, 0x2F, 0x02, 0x2F, 0x2F, 0x2F, 0x2F, 0x01]
THRESH = [500, 500, 500, 500, 500, 500, 0, 500]
CTX_TYPES = 0x2F


def oracle_runs(x, types, thresh):
    o = O.Oracle(types, thresh, 0, keep_dec=True)
    o.process(x)
    return capture.captures(o.dec(), types, thresh)[0]


def carrier(x, first, last):
    """raw complex samples [first, last) of the u8 stream x: a carrier at full scale on I."""
    x[2 * first:2 * last:2] = 228
    x[2 * first + 1:2 * last:2] = 128


def aim(base, place, measure, target, types, thresh, modulo=None):
    """Move a burst until measure(runs) == target (modulo: in that residue class).  The front end decimates by four and is time
    invariant, so one decimated sample is four raw ones: a few rounds, the noise around the edge permitting."""
    pos = 0
    for _ in range(12):
        x = base.copy()
        place(x, pos)
        got = measure(oracle_runs(x, types, thresh))
        d = target - got
        if modulo:
            d = (d + modulo // 2) % modulo - modulo // 2
        if d == 0:
            return x
        pos += 4 * d
    raise AssertionError("the burst did not settle")


@functools.lru_cache(maxsize=None)
def scene():
    rng = np.random.default_rng(17)
    n = NB * api.BLOCK_BYTES
    quiet = lambda: rng.integers(126, 131, n, dtype=np.uint8)  # noqa: E731
    end = lambda r: int(r["start_sample"] + r["n_samples"])  # noqa: E731
    rows = [quiet()]
    # 1: 300 decimated samples of carrier that end 100 ahead of block 2 -- the run crosses into it -- starting at bit 63 of a word
    rows.append(aim(quiet(), lambda x, p: carrier(x, 4 * (2 * B - 400) + p, 4 * (2 * B - 400) + p + 1200),
                    lambda r: int(r[0]["start_sample"]) % 64, 63, TYPES[1], THRESH[1], modulo=64))
    # 2: the burst's end moves until the run's last sample is bit 0 of a word
    rows.append(aim(quiet(), lambda x, p: carrier(x, 4 * 5000, 4 * 5300 + p), lambda r: (end(r[0]) - 1) % 64, 0, TYPES[2], THRESH[2],
                    modulo=64))
    for k, length in ((3, 1), (4, 3), (5, 5)):
        rows.append(aim(quiet(), lambda x, p: carrier(x, 4 * (M - 40) + p, n // 2), lambda r: int(r[-1]["start_sample"]), M - length,
                        TYPES[k], THRESH[k]))
    rows.append(rng.integers(0, 256, n, dtype=np.uint8))
    rows.append(rows[1].copy())
    iq = np.stack(rows)
    iq.setflags(write=False)
    return iq


def want_tables(decs, states):
    """The restatement on one submit's decimated samples -> (table, pool); states: each stream's carried state, updated.  Stream s
    has the settings of the scene's row s mod N."""
    per = []
    for s, d in enumerate(decs):
        runs, pool, states[s] = capture.captures(d, TYPES[s % N], THRESH[s % N], states[s])
        per.append((runs, pool))
    return capture.table(per)
