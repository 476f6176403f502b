"""The inputs the frame check's tests share (tests/test_crc_cpu.py, tests/test_crc_gpu.py), none of which needs a GPU:
the settings the GPU tests run, tracks with frames planted by construction, the restatement run submit by submit, and the figures
the feature was specified with.  Imported as a plain module (`import crc_rows`)."""
import numpy as np

import linecode_rows as LR
import phase_rows as P
import recorder_rows as RR
from tfrec_amd import api, crc, linecode, sync, track

B = api.BLOCK_DEC

# the settings of the GPU tests: crc.Settings' arguments (rate, N, W, poly, init, xorout, skip, lsb, invert)
#   crc8   the TFA_2 family's: D = 891
#   whb    WHB's: D = 11776, above a block -- in one-block submits a frame's bits lie in three pieces, and 64 carried words would not do
#   ccitt  CRC-16/GENIBUS on complemented bits: D = 320
#   crc24  OpenPGP's polynomial and init, LSB-first bytes behind a skipped one: D = 1920
#   reach  the largest reach there is: N = 32 at 6001 bit/s is D = 16381 (6000: 16384, refused)
SETS = {"crc8": (17240, 5, 8, 0x31), "whb": (6000, 23, 32, 0x04C11DB7, 0xF59C5A1E, 0, 1, True),
        "ccitt": (38400, 4, 16, 0x1021, 0xFFFF, 0xFFFF, 0, False, True), "crc24": (9600, 6, 24, 0x864CFB, 0xB704CE, 0, 1, True, False),
        "reach": (6001, 32, 8, 0x07)}
REACH = {"crc8": 891, "whb": 11776, "ccitt": 320, "crc24": 1920, "reach": 16381}

# the issue's table: scene -> (track mode, sync word, LSB-first bytes, [(N, per burst the sync centre c, per burst whether the CRC
# holds)]); the frequency scenes check crc8(0x31) over all but the last byte, WHB crc32 with its type's init behind a skipped byte
GOLDEN = {"tfa_2": ("fsk", 0x2DD4, False, [(5, (530, 530), (True, True))]),
          "tfa_3": ("fsk", 0x2DD4, False, [(5, (1588, 1589), (True, True))]),
          "tx22": ("fsk", 0x2DD4, False, [(7, (1377, 1377), (True, False)), (9, (1377, 1377), (False, True))]),
          "tfa_1": ("psk", 0xB42B, True, [(9, (2157, 2158), (True, True))]),
          "whb": ("psk+g3ruh", 0xB42B, True, [(23, (14312,), (True,))])}
GOLDEN_FRAMES = {"tfa_2": ("960709605b", "9881222530"), "tfa_3": ("9144363de8", "9684624449"),
                 "tx22": ("a59201891079f1", "acdb06811035233b1a"), "tfa_1": ("3dc488941c6010566e", "7fd682573a60d05660"),
                 "whb": ("2b1603a290d9d3cf962a73e1ec2a34c87390cc8e5308a0",)}
GOLDEN_D = {("tfa_2", 5): 891, ("tfa_3", 5): 1600, ("tx22", 7): 2432, ("tx22", 9): 3127, ("tfa_1", 9): 720, ("whb", 23): 11776}
WHB_N_OK, WHB_FIRST_AT = 64, 26057


def settings(name):
    return crc.Settings(*SETS[name])


def golden_settings(name, N):
    if name == "whb":
        return crc.Settings(6000, N, 32, 0x04C11DB7, 0xF59C5A1E, 0, 1, True)
    return crc.Settings(RR.RATE[name], N, 8, 0x31, lsb=GOLDEN[name][2])


def golden_tracks(name, sizes=None):
    """The sync's input track of a golden scene, by the restatements -> [(records, words)] per submit of `sizes` blocks (default:
    one submit of every whole block)."""
    d = RR.golden_dec(name)
    nb = len(d) // (2 * B)
    sizes = sizes or (nb,)
    if GOLDEN[name][0] == "fsk":
        return RR.submits(d, sizes, track.smooth_of(RR.RATE[name]))
    rate, m, L = P.GOLDEN[name][:3]
    tsubs = [s[1:] for s in P.submits(d, sizes, L, m)]
    return LR.code_submits(tsubs, linecode.g3ruh(rate)) if name == "whb" else tsubs


def crc_submits(tsubs, st, brute=False, n_streams=1, state=None, max_samples=None):
    """Input submits [(records, words)] -> the check's [(records, words)], the state carried from one to the next."""
    out = []
    for recs, words in tsubs:
        r, w, state = (crc.crcs_bruteforce if brute else crc.crcs)(recs, words, st, state, n_streams, max_samples)
        out.append((r, w))
    return out


def frame_bits(st, frame):
    """A frame's bytes -> its 8 N bits in the order received, as they stand on the track (INVERT undone)."""
    inv = 1 if st.invert else 0
    return [((x >> (q if st.lsb else 7 - q)) & 1) ^ inv for x in frame for q in range(8)]


def bytes_of(st, bits):
    """8 N track bits in the order received -> the frame's bytes."""
    inv = 1 if st.invert else 0
    return bytes(st.byte_of([b ^ inv for b in bits[j:j + 8]]) for j in range(0, len(bits), 8))


def random_frame(st, seed):
    """N bytes that check: random bytes with their CRC appended."""
    data = [int(x) for x in np.random.default_rng(seed).integers(0, 256, st.N - st.W // 8)]
    return bytes(data) + st.field_of(data)


def edges(rate, n):
    """Symbol i of a held track occupies the samples [edges[i], edges[i + 1])."""
    return [(384000 * i) // rate for i in range(n + 1)]


def planted_symbols(st, seed, pre=40, post=12, flip=None):
    """`pre` random symbols, the frame of random_frame(st, seed) as it stands on the track, `post` random symbols -> (the symbols,
    the frame).  flip: a payload bit (1 .. 8 N) that is complemented.  The symbols next to the frame are chosen so that the frame
    read a symbol early or late does not check -- with init = xorout = all ones a frame moved by a bit still checks when the bit it
    loses and the bit it gains are both 1: (x + 1) times the all-ones word is x^(8 N) + 1."""
    rng = np.random.default_rng(1000 + seed)
    frame = random_frame(st, seed)
    bits = frame_bits(st, frame)
    if flip is not None:
        bits[flip - 1] ^= 1
    symbols = rng.integers(0, 2, pre).tolist() + bits + rng.integers(0, 2, post).tolist()
    for at, nb in ((pre - 1, pre - 1), (pre + 1, pre + len(bits))):  # the frame read a symbol early or late: if it checks, flip its new bit
        if 0 <= nb < len(symbols) and at >= 0 and st.check(bytes_of(st, symbols[at:at + len(bits)])):
            symbols[nb] ^= 1
    return symbols, frame


def planted(st, seed, pre=40, post=12, flip=None):
    """A held-symbol track of planted_symbols -> (the track, the frame, c: the centre of the last symbol ahead of the frame -- where
    a sync word's plateau would have its sample).  The frame's bit i is read at c + delta(i), inside symbol pre + i - 1; k = c + D is
    the centre of its last bit."""
    symbols, frame = planted_symbols(st, seed, pre, post, flip)
    e = edges(st.rate, len(symbols))
    t = np.repeat(np.asarray(symbols, dtype=np.uint8), np.diff(e))
    c = (384000 * (2 * pre - 1)) // (2 * st.rate)  # floor of the centre of symbol pre - 1
    return t, frame, c


def frame_at(st, t, k):
    """The N bytes whose last bit sits at sample k of the track t."""
    return bytes_of(st, [int(t[k - o]) for o in st.offs])


def stretch(v, k):
    """The maximal run of ones of v that holds k -> (first, last), or None."""
    if not v[k]:
        return None
    a = b = k
    while a > 0 and v[a - 1]:
        a -= 1
    while b + 1 < len(v) and v[b + 1]:
        b += 1
    return a, b


# ---- hand-made rows for the GPU tests (channel-rate contexts; threshold 100, the floor stays below it)
def planted_rows():
    """int16 [3, 3 B, 2] and what is planted in them.  Stream 0: an FSK transmission at 6000 bit/s from B - 1000 to 2 B + 3000, four
    symbols and then a frame of the "whb" settings (184 symbols of 64 samples): in submits of one block a chain of three pieces
    whose last holds the frame's last bit, 11776 samples behind its first.  Stream 1: at 17240 bit/s from B - 600 a frame of the
    "crc8" settings behind 20 symbols, across the block boundary.  Stream 2: at 6001 bit/s from sample 500 four symbols and a frame of the
    "reach" settings, 256 symbols: its last bit lies in the third block, 16381 samples behind the sync's centre in the first -- the
    largest reach there is -> (the rows, {stream: (the settings' name, the frame)})."""
    rows = np.stack([RR.quiet(3, 55), RR.quiet(3, 56), RR.quiet(3, 57)])
    sym, whb = planted_symbols(settings("whb"), 21, pre=4, post=8)
    n = B + 4000
    rows[0, B - 1000:B - 1000 + n] = RR.fsk(sym, 6000)[:n]
    sym, crc8 = planted_symbols(settings("crc8"), 22, pre=20, post=8)
    x = RR.fsk(sym, 17240)[:(len(sym) - 1) * 384000 // 17240]
    rows[1, B - 600:B - 600 + len(x)] = x
    sym, reach = planted_symbols(settings("reach"), 23, pre=4, post=12)
    x = RR.fsk(sym, 6001)[:(len(sym) - 1) * 384000 // 6001]
    rows[2, 500:500 + len(x)] = x
    rows.setflags(write=False)
    return rows, {0: ("whb", whb), 1: ("crc8", crc8), 2: ("reach", reach)}


# ---- tfrec_gpu -G 6000,psk -U g3ruh -Y b42b,0,23,0,1 -V 32,04c11db7,f59c5a1e,0,1
CLI_ARGS = ["-G", "6000,psk", "-U", "g3ruh", "-Y", "b42b,0,23,0,1", "-V", "32,04c11db7,f59c5a1e,0,1"]


def cli_scene():
    """linecode_rows.cli_scene()'s recording -- the golden WHB scene moved 9000 decimated samples on inside 8 blocks -- read with -b 1:
    eight batches, the burst is cut three times and the frame's bits lie in two batches behind the one with its sync word -> (its
    bytes, the lines the restatements expect of tfrec_gpu with CLI_ARGS on a file named %s: per burst its centre line, its bits
    line, its code line, its frame lines with their verdicts and its crc line)."""
    import parity
    x = LR.cli_scene()[0]
    dec = parity.fresh_oracle(x, 0x2F, 500, keep_dec=True).dec().reshape(-1)
    subs = P.submits(dec, (1,) * 8, track.smooth_of(LR.CLI_RATE), track.lag_of(LR.CLI_RATE))
    sst, st = sync.Settings(LR.CLI_RATE, LR.WORD, 16, 0), golden_settings("whb", 23)
    csubs = LR.code_submits([s[1:] for s in subs], linecode.g3ruh(LR.CLI_RATE))
    ssubs, vsubs = LR.sync_submits(csubs, sst), crc_submits(csubs, st)
    assert sum(1 for recs, _ in csubs for r in recs if r["flags"] & LR.CONT) >= 2, "the burst is not cut twice by the batches"
    cen, trk = P.chains(subs)
    want = []
    for c, t, u, s, v in zip(cen, trk, linecode.chains(csubs), sync.chains(ssubs), crc.chains(vsubs)):
        fr = sync.frames(u, s, sst, 23, lsb=True)
        want += [track.centre_line("%s", c), track.line("%s", t, LR.CLI_RATE), linecode.line("%s", u, LR.CLI_RATE)]
        want += [sync.line("%s", s, f) + " " + w for f, w in zip(fr, crc.verdicts(fr, v, st))]
        want.append(crc.line("%s", v, st))
    return x, want
