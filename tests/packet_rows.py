"""The inputs the packet check's tests share (tests/test_packet_cpu.py, tests/test_packet_gpu.py), none of which needs a
GPU: the settings table, rows with packets planted by construction, and the restatements run submit by submit.  Imported as a plain
module (`import packet_rows`)."""
import functools

import numpy as np

import crc_rows as CR
import linecode_rows as LR
import recorder as R
import recorder_rows as RR
from tfrec_amd import api, decin, packet, sync

B = api.BLOCK_DEC
L = 11  # the track's smoothing in every case
WORD, P = 0x2DD4, 16

# the settings of the tests: packet.Settings' arguments
#   cc1101  the CC1101's packet engine: CRC-16 0x8005 from 0xFFFF over the length byte and the payload, PN9, MSB-first
#   plain   CRC-16/GENIBUS on complemented bits, no whitening; a symbol is 80 samples; len_max = 20 reaches 14720
#   crc8    a byte behind the length byte that the length does not count, and the length byte itself not covered; LSB-first
#   reach   T_max = 32 at 6001 bit/s: delta(8 T_max) = 16381 (6000: 16384, refused)
SETS = {"cc1101": dict(rate=38400, len_max=160, width=16, poly=0x8005, init=0xFFFF, whiten=packet.pn9(274)),
        "plain": dict(rate=4800, len_max=20, len_min=1, width=16, poly=0x1021, init=0xFFFF, xorout=0xFFFF, invert=True),
        "crc8": dict(rate=17240, len_max=40, len_min=0, len_add=1, skip=1, width=8, poly=0x31, lsb=True),
        "reach": dict(rate=6001, len_max=30, width=8, poly=0x07)}


def settings(name):
    return packet.Settings(**SETS[name])


def sync_settings(st):
    return sync.Settings(st.rate, WORD, P, 0)


def symbols(st, L_byte, seed, pre=24, post=12, flip=None, cut=None):
    """`pre` random symbols, the sync word, a packet that checks whose length byte is L_byte (any: L_byte + len_add random bytes
    follow it) as it stands on the air, `post` random symbols -> (the symbols, the packet's de-whitened bytes).  flip: an on-air
    packet bit (0: the length byte's first) that is complemented.  cut: only the first `cut` on-air packet bits are sent, and
    nothing behind them.  The seeds are chosen so that the restatement alone reports exactly the planted packets
    (tests/test_packet_cpu.py asserts it)."""
    rng = np.random.default_rng(2000 + seed)
    data = st.packet_of(rng.integers(0, 256, L_byte + st.add).astype(np.uint8).tobytes())
    bits = st.on_air(data)
    if flip is not None:
        bits[flip] ^= 1
    head = rng.integers(0, 2, pre).tolist() + RR.word_bits(WORD, P)
    if cut is not None:
        return head + bits[:cut], data
    return head + bits + rng.integers(0, 2, post).tolist(), data


def word_end(st, pre):
    """The samples from a plant's first to the end of its sync word's last symbol."""
    return CR.edges(st.rate, pre + P)[-1]


def row(nb, seed, st, plants):
    """int16 [nb B, 2]: quiet, with an FSK transmission of each (at, symbols) of plants from sample at."""
    x = RR.quiet(nb, seed)
    for at, sym in plants:
        s = RR.fsk(sym, st.rate)[:CR.edges(st.rate, len(sym))[-1]]
        assert at >= 0 and at + len(s) <= len(x)
        x[at:at + len(s)] = s
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def case(name, kind, arg=None):
    """A planted row of the settings `name` -> (the settings, int16 [n, nb B, 2], per stream the planted packet's bytes, or None
    where nothing that checks is planted).
      whole       a packet of middling length inside the first block
      across      its sync word ends two samples ahead of the block boundary: in one-block submits the word lies in the carried
                  history and the length byte in the next submit ("reach": T = T_max, whose bits lie in three pieces)
      length      (arg = L) a packet with that length byte
      end         a packet whose ok plateau holds the last sample of block 0 and the first of block 1
      cut         the burst ends behind the packet's second byte: never evaluated
      flip        (arg = the on-air bit) one complemented bit
      three       three streams: a whole packet, one across the boundary, a flipped one"""
    st = settings(name)
    mid = {"cc1101": 9, "plain": 3, "crc8": 5, "reach": 2}[name]
    if kind == "whole":
        return st, row(2, 71, st, [(300, symbols(st, mid, 1)[0])])[None], [symbols(st, mid, 1)[1]]
    if kind == "across":
        Lb = st.len_max if name == "reach" else mid
        sym, data = symbols(st, Lb, 2)
        nb = -(-(B + CR.edges(st.rate, 8 * st.total(Lb) + 12)[-1]) // B)
        return st, row(nb, 72, st, [(B - 2 - word_end(st, 24), sym)])[None], [data]
    if kind == "length":
        sym, data = symbols(st, arg, 3 + arg)
        return st, row(3, 73, st, [(300, sym)])[None], [data if st.len_min <= arg <= st.len_max else None]
    if kind == "end":
        sym, data = symbols(st, mid, 4)
        k = word_end(st, 24) - 192000 // st.rate + packet.delta(st.rate, 8 * st.total(mid))  # the end, from the plant's first sample
        return st, row(2, 74, st, [(B - k - 192000 // st.rate, sym)])[None], [data]
    if kind == "cut":
        sym, _ = symbols(st, {"cc1101": 30, "plain": 3, "crc8": 20, "reach": 10}[name], 5, cut=16)  # (the rest outlasts the trigger's hold)
        return st, row(2, 75, st, [(300, sym)])[None], [None]
    if kind == "flip":
        sym, _ = symbols(st, mid, 6, flip=arg)
        return st, row(2, 76, st, [(300, sym)])[None], [None]
    assert kind == "three"
    rows = [case(name, "whole")[1][0], case(name, "across")[1][0][:2 * B], case(name, "flip", 20)[1][0]]
    return st, np.stack(rows), [case(name, "whole")[2][0], case(name, "across")[2][0], None]


def restated(st, rows, sizes):
    """The restatements on the rows, one stream at a time, in submits of `sizes` blocks -> per stream (the track's submits, the
    sync's, the packet check's), each [(records, words)]."""
    out = []
    for x in rows:
        tsubs = RR.submits(decin.clamp(x[None])[0].reshape(-1), sizes, L, thresh=R.T)
        ssubs = LR.sync_submits(tsubs, sync_settings(st))
        state, vsubs = None, []
        for (tr, tw), (sr, sw) in zip(tsubs, ssubs):
            v, w, state = packet.packets(tr, tw, sr, sw, st, state, 1)
            vsubs.append((v, w))
        out.append((tsubs, ssubs, vsubs))
    return out


# ---- tfrec_gpu -G 38400 -Y 2dd4,0,8 -V 16,8005,ffff -N 160,0,0,pn9
CLI_ARGS = ["-G", "38400", "-Y", "2dd4,0,8", "-V", "16,8005,ffff", "-N", "160,0,0,pn9"]


@functools.lru_cache(maxsize=None)
def cli_scene():
    """Three u8 recordings at 1.536 MS/s of two blocks each, read with -b 1 as three streams: RR.fsk transmissions of the "cc1101"
    settings -- a packet inside the first block, one whose sync word ends at the batch boundary (its length byte lies in the second
    batch), and one with a flipped payload bit -> (their bytes, per recording the lines the restatements expect of tfrec_gpu with
    CLI_ARGS on a file named %s: per burst its bits line, its frame lines, its packet lines and its pkts line)."""
    import parity
    from tfrec_amd import track
    st = settings("cc1101")
    sst, Ls = sync_settings(st), track.smooth_of(st.rate)
    plants = [(symbols(st, 9, 11)[0], 3000), (symbols(st, 40, 12)[0], B - 12 - word_end(st, 24)), (symbols(st, 9, 13, flip=20)[0], 2000)]
    xs, wants = [], []
    for sym, at in plants:
        x = (127 + np.arange(2 * api.BLOCK_BYTES) * 7919 % 3).astype(np.uint8)
        s = RR.fsk(sym, st.rate // 4, amp=100, dev=10000)  # (four input samples a decimated one: the same symbols and tones)
        x[8 * at:8 * at + 2 * len(s)] = (128 + s).reshape(-1)
        dec = parity.fresh_oracle(x, 0x2F, 500, keep_dec=True).dec().reshape(-1)
        tsubs = RR.submits(dec, (1, 1), Ls)
        ssubs = LR.sync_submits(tsubs, sst)
        state, vsubs = None, []
        for (tr, tw), (sr, sw) in zip(tsubs, ssubs):
            v, w, state = packet.packets(tr, tw, sr, sw, st, state, 1)
            vsubs.append((v, w))
        want = []
        for t, s_, v in zip(track.chains(tsubs), sync.chains(ssubs), packet.chains(vsubs)):
            want.append(track.line("%s", t, st.rate))
            want += [sync.line("%s", s_, f) for f in sync.frames(t, s_, sst, 8)]
            want += [packet.line("%s", v, item) for item in packet.read(t, s_, v, st)]
            want.append(packet.summary_line("%s", v))
        xs.append(x)
        wants.append(want)
    return xs, wants
