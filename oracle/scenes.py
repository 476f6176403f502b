"""Scene families: hand-placed inputs for the window geometry and the state that crosses windows -- TEST INFRASTRUCTURE.

Three kinds of rows, all integer-only (the bytes are the same on every machine):
  scene  -- tfrec_amd.synth.gen_scene over an explicit burst list (repeats, collisions, clock offsets, levels, hand-built
            frames; iq_swap: I and Q exchanged, every FSK deviation negated);
  comb   -- copies of one short pulse pasted so that the trigger test |I| + |Q| > thresh (fm_demod.cpp:45,
            frontend.hip:8) fires on chosen decimated samples (dense windows, block and submit edges);
  splice -- a scene cut open by stretches of silence, the rest shifted back (a burst's parts in separate trigger windows).

A family is a list of rows run as one batch.  oracle/mint_golden.py pins a subset against the real reference
(tests/golden/scenes.json); tests/test_scenes_cpu.py and tests/test_gpu_scenes.py replay them.  The last two families,
frames and splices, are about the decoders' carried state: tests/test_carried_cpu.py measures their classes,
tests/test_carried_gpu.py runs them through reset, save / load and tfrec_gpu.
"""
from __future__ import annotations

import numpy as np

from tfrec_amd import synth

BLOCK_DEC = 8192                   # decimated samples per 65536-byte block
# trigger windows per chain (capi.hip ChainParams::window): TFA_1 40*BITPERIOD, TFA_2 / TFA_3 / TX22 (int)(16*spb),
# WHB 8*spb (spb = 384000 / baud)
WINDOW = {0: 400, 1: 356, 2: 640, 3: 694, 4: 512}
THRESH = 500

# "dot": one input sample of +47 LSB on both rails at an input sample 4k; with the narrow filter and thresh 500 exactly one
# decimated sample triggers, k + 5 (pulse() measures it on the decimator)
DOT_AMP = 47


def table_sizes(m: int) -> dict:
    """The window tables capi.hip sizes for M decimated samples per submit."""
    cap = m // 356 + 2
    return dict(cap=cap, slots=m // 32 + cap + 2, bit_words=m // 64 + 3 * cap + 8, whbrec=m // 64 + 2 * cap + 2)


def _pulse_bytes(kind: str) -> np.ndarray:
    """One pulse as u8 IQ bytes, starting at an input sample that is a multiple of 4 (the decimation phase is fixed)."""
    if kind == "dot":
        return np.array([128 + DOT_AMP, 128 + DOT_AMP], np.uint8)
    if kind == "fsk":
        # a TFA_2 burst with a one-byte frame (8 preamble bits, 8 bits, tail): ~400 triggered samples that carry edges
        iq = synth.gen_scene(1, 1, [dict(proto=1, start=256, frame=b"\x2d", amp=40, f0_hz=3000)], noise_q8=0)
        nz = np.nonzero(iq.reshape(-1, 2).astype(int).sum(1) != 256)[0]
        return iq[2 * 256: 2 * (int(nz[-1]) + 1)].copy()
    raise ValueError(kind)


_PULSES: dict = {}


def pulse(kind: str):
    """(bytes, first trigger offset, last trigger offset): triggers relative to the decimated sample input_pos / 4."""
    if kind not in _PULSES:
        from oracle import oracle as O

        b = _pulse_bytes(kind)
        iq = np.full(2 * 32768, 128, np.uint8)
        p0 = 4096
        iq[2 * p0: 2 * p0 + b.size] = b
        d = np.empty(2 * 8192, np.int16)
        O.lib().orc_decimate(iq.ctypes.data, 32768, 0, d.ctypes.data)
        trig = np.nonzero(np.abs(d.reshape(-1, 2).astype(int)).sum(1) > THRESH)[0] - p0 // 4
        _PULSES[kind] = (b, int(trig[0]), int(trig[-1]), trig)
    return _PULSES[kind][:3]


def pulse_triggers(kind: str) -> np.ndarray:
    pulse(kind)
    return _PULSES[kind][3]


def comb_firsts(spec) -> list:
    """Decimated samples on which the pulses' first trigger falls."""
    if "at" in spec:
        return list(spec["at"])
    _, f, l = pulse(spec["pulse"])
    m = spec["n_blocks"] * BLOCK_DEC
    gaps = spec["gaps"]
    out, t, k = [], spec["first"], 0
    while t + (l - f) < m - spec.get("tail", 0):
        out.append(t)
        t += (l - f) + gaps[k % len(gaps)]  # gap = next first trigger - this pulse's last trigger
        k += 1
    return out


def render_comb(spec) -> np.ndarray:
    b, f, _ = pulse(spec["pulse"])
    n = spec["n_blocks"] * 65536
    iq = np.full(n, 128, np.uint8)
    for t in comb_firsts(spec):
        pos = 4 * (t - f)
        assert pos >= 0 and 2 * pos + b.size <= n, (spec, t)
        iq[2 * pos: 2 * pos + b.size] = b
    return iq


def render_splice(spec) -> np.ndarray:
    """spec["base"] rendered, then cut open: at every input sample `at` of spec["cuts"] = [[at, n], ...] (positions in the base,
    ascending, at and n multiples of 4: the decimation phase of what follows is kept) n samples of silence (0x80) are inserted and
    the rest is shifted back; what no longer fits the row is dropped.  spec["dots"]: input samples of the spliced row (multiples
    of 4, inside silence) that get a dot pulse, each a trigger window that hands the decoders nothing."""
    base = render(spec["base"]).reshape(-1, 2)
    n = spec["n_blocks"] * 32768
    parts, pos = [], 0
    for at, gap in spec["cuts"]:
        assert at % 4 == 0 and gap % 4 == 0 and pos <= at <= len(base), spec["name"]
        parts += [base[pos:at], np.full((gap, 2), 128, np.uint8)]
        pos = at
    parts.append(base[pos:])
    iq = np.concatenate(parts)
    assert len(iq) >= n and not (iq[n:] != 128).any(), spec["name"]  # only silence falls off the end
    iq = np.ascontiguousarray(iq[:n])
    for at in spec.get("dots", ()):
        assert at % 4 == 0 and (iq[at - 64:at + 64] == 128).all(), spec["name"]
        iq[at] = 128 + DOT_AMP
    return iq.reshape(-1)


def render(spec) -> np.ndarray:
    if spec["kind"] == "comb":
        return render_comb(spec)
    if spec["kind"] == "splice":
        return render_splice(spec)
    # (a hand-built frame is written as hex digits, so that a spec stays plain JSON)
    bursts = [dict(b, frame=bytes.fromhex(b["frame"])) if isinstance(b.get("frame"), str) else b for b in spec["bursts"]]
    iq = synth.gen_scene(spec["seed"], spec["n_blocks"], bursts, spec.get("noise_q8", 256), tuple(spec.get("dc_iq", (0, 0))))
    if spec.get("iq_swap"):
        iq = iq.reshape(-1, 2)[:, ::-1].reshape(-1).copy()  # Q, I: the spectrum mirrored, every FSK deviation negated
    return iq


def render_batch(rows) -> np.ndarray:
    n = {r["n_blocks"] for r in rows}
    assert len(n) == 1
    return np.stack([render(r) for r in rows])


def events_digest(events) -> str:
    """sha256 over flush events (slot, end_sample, byte_cnt, rssi_db, offset, rdata), per slot in flush order: how
    tests/golden/scenes.json pins the reference's events without storing every 64-byte rdata."""
    import hashlib

    lines = ["%d %d %d %d %d %s" % (e[0], e[1], e[2], e[3], e[4], bytes(e[5]).hex())
             for e in sorted(events, key=lambda e: e[0])]
    return hashlib.sha256("\n".join(lines).encode()).hexdigest()


def flush_counts(events) -> list:
    return [sum(1 for e in events if e[0] == slot) for slot in range(5)]


# ------------------------------------------------------------------------------------------------ families

def _dense():
    rows = []
    for slot, w in sorted(WINDOW.items()):
        # tightest packing for this chain: every window a single trigger sample, next one W after it
        rows.append(dict(kind="comb", name="dense_w%d_exact" % w, n_blocks=24, pulse="dot", first=7, gaps=[w]))
        # W-2 .. W+2 in turn: merges (gap < W) next to splits (gap >= W), the close rule first > last + W - 1
        rows.append(dict(kind="comb", name="dense_w%d_pm2" % w, n_blocks=24, pulse="dot", first=9,
                         gaps=[w - 2, w - 1, w, w + 1, w + 2]))
    # combs that carry bits: FSK pulses of the TFA_2 family at its W and just around it
    rows.append(dict(kind="comb", name="dense_fsk_w356", n_blocks=24, pulse="fsk", first=11, gaps=[356]))
    rows.append(dict(kind="comb", name="dense_fsk_pm2", n_blocks=24, pulse="fsk", first=6, gaps=[354, 355, 356, 357, 358]))
    return rows


def _edges():
    n_blocks = 12
    rows = []
    last = n_blocks * BLOCK_DEC - 1
    # first trigger on a block's decimated sample 0 / 1 / 2, its last sample, and the last sample of every submit of the
    # cut 1 | 2 | 5 | 4 blocks (tests/test_gpu_scenes.py), each with and without an FSK pulse that opens a window there
    cuts = [1, 3, 8, 12]
    for k, off in enumerate((0, 1, 2)):
        at = [b * BLOCK_DEC + off for b in range(1, n_blocks)]
        rows.append(dict(kind="comb", name="edge_dot_block_sample%d" % off, n_blocks=n_blocks, pulse="dot", at=at))
        at = [b * BLOCK_DEC + off for b in range(1, n_blocks, 2)]
        rows.append(dict(kind="comb", name="edge_fsk_block_sample%d" % off, n_blocks=n_blocks, pulse="fsk", at=at))
    rows.append(dict(kind="comb", name="edge_dot_block_last", n_blocks=n_blocks, pulse="dot",
                     at=[b * BLOCK_DEC - 1 for b in range(1, n_blocks + 1)]))
    rows.append(dict(kind="comb", name="edge_dot_submit_last", n_blocks=n_blocks, pulse="dot",
                     at=[c * BLOCK_DEC - 1 - d for c in cuts for d in (0, 200)]))
    _, f, l = pulse("fsk")
    rows.append(dict(kind="comb", name="edge_fsk_across_cuts", n_blocks=n_blocks, pulse="fsk",
                     at=[c * BLOCK_DEC - (l - f) // 2 for c in cuts[:-1]] + [last - 2000]))
    # a window held open across a whole submit by a trigger every W-1 samples (the timeout carry, twice)
    rows.append(dict(kind="comb", name="edge_dot_held_open", n_blocks=n_blocks, pulse="dot", first=BLOCK_DEC // 2,
                     gaps=[355], tail=4 * BLOCK_DEC))
    return rows


def _frames_burst(proto, start, seed, **kw):
    return dict(proto=proto, start=start, payload_seed=seed, **kw)


def _repeats():
    rows = []
    for proto in range(5):
        w = WINDOW[proto]
        for tag, gap in (("one_window", 4 * w // 2), ("split", 4 * (w + 40))):
            rows.append(dict(kind="scene", name="repeat_%s_%s" % (synth.PROTO_NAMES[proto].lower(), tag), seed=100 + proto,
                             n_blocks=24, noise_q8=256,
                             bursts=[_frames_burst(proto, 30000, 7 + proto, amp=60, f0_hz=-2000, repeats=3,
                                                   repeat_gap=gap)]))
    # short gaps of a few bits: the decoder re-syncs while synced, WHB's level stays frozen over the whole span
    rows.append(dict(kind="scene", name="repeat_whb_tight", seed=120, n_blocks=24, noise_q8=256,
                     bursts=[_frames_burst(4, 20000, 21, amp=70, repeats=3, repeat_gap=300)]))
    rows.append(dict(kind="scene", name="repeat_tfa1_tight", seed=121, n_blocks=24, noise_q8=256,
                     bursts=[_frames_burst(0, 20000, 22, amp=70, repeats=4, repeat_gap=40)]))
    rows.append(dict(kind="scene", name="repeat_tx22_tight", seed=122, n_blocks=24, noise_q8=256,
                     bursts=[_frames_burst(3, 20000, 23, amp=70, repeats=4, repeat_gap=90)]))
    return rows


def _collisions():
    rows = []
    pairs = [
        # (a, b, start offset of b in input samples, amp a, amp b, f0 a, f0 b)
        (0, 1, 0, 60, 60, 0, 0),
        (1, 4, 3000, 70, 50, -8000, 9000),
        (2, 3, 1500, 60, 60, 2000, 2000),
        (4, 0, 20000, 90, 25, 0, -5000),
        (1, 2, 500, 100, 15, 0, 0),
        (3, 1, 8000, 20, 90, 5000, -5000),
        (0, 4, 60000, 50, 50, 7000, -7000),
        (2, 4, 0, 40, 80, 0, 12000),
    ]
    for k, (a, b, off, aa, ab, fa, fb) in enumerate(pairs):
        bursts = [_frames_burst(a, 30000, 40 + k, amp=aa, f0_hz=fa), _frames_burst(b, 30000 + off, 60 + k, amp=ab, f0_hz=fb),
                  # and a clean copy of both later on, for contrast
                  _frames_burst(a, 450000, 40 + k, amp=aa, f0_hz=fa), _frames_burst(b, 620000, 60 + k, amp=ab, f0_hz=fb)]
        rows.append(dict(kind="scene", name="collide_%s_%s" % (synth.PROTO_NAMES[a].lower(), synth.PROTO_NAMES[b].lower()),
                         seed=200 + k, n_blocks=32, noise_q8=256, bursts=bursts))
    return rows


DRIFT_PPM = (5000, 10000, 20000, 30000)
DRIFT_BEYOND = 80000


def _drift():
    rows = []
    for proto in range(5):
        for sign in (1, -1):
            bursts, pos = [], 20000
            ppms = [sign * p for p in DRIFT_PPM] + ([sign * DRIFT_BEYOND] if sign > 0 else [])
            for k, ppm in enumerate(ppms):
                bursts.append(_frames_burst(proto, pos, 80 + 10 * proto + k, amp=55, f0_hz=1000 * k - 2000, baud_ppm=ppm))
                pos += synth.burst_length(proto, 49 if proto == 4 else 15, ppm) + 12000
            rows.append(dict(kind="scene", name="drift_%s_%s" % (synth.PROTO_NAMES[proto].lower(), "fast" if sign > 0 else "slow"),
                             seed=300 + 2 * proto + (sign < 0), n_blocks=32, noise_q8=256, bursts=bursts))
    return rows


def _levels():
    rows = []
    for proto in range(5):
        # clipping: the carrier far beyond the 8-bit range
        rows.append(dict(kind="scene", name="clip_%s" % synth.PROTO_NAMES[proto].lower(), seed=400 + proto, n_blocks=16,
                         noise_q8=256, bursts=[_frames_burst(proto, 30000, 90 + proto, amp=220, f0_hz=4000),
                                               _frames_burst(proto, 260000, 95 + proto, amp=150, f0_hz=-4000)]))
        # weak: |I| + |Q| around thresh, the trigger flickers inside the burst with gaps around W
        rows.append(dict(kind="scene", name="weak_%s" % synth.PROTO_NAMES[proto].lower(), seed=410 + proto, n_blocks=16,
                         noise_q8=384, bursts=[_frames_burst(proto, 30000, 100 + proto, amp=6.5),
                                               _frames_burst(proto, 260000, 105 + proto, amp=8)]))
    rows.append(dict(kind="scene", name="dc_offset", seed=420, n_blocks=16, noise_q8=256, dc_iq=(3, -2),
                     bursts=[_frames_burst(p, 20000 + 95000 * p, 110 + p, amp=40) for p in range(5)]))
    rows.append(dict(kind="scene", name="dc_offset_near_thresh", seed=421, n_blocks=16, noise_q8=256, dc_iq=(5, 2),
                     bursts=[_frames_burst(p, 20000 + 95000 * p, 115 + p, amp=12) for p in range(5)]))
    return rows


# ------------------------------------------------------------------------------------------------ hand-built frames
#
# The decoders' carried state (decode.h, whb_commit.h, chains.hip): what one trigger window or one submit leaves to the next.
# `frames` makes verdicts and bytes depend on it with hand-built frames on a clean signal, `splices` cuts a burst open inside
# its sync word.  Every row is 8 blocks; tests/test_carried_cpu.py measures each class back from the oracle.

CARRIED_BLOCKS = 8
CARRIED_CUTS = [2, 2, 4]           # submits (blocks) of the GPU tests: boundaries at input samples 65536 and 131072
CUT_A, CUT_B = 65536, 131072
BAUD = (38400, 17240, 9600, 8842, 6000)
PREAMBLE = (200, 8, 24, 16, 200)   # on-air bits ahead of the frame (iqgen.c burst_bits)


def bit_sample(proto: int, start: int, bit: int) -> int:
    """Input sample at which on-air bit `bit` of a burst that starts at `start` begins (iqgen.c bit_end, nominal clock)."""
    return start + bit * 1536000 // BAUD[proto]


def frame_span(proto: int, start: int, nbytes: int) -> tuple:
    """(end of the sync word, end of the frame's last byte) of a burst, in input samples."""
    sync = 4 if proto == 4 else 2
    return bit_sample(proto, start, PREAMBLE[proto] + 8 * sync), bit_sample(proto, start, PREAMBLE[proto] + 8 * nbytes)


def crc8(data: bytes) -> int:
    """Polynomial 0x31, MSB first, from 0 (tfa1.cpp, tfa2.cpp)."""
    c = 0
    for v in data:
        c ^= v
        for _ in range(8):
            c = ((c << 1) ^ 0x31) & 0xff if c & 0x80 else (c << 1) & 0xff
    return c


WHB_INIT = {0x02: 0x97d97a26, 0x03: 0xf59c5a1e, 0x04: 0x98e1d11f}   # whb.cpp:50-62, the types used here


def crc32(data: bytes, init: int) -> int:
    """Polynomial 0x04c11db7, MSB first (whb.cpp)."""
    c = init
    for v in data:
        c ^= v << 24
        for _ in range(8):
            c = ((c << 1) ^ 0x04c11db7) & 0xffffffff if c & 0x80000000 else (c << 1) & 0xffffffff
    return c


def _hexs(b) -> str:
    return bytes(b).hex()


def complemented(frame: str) -> str:
    return _hexs(v ^ 0xff for v in bytes.fromhex(frame))


def tfa23_frame(ident: int, temp: int, hum: int) -> str:
    """2d d4 | 9, id (6 bits), 2 zero bits, (temp + 40) * 10 as three BCD digits | humidity | crc8 (tfa2.cpp:6-52)."""
    t = "%03d" % temp
    body = bytes([0x90 | (ident >> 2), ((ident & 3) << 6) | int(t[0]), (int(t[1]) << 4) | int(t[2]), hum])
    return _hexs(b"\x2d\xd4" + body + bytes([crc8(body)]))


def tx22_frame(ident: int, words, nibble: int = 0xa, num=None) -> str:
    """2d d4 | nibble, id (6 bits), no error, num | num 16-bit words | crc8 over all behind the sync."""
    num = len(words) if num is None else num
    body = bytes([(nibble << 4) | (ident >> 2), ((ident & 3) << 6) | 0x10 | num]) + b"".join(w.to_bytes(2, "big") for w in words)
    return _hexs(b"\x2d\xd4" + body + bytes([crc8(body)]))


def whb_frame(stype: int, body: bytes, plen=None) -> str:
    """4b 2d d4 2b | plen | type | body | crc32 over plen .. body; plen = the crc's index in the frame unless given."""
    n = 6 + len(body) if plen is None else plen
    msg = bytes([n, stype]) + body
    return _hexs(b"\x4b\x2d\xd4\x2b" + msg + crc32(msg, WHB_INIT[stype]).to_bytes(4, "big"))


def _fb(proto, start, frame, **kw):
    return dict(proto=proto, start=start, frame=frame, amp=60, **kw)


def _frames_row(name, seed, bursts, **kw):
    return dict(kind="scene", name=name, seed=seed, n_blocks=CARRIED_BLOCKS, noise_q8=256, bursts=bursts, **kw)


def _filler(n: int) -> str:
    """n bytes without an edge pattern that holds a sync word of any decoder, plain or complemented, at any bit offset."""
    return "33" * n


# TX22 stale pair: B's flush has byte_cnt 10 or 11, its num is 7, so tfa2_decoder::flush_tx22 takes the checksum over
# rdata[2 .. 17] and compares it with rdata[18]: the bytes from 10 or 11 on are what A (19 bytes) left.  A's last byte is chosen
# so that B is accepted (from B's flush on the oracle: what lies between B's last byte and its byte_cnt is the demodulator's).
TX22_A = tx22_frame(0x12, [0x0512, 0x1045, 0x2123, 0x3456, 0x4234, 0x0678, 0x1099])
TX22_B = "2dd4a257112233"
TX22_C = tx22_frame(0x2a, [0x0345, 0x1067, 0x2111])   # 11 bytes: its byte_cnt 14 leaves bytes 11 .. 13 on top of A's
TX22_A18 = dict(accept=0x27, over=0x30)           # A's byte 18 for the pair to be accepted, without and with C in between

# WHB stale pair: B (8 bytes, byte_cnt 14) has plen 20: the CRC-32 runs over rdata[4 .. 19] and is compared with
# rdata[20 .. 23]; bytes 14 .. 23 are A's
WHB_A = whb_frame(0x03, bytes(range(0x41, 0x41 + 20)))  # 30 bytes
WHB_B = "4b2dd42b1402a5c3"
WHB_A20 = "a9282701"                            # A's bytes 20 .. 23 for B to be accepted


def _set_bytes(frame: str, at: int, val: bytes) -> str:
    f = bytearray(bytes.fromhex(frame))
    f[at:at + len(val)] = val
    return _hexs(f)


POLARITY = {1: [tfa23_frame(0x15, 612, 45), tfa23_frame(0x2b, 587, 61), tfa23_frame(0x07, 633, 38)],
            2: [tfa23_frame(0x31, 655, 52), tfa23_frame(0x0e, 571, 77), tfa23_frame(0x22, 604, 49)],
            3: [tx22_frame(0x05, [0x0622, 0x1034]), tx22_frame(0x19, [0x0587, 0x1099, 0x2123]), tx22_frame(0x33, [0x0601, 0x1042])]}


def _straddle(proto: int, nbytes: int, cut: int) -> int:
    """A burst start (a multiple of 4) that puts `cut` half way between the end of the sync word and the frame's last byte."""
    a, b = frame_span(proto, 0, nbytes)
    return (cut - (a + b) // 2) // 4 * 4


def _frames():
    rows = []
    for p in (1, 2, 3):
        name = synth.PROTO_NAMES[p].lower()
        f, g, h = POLARITY[p]
        gi = complemented(g)
        n = len(g) // 2
        # the complemented frame lies across the first submit cut: st.invert crosses it in ChainState
        s1 = _straddle(p, n, CUT_A)
        rows.append(_frames_row("pol_%s_inverted" % name, 600 + p, [_fb(p, s1, gi)]))
        for tag, gap in (("one_window", 600), ("split", 4 * (WINDOW[p] + 40))):
            s0 = s1 - gap - synth.burst_length(p, len(f) // 2)
            s2 = s1 + synth.burst_length(p, n) + gap
            rows.append(_frames_row("pol_%s_%s" % (name, tag), 610 + p, [_fb(p, s0, f), _fb(p, s1, gi), _fb(p, s2, h)]))
        rows.append(_frames_row("pol_%s_iq_swap" % name, 620 + p,
                                [_frames_burst(p, 30000, 31 + p, amp=60), _frames_burst(p, _straddle(p, 7, CUT_B), 41 + p, amp=60)],
                                iq_swap=1))
    # ---- TX22 lengths and num
    # (what follows a frame's last byte is the demodulator's: the noise seeds of the length rows are the ones at which the
    # oracle counts exactly these bytes -- tests/test_carried_cpu.py measures them)
    rows.append(_frames_row("tx22_n6_n7_num0_nibble", 632, [
        _fb(3, 8000, "2dd4"), _fb(3, 40000, "2dd4a1"), _fb(3, 80000, tx22_frame(0x11, [])),
        _fb(3, 120000, tx22_frame(0x11, [0x0622, 0x1034], nibble=0xb))]))
    long_tx22 = tx22_frame(0x05, [0x0622, 0x1034])
    rows.append(_frames_row("tx22_n63", 631, [_fb(3, 8000, long_tx22 + _filler(50))]))
    rows.append(_frames_row("tx22_n64", 633, [_fb(3, 8000, long_tx22 + _filler(51))]))
    rows.append(_frames_row("tx22_num7", 636, [_fb(3, 8000, TX22_A)]))
    a = {k: _set_bytes(TX22_A, 18, bytes([v])) for k, v in TX22_A18.items()}
    a["reject"] = _set_bytes(TX22_A, 18, bytes([TX22_A18["accept"] ^ 0x10]))
    rows.append(_frames_row("tx22_stale_accept", 634, [_fb(3, 4000, a["accept"]), _fb(3, 70000, TX22_B)]))
    rows.append(_frames_row("tx22_stale_reject", 634, [_fb(3, 4000, a["reject"]), _fb(3, 70000, TX22_B)]))
    rows.append(_frames_row("tx22_stale_over", 635, [_fb(3, 4000, a["over"]), _fb(3, 40000, TX22_C), _fb(3, 70000, TX22_B)]))
    # ---- WHB lengths and plen
    rows.append(_frames_row("whb_n10_n11", 640, [_fb(4, 8000, "4b2dd42b"), _fb(4, 100000, "4b2dd42b0a")]))
    body = bytes(range(0x61, 0x61 + 44))
    rows.append(_frames_row("whb_n60", 641, [_fb(4, 8000, whb_frame(0x02, body))]))              # 54 bytes
    rows.append(_frames_row("whb_n61", 642, [_fb(4, 8000, whb_frame(0x02, body + b"\x7e"))]))   # 55 bytes
    rows.append(_frames_row("whb_plen_0_3_4", 643, [_fb(4, 4000 + 85000 * k, "4b2dd42b%02x02" % pl) for k, pl in enumerate((0, 3, 4))]))
    rows.append(_frames_row("whb_plen_60_61_type", 644, [_fb(4, 4000, "4b2dd42b3c02"), _fb(4, 89000, "4b2dd42b3d02"),
                                                         _fb(4, 174000, "4b2dd42b0a05112233")]))
    acc = bytes.fromhex(WHB_A20)
    rej = bytes([acc[0], acc[1], acc[2] ^ 0x04, acc[3]])
    rows.append(_frames_row("whb_stale_accept", 645, [_fb(4, 4000, _set_bytes(WHB_A, 20, acc)), _fb(4, 136000, WHB_B)]))
    rows.append(_frames_row("whb_stale_reject", 645, [_fb(4, 4000, _set_bytes(WHB_A, 20, rej)), _fb(4, 136000, WHB_B)]))
    # ---- TFA_1 lengths: a telegram with two bytes behind its checksum, then frames of 4, 3 and 5 bytes
    t = "2dd465b086202360e05697"
    rows.append(_frames_row("tfa1_n10_n9_n11", 652, [_fb(0, 10000, t + "c35a"), _fb(0, 40000, t[:8]), _fb(0, 70000, t[:6]),
                                                    _fb(0, 100000, t[:10])]))
    # ---- long counts: a sync word and then abutting bursts without one, all in one trigger window
    for p, first, nb in ((1, "2dd4", 5), (0, "2dd4", 4)):
        n = synth.burst_length(p, 64)
        rows.append(_frames_row("long_%s" % synth.PROTO_NAMES[p].lower(), 660 + p,
                                [_fb(p, 4000 + k * n, (first + _filler(62)) if k == 0 else _filler(64)) for k in range(nb)]))
    return rows


# ---- splices: a burst cut open, the parts in separate trigger windows.  Noise 0: a window in the silence hands the decoders no
# bit, so the bits of the two parts meet in the shift register as if nothing lay between them.
#
# TFA_1: README.md:123's telegram, cut SPLIT_AT's bits into its sync word (found on the oracle: of the 140 positions
# between bit 1 and bit 16, a multiple of 4 samples apart, these 50 decode -- at the others the demodulator loses or adds a
# bit at the cut).  460 decimated samples of silence: more than the 400 of TFA_1's window, so the first part is flushed as an
# empty window, and the telegram of the second exists only through the shift register the flush did not clear.
#
# WHB: whb_decoder carries its descrambler (lfsr) and the NRZ-S / PSK parities across windows, and a window that ends unsynced
# does not even flush.  But no cut of a WHB burst was found after which the demodulator's bits continue where they stopped: at
# each of the 4 .. 47 bit positions ahead of and behind the sync word, every 4 samples, at three seeds, amplitudes 30 .. 100 and
# offsets 0 .. -5 kHz, whb_demod hands over two more bits at the cut (the level's decay is a peak to it) -- so the
# self-synchronising descrambler needs its 17 bits again, and a sync word fewer than 17 bits behind the second window's first
# bit is never found, whatever lfsr was handed over.  The nearest cuts that still decode lie 18 bits ahead of the sync word;
# the WHB rows use those, and tests/test_carried_cpu.py shows both: the rows decode, and the handed-over lfsr decides nothing.
TFA1_TELEGRAM = "2dd465b086202360e05697"
SPLICE_START = 30000
SPLIT_AT = {3: 38140, 5: 38220, 7: 38300, 10: 38420, 12: 38500}   # bits into the sync word -> cut, for a burst at SPLICE_START
SPLICE_GAP = 4 * 460
WHB_SPLICE_AT = 30000 + 200 * 256 - 18 * 256 + 64                  # 17.75 bits ahead of the sync word
WHB_SPLICE_GAP = 4 * 560


def _splice(name, proto, shift, at, gap, dots=(), **burst):
    """A burst of `proto` at SPLICE_START + shift, cut at at + shift."""
    base = dict(kind="scene", name=name + "_base", seed=500 + (proto == 4), n_blocks=CARRIED_BLOCKS, noise_q8=0,
                bursts=[dict(proto=proto, start=SPLICE_START + shift, amp=60, **burst)])
    ats = [at] if isinstance(at, int) else at   # (several cuts: each position in the burst, each `gap` wide)
    return dict(kind="splice", name=name, n_blocks=CARRIED_BLOCKS, base=base, cuts=[[a + shift, gap] for a in ats],
                dots=[d + shift for d in dots])


def splice_parts(row) -> tuple:
    """(last input sample of the first part + 1, first input sample of the second part) of a splice row, in the row."""
    at, gap = row["cuts"][0]
    return at, at + gap


def _splices():
    rows = []
    g = SPLICE_GAP
    t1 = dict(frame=TFA1_TELEGRAM)
    for bit, at in sorted(SPLIT_AT.items()):   # both windows in one submit
        rows.append(_splice("tfa1_split_bit%d" % bit, 0, 0, at, g, **t1))
    for bit in (5, 10):
        at = SPLIT_AT[bit]
        # the first window closes 400 decimated samples behind the cut, the second part begins 460 behind it: the submit cut
        # at 430 puts the second part into window 0 of the next submit
        rows.append(_splice("tfa1_split_bit%d_submit_cut" % bit, 0, CUT_A - 4 * 430 - at, at, g, **t1))
        # the submit cut 200 samples behind the cut: the first window is still open there, closes as window 0 of the next
        # submit without a bit, and the second part is its window 1 (have = 0)
        rows.append(_splice("tfa1_split_bit%d_open_at_cut" % bit, 0, CUT_A - 4 * 200 - at, at, g, **t1))
    at = SPLIT_AT[7]
    # one and two dot windows between the parts, in one submit ...
    rows.append(_splice("tfa1_split_one_empty", 0, 0, at, 2 * g, dots=[at + g], **t1))
    rows.append(_splice("tfa1_split_two_empty", 0, 0, at, 3 * g, dots=[at + g, at + 2 * g], **t1))
    # ... and with the first part in the submit before: the submit cut between the first flush and the dot
    rows.append(_splice("tfa1_split_empty_behind_cut", 0, CUT_A - 4 * 430 - at, at, 2 * g, dots=[at + g], **t1))
    # cut twice inside the sync word: the middle window holds 7 of its bits, the last window's register is pieced together
    # from two windows (one submit), and from one window and ChainState.sr (0 < have < 32: the middle window is window 0 of the
    # submit behind the cut)
    a1, a2 = SPLIT_AT[3], SPLIT_AT[10]
    rows.append(_splice("tfa1_split_three_ways", 0, 0, [a1, a2], g, **t1))
    rows.append(_splice("tfa1_split_three_ways_submit_cut", 0, CUT_A - 4 * 430 - a1, [a1, a2], g, **t1))
    # WHB, cut in its preamble
    w = dict(payload_seed=5)
    rows.append(_splice("whb_cut_preamble", 4, 0, WHB_SPLICE_AT, WHB_SPLICE_GAP, **w))
    # (the submit cut 540 samples behind the cut: the first window, 512 long, has closed there)
    rows.append(_splice("whb_cut_preamble_submit_cut", 4, CUT_B - 4 * 540 - WHB_SPLICE_AT, WHB_SPLICE_AT, WHB_SPLICE_GAP, **w))
    return rows


FAMILIES = dict(dense=_dense, edges=_edges, repeats=_repeats, collisions=_collisions, drift=_drift, levels=_levels,
                frames=_frames, splices=_splices)


def carried_boundaries() -> list:
    """The submit boundaries of CARRIED_CUTS in input samples."""
    return [int(v) * 32768 for v in np.cumsum(CARRIED_CUTS)]


def carried_cut_claims(fam) -> list:
    """Where the submits of CARRIED_CUTS must cut a family's rows for state to be carried in ChainState: [(row name, the submit
    boundary in input samples, lo, hi)], the boundary to lie in (lo, hi) -- inside every complemented frame between its sync word
    and its last byte, between A and B of a stale pair, between the parts of a splice that is meant to lie across a cut."""
    out = []
    for row in FAMILIES[fam]():
        name = row["name"]
        if name.startswith("pol_"):
            p = row["bursts"][0]["proto"]
            for b in row["bursts"]:
                inverted = row.get("iq_swap") or ("frame" in b and b["frame"].startswith("d22b"))
                a, e = frame_span(p, b["start"], len(b["frame"]) // 2 if "frame" in b else 7)
                for cut in (CUT_A, CUT_B):
                    if inverted and a < cut < e:
                        out.append((name, cut, a, e))
        elif "_stale_" in name:
            a, b = row["bursts"][-2], row["bursts"][-1]
            cut = CUT_B if a["proto"] == 4 else CUT_A
            out.append((name, cut, frame_span(a["proto"], a["start"], len(a["frame"]) // 2)[1], b["start"]))
        elif row["kind"] == "splice" and ("submit_cut" in name or "at_cut" in name or "behind_cut" in name):
            lo, hi = splice_parts(row)
            out.append((name, CUT_B if name.startswith("whb") else CUT_A, lo, hi))
    return out



def family(name: str) -> list:
    return FAMILIES[name]()


# ------------------------------------------------------------------------------------------------ windows (CPU model)

def trigger_samples(dec: np.ndarray, thresh: int = THRESH) -> np.ndarray:
    d = dec.reshape(-1, 2).astype(np.int64)
    return np.nonzero(np.abs(d).sum(1) > thresh)[0]


def windows(trig: np.ndarray, w: int) -> list:
    """[(open, close)] of one chain: a window opens at a trigger while none is open and closes W-1 samples after its last
    trigger (tfa1.cpp:147-149,179 / tfa2.cpp:351-355,428 / whb.cpp:636-641,691)."""
    out = []
    if len(trig) == 0:
        return out
    brk = np.nonzero(np.diff(trig) > w - 1)[0]
    firsts = np.concatenate([[trig[0]], trig[brk + 1]])
    lasts = np.concatenate([trig[brk], [trig[-1]]])
    return [(int(a), int(b) + w - 1) for a, b in zip(firsts, lasts)]


def table_demand(wins: list, m: int, n_submits: int, bits_per_window=None) -> dict:
    """What the windows of one chain need of the device tables in the worst submit of n_submits submits of M samples each:
    windows (T.cap), window-relative 32-sample slots (win_slot0 = (og >> 5) + j, T.slots), bit words (window j's bits from
    word (og >> 6) + 3 j, T.bit_words) and WHB step records (one per 64-sample step a window touches + one per window that
    begins locked + the end mark, T.whbrec_stride without its slack)."""
    worst = dict(windows=0, slots=0, bit_words=0, whbrec=0)
    for s in range(n_submits):
        lo, hi = s * m, (s + 1) * m
        j = 0
        need = dict(windows=0, slots=0, bit_words=0, whbrec=1)
        for k, (a, b) in enumerate(wins):
            if b < lo or a >= hi:
                continue
            og = max(a, lo) - lo  # a window carried in from the submit before is re-opened at its first sample
            last = min(b, hi - 1) - lo
            n = last - og + 1
            need["windows"] = j + 1
            need["slots"] = max(need["slots"], (og >> 5) + j + (n + 31) // 32)
            nb = bits_per_window[k] if bits_per_window is not None else n
            need["bit_words"] = max(need["bit_words"], (og >> 6) + 3 * j + (nb + 31) // 32 + 1)
            need["whbrec"] += (og % 64 + n + 63) // 64 + 1
            j += 1
        for key in worst:
            worst[key] = max(worst[key], need[key])
    return worst
