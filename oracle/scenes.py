"""Scene families: hand-placed inputs for the window geometry and the state that crosses windows -- TEST INFRASTRUCTURE.

Two kinds of rows, both integer-only (the bytes are the same on every machine):
  scene  -- tfrec_amd.synth.gen_scene over an explicit burst list (repeats, collisions, clock offsets, levels);
  comb   -- copies of one short pulse pasted so that the trigger test |I| + |Q| > thresh (fm_demod.cpp:45,
            frontend.hip:8) fires on chosen decimated samples (dense windows, block and submit edges).

A family is a list of rows run as one batch.  oracle/mint_golden.py pins a subset against the real reference
(tests/golden/scenes.json); tests/test_scenes_cpu.py and tests/test_gpu_scenes.py replay them.
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


def render(spec) -> np.ndarray:
    if spec["kind"] == "comb":
        return render_comb(spec)
    return synth.gen_scene(spec["seed"], spec["n_blocks"], spec["bursts"], spec.get("noise_q8", 256),
                           tuple(spec.get("dc_iq", (0, 0))))


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


FAMILIES = dict(dense=_dense, edges=_edges, repeats=_repeats, collisions=_collisions, drift=_drift, levels=_levels)


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
