"""The inputs of the front end's tests that need no GPU -- the scenes at other sample rates and in other formats, the recordings with
bursts beyond +-768 kHz, the wide 15.36 MS/s scene, the rows several receivers share, the rows of the two rate sweeps -- and their
restated expectations, from the oracle and the numpy restatements.  Everything is computed once per session where it is cached
and read-only where it is shared.  Imported as a plain module (`import input_rows`) from the CPU and the GPU test modules; the
tests that hold these inputs to what they are there for are in the CPU modules of each feature."""
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import parity
from oracle import oracle as O
from tfrec_amd import api, formats, resample, synth, tune

TYPES, THRESH = 0x2F, 500

# ---- the scenes at other sample rates: the generator's streams at rate_mult = P with every Q-th complex sample kept
# are recordings at 1536000 P / Q samples per second -- 2.048 MS/s and 2.4 MS/s
SCENE_RATES = [(4, 3), (25, 16)]
SCENE_BLOCKS = 12
SCENE_STREAMS = [(1, 0), (3, 1)]  # (seed, stream): chosen on the CPU so that every protocol decodes (test_resample_cpu.py asserts it)


def rate_stream(p, q, seed, stream, n_blocks=SCENE_BLOCKS, noise_q8=256):
    """u8 IQ of n_blocks blocks' worth of input at 1536000 p / q samples per second."""
    x = synth.gen_stream(seed, stream, n_blocks, 0x1F, noise_q8, rate_mult=p).reshape(-1, 2)[::q]
    x = np.ascontiguousarray(x).reshape(-1)
    assert len(x) == 2 * resample.input_samples(n_blocks, p, q), "%d/%d: %d bytes" % (p, q, len(x))
    return x


def rate_scene(p, q, n_blocks=SCENE_BLOCKS):
    """[streams, bytes]: the scene of one rate."""
    return np.stack([rate_stream(p, q, seed, s, n_blocks) for seed, s in SCENE_STREAMS])


def oracle_of(x, p, q, types=TYPES, thresh=THRESH, wide=0, log_bits=False):
    """The oracle fed the restatement's stage 0 of one stream's input."""
    o = O.Oracle(types, thresh, wide, log_bits=log_bits)
    o.process_s16(resample.resample_s16(x, p, q))
    return o


# ---- the scenes in other sample formats.  `kind` names a format and how the scene fills it:
#   s8    the u8 scene's bytes ^ 0x80: the same x
#   s16   ((u8 - 128) << 8) + e, e in [-128, 127]: full-scale int16 whose content below u8's resolution reaches x
#   s16d  (x << 2) + d, d in [-2, 1]: the bits >> 2 drops -- a negative d moves x down by one, the shift floors
#   f32   the s16 scene's values / 32768: v = s16 / 4 lands on quarters, so rint rounds where >> 2 floors, ties included
KINDS = {"s8": "s8", "s16": "s16", "s16d": "s16", "f32": "f32"}


@functools.lru_cache(maxsize=None)
def scene_u8(p, q):
    """[streams, bytes]: rate_scene of the rate, or -- 1/1 -- the generator's streams of the same seeds."""
    if (p, q) != (1, 1):
        return rate_scene(p, q)
    return np.stack([synth.gen_stream(seed, s, SCENE_BLOCKS, 0x1F, 256, rate_mult=1) for seed, s in SCENE_STREAMS])


@functools.lru_cache(maxsize=None)
def scene(kind, p, q):
    """[streams, bytes] (uint8, read-only): the scene of one rate as rows of the kind's format."""
    u = scene_u8(p, q)
    rng = np.random.default_rng(100 * p + q)
    if kind == "s8":
        rows = u ^ 0x80
    elif kind == "s16d":
        x = (u.astype(np.int32) - 128) << 6
        rows = np.clip((x << 2) + rng.integers(-2, 2, u.shape), -32768, 32767).astype("<i2").view(np.uint8)
    else:
        v = np.clip(((u.astype(np.int32) - 128) << 8) + rng.integers(-128, 128, u.shape), -32768, 32767)
        rows = v.astype("<i2").view(np.uint8) if kind == "s16" else (v.astype(np.float32) / np.float32(32768.0)).astype("<f4").view(np.uint8)
    rows = np.ascontiguousarray(rows)
    want = (len(u), u.shape[1] * formats.bytes_per_sample(KINDS[kind]) // 2)
    assert rows.shape == want, "%s %d/%d: rows of shape %s, want %s" % (kind, p, q, rows.shape, want)
    rows.setflags(write=False)
    return rows


def format_stage0(fmt, row, p, q):
    """The restatement's stage 0 of one stream's row: x, resampled unless the rate is 1/1."""
    x = formats.to_x(fmt, row)
    return x if (p, q) == (1, 1) else resample.resample_x16(x, p, q)


@functools.lru_cache(maxsize=None)
def scene_stage0(kind, p, q, s):
    y = format_stage0(KINDS[kind], scene(kind, p, q)[s], p, q)
    y.setflags(write=False)
    return y


@functools.lru_cache(maxsize=None)
def scene_oracle(kind, p, q, s, log_bits=False):
    """The oracle fed the restatement's stage 0 of stream s of a scene (computed once per session)."""
    o = O.Oracle(TYPES, THRESH, 0, log_bits=log_bits)
    o.process_s16(scene_stage0(kind, p, q, s))
    return o


# ---- the recordings of the input-rate tune: one per rate with a burst of its own protocol at every frequency of
# WIDE_SCENES -- at the centre, inside +-768 kHz and beyond it.  Chosen on the CPU so that the oracle decodes each burst for exactly
# the receiver tuned to it, and so that a burst beyond +-768 kHz stays out of reach of the tune behind the resampler
# (test_input_tune_cpu.py asserts it).
WIDE_SCENES = {(25, 16): (0, 300000, 1100000, -1050000),  # 2.4 MS/s: +-1.2 MHz
               (25, 12): (0, -400000, 1300000)}           # 3.2 MS/s: +-1.6 MHz
WIDE_ROW_BLOCKS = 6


def wide_row(p, q, n_blocks=WIDE_ROW_BLOCKS, seed=77):
    """[1, bytes]: u8 IQ at 1536000 p / q with burst j (protocol j) at WIDE_SCENES[p, q][j] Hz from the centre."""
    freqs = WIDE_SCENES[p, q]
    n = n_blocks * api.BLOCK_BYTES // 2 * p
    bursts = [dict(proto=j, start=(40000 * p + j * (n - 100000 * p) // len(freqs)) // q * q, payload_seed=21 + j, f0_hz=f, amp=50)
              for j, f in enumerate(freqs)]
    x = synth.gen_scene(seed, n_blocks, bursts, rate_mult=p).reshape(-1, 2)[::q]
    x = np.ascontiguousarray(x).reshape(1, -1)
    assert x.shape[1] == 2 * resample.input_samples(n_blocks, p, q), "%d/%d: %d bytes" % (p, q, x.shape[1])
    return x


def tuned_stage0(x, p, q, input_hz):
    """The restatement's stage 0 of one stream's input with an input-rate tune."""
    return resample.resample_x16(tune.mix_in_s16(tune.s16_of_u8(x), input_hz, p, q), p, q)


def stage0_of_x(x, p, q, input_hz=0):
    """... and of samples that are x already (behind an input correction): the mixer only where tuned, no stage at 1/1."""
    x = tune.mix_in_s16(x, input_hz, p, q) if input_hz else x
    return x if (p, q) == (1, 1) else resample.resample_x16(x, p, q)


def input_oracle(x, p, q, input_hz, narrow_hz=0, log_bits=False):
    """The oracle fed the restatement: the input-rate mixer, the resampling stage, then the tune behind it."""
    o = O.Oracle(TYPES, THRESH, 0, log_bits=log_bits)
    o.process_s16(tune.mix_s16(tuned_stage0(x, p, q, input_hz), narrow_hz, 0))
    return o


# ---- the wide scene of the shared inputs and the wideband tune: one burst per protocol of the TFA_2 family and
# TFA_1, each at its own offset in the 15.36 MS/s band, each in its own time slot; nothing at EMPTY_HZ
WIDE_SCENE_BLOCKS = 4
WIDE_BURSTS = ((-5200000, 0), (-1100000, 1), (3300000, 2), (6900000, 3))  # (offset in Hz, protocol = slot)
EMPTY_HZ = 2000000


def wide_scene(seed=41, n_blocks=WIDE_SCENE_BLOCKS, amp=40):
    n = n_blocks * api.BLOCK_BYTES // 2 * 10  # input samples
    bursts = [dict(proto=p, start=(200000 + j * (n - 400000) // 4) // 10 * 10, payload_seed=5 + j, f0_hz=f, amp=amp)
              for j, (f, p) in enumerate(WIDE_BURSTS)]
    return synth.gen_scene(seed, n_blocks, bursts, rate_mult=10)


# ---- the rows several receivers share
DFLT = (0x2F, 500, 0)
ROWS = 6
# the four receivers of row j are tuned to ROW_TUNES[j]; each row carries a burst at every one of them (and one at the centre)
ROW_TUNES = [(0, 200000, -250000, 25000), (150000, 0, -400000, 767999), (-767999, 12345, 0, 500000),
             (-200000, 99999, 700001, 0), (0, -25000, 31, -654321), (300000, -1, -500000, 0)]
CFGS = {1: (0x2F, 500, 1), 2: (0x03, 0, 0), 4: (0x21, 300, 0), 5: (0x2F, 0, 1), 7: (0x01, 500, 0), 8: (0x2F, 900, 0),
        10: (0x02, 0, 1), 13: (0x2F, 300, 0), 14: (0x06, 0, 0), 17: (0x0C, 500, 0), 20: (0x28, 500, 1), 23: (0x01, 0, 1)}


def make_rows(seed, n_blocks, rows=ROWS):
    out = []
    n = n_blocks * api.BLOCK_BYTES // 2
    for j in range(rows):
        offs = sorted(set(ROW_TUNES[j % len(ROW_TUNES)]) | {0})
        bursts = [dict(proto=(j + i) % 5, start=20000 + i * (n - 60000) // len(offs), payload_seed=7 + j + 11 * i, f0_hz=f,
                       amp=50 + 5 * i) for i, f in enumerate(offs)]
        out.append(synth.gen_scene(seed * 100 + j, n_blocks, bursts))
    return np.stack(out)


# ---- the rows and the expectations of a rate sweep, computed once per session
@functools.lru_cache(maxsize=None)
def sweep_rows(fmt, p, q, n_streams, n_blocks):
    """[streams, bytes] (uint8, read-only): different full-scale random data per stream, so that a row mix-up shows; the f32
    rows reach beyond +-1, so that the clamp acts."""
    n = resample.input_samples(n_blocks, p, q)
    if fmt == "u8":
        rows = np.random.default_rng(1000 * p + q).integers(0, 256, (n_streams, 2 * n), dtype=np.uint8)
    else:
        rows = np.concatenate([parity.full_scale_row(fmt, n, 1000 * p + q + 7 * s + 1) for s in range(n_streams)])
    want = (n_streams, n * formats.bytes_per_sample(fmt))
    assert rows.shape == want, "%d/%d %s: rows of shape %s, want %s" % (p, q, fmt, rows.shape, want)
    assert not np.array_equal(rows[0], rows[1]), "%d/%d %s: rows 0 and 1 are the same" % (p, q, fmt)
    rows.setflags(write=False)
    return rows


@functools.lru_cache(maxsize=None)
def sweep_stage0(fmt, p, q, hz, n_blocks):
    """The restatement's stage 0 of every stream of sweep_rows over the whole run (read-only), stream s tuned to hz[s] at the
    input rate: u8 through resample_s16 or -- any stream tuned -- tuned_stage0, a format through formats.to_x, tune.mix_in_s16
    and resample_x16."""
    rows = sweep_rows(fmt, p, q, len(hz), n_blocks)

    def one(s):
        if fmt == "u8":
            y = tuned_stage0(rows[s], p, q, hz[s]) if any(hz) else resample.resample_s16(rows[s], p, q)
        else:
            x = formats.to_x(fmt, rows[s])
            y = resample.resample_x16(tune.mix_in_s16(x, hz[s], p, q) if hz[s] else x, p, q)
        assert len(y) == 2 * n_blocks * 32768, "%d/%d %s stream %d: %d values, want %d" % (p, q, fmt, s, len(y), 2 * n_blocks * 32768)
        y.setflags(write=False)
        return y

    with ThreadPoolExecutor(len(rows)) as ex:  # (numpy releases the GIL in the gathers and sums)
        return tuple(ex.map(one, range(len(rows))))


# ---- the sweep across the rates of Q <= 64 (test_rate_sweep_cpu.py, test_rate_sweep_gpu.py): (P, Q, T, block unit, tile of the
# tuned and the format launches, format of case (d)).  Each is there for something the kernels care about;
# test_rate_sweep_cpu.py's test_sweep_rates_are_what_they_are_there_for asserts it.
#   65/64         the smallest r: T = 8, the largest sum |h| (108112), 64 phases, phi wraps on almost every output
#   3/2, 127/64   T = 10 and 12; r just under 2
#   2/1, 4/1, 9/1 Q = 1: one phase, P mod Q = 0; T = 12, 24, 54
#   19/2          T = 58 with Q = 2
#   39/4          T = 60 with a small Q: the tile's first read reaches 59 samples into the history; a half-tile rate (49344)
#   461/64        the last whole-tile rate: the tuned launch's LDS is exactly the 49152-byte limit
#   267/32, 463/64  the first half-tile rates: 49248 and 49280
#   639/64        the largest rate: the plain kernel's LDS maximum (35936), T = 60
#   5/3, 25/12    block unit 3
#   7/5           block unit 5
# The format of case (d) cycles s8, s16, f32 down the table, so that each format meets whole-tile and half-tile rates.
RATE_SWEEP = [
    (65, 64, 8, 1, 1024, "s8"),
    (3, 2, 10, 1, 1024, "s16"),
    (127, 64, 12, 1, 1024, "f32"),
    (2, 1, 12, 1, 1024, "s8"),
    (4, 1, 24, 1, 1024, "s16"),
    (9, 1, 54, 1, 1024, "f32"),
    (19, 2, 58, 1, 1024, "s8"),
    (39, 4, 60, 1, 512, "s16"),
    (461, 64, 44, 1, 1024, "f32"),
    (267, 32, 52, 1, 512, "s8"),
    (463, 64, 44, 1, 512, "s16"),
    (639, 64, 60, 1, 512, "f32"),
    (5, 3, 10, 3, 1024, "s8"),
    (25, 12, 14, 3, 1024, "s16"),
    (7, 5, 10, 5, 1024, "f32"),
]
RATE_SWEEP_IDS = ["%d/%d" % r[:2] for r in RATE_SWEEP]
RATE_SWEEP_FORMAT = {r[:2]: r[5] for r in RATE_SWEEP}
RATE_SWEEP_STREAMS = 3
LDS_LIMIT = 49152


# the launch geometry as csrc/resample.h documents it, restated: this records why a rate is in the sweep
def raw_chunks(p, q, t, tile):
    """16-byte chunks of raw u8 a tile stages: its samples (the last one floor((Q - 1 + (tile - 1) P) / Q) behind the first
    output's i0, T - 1 before it) and up to 14 bytes of alignment."""
    return (2 * ((q - 1 + (tile - 1) * p) // q + t) + 29) // 16


def tuned_lds(p, q, t, tile):
    """Bytes of LDS of a tuned launch: the table padded to 4 dwords, the int16 image (8 dwords per chunk), the cosine table."""
    return (((q * t + 3) & ~3) + 8 * raw_chunks(p, q, t, tile)) * 4 + 8192


def tile_of(p, q, t):
    return 1024 if tuned_lds(p, q, t, 1024) <= LDS_LIMIT else 512


def rate_sweep_sizes(q):
    """The submits of a sweep run, in blocks: both history buffers are used and the first one reused, the phase carries twice,
    and the first and last submits are smaller than the context's buffers (max_blocks = 2 units)."""
    unit = resample.permitted_blocks(q)
    return (unit, 2 * unit, unit)


def rate_sweep_tunes(p, q):
    """Per stream: 1234 Hz inside the limit of the input-rate tune, untuned, and a negative tune."""
    return ((1536000 * p + 2 * q - 1) // (2 * q) - 1 - 1234, 0, -123457)


def rate_sweep_rows(fmt, p, q):
    return sweep_rows(fmt, p, q, RATE_SWEEP_STREAMS, sum(rate_sweep_sizes(q)))


def rate_sweep_stage0(fmt, p, q, tuned):
    return sweep_stage0(fmt, p, q, rate_sweep_tunes(p, q) if tuned else (0,) * RATE_SWEEP_STREAMS, sum(rate_sweep_sizes(q)))


# ---- the sweep across the whole-kHz rates, Q | 1536 (test_khz_rates_cpu.py, test_khz_rates_gpu.py): (P, Q, streams, submits in
# blocks, untuned formats, format of the tuned case)
#   125/96      T 8, unit 3, a small table (768 taps): the staged kernels
#   625/384     Q T = 3840, the largest table the staged kernels take; unit 6
#   129/128     unit 2, where the odd part would say 1
#   3125/384    T 50, 19200 taps (75 KB): the first case whose table cannot sit in LDS; a half-tile rate
#   735/512     Q 512, T 10: 5120 taps
#   1537/1536   T 8: every output of a tile another phase
#   15359/1536  T 60: the largest table (92160 taps) and the largest P; two streams and two formats keep the restatement within seconds
KHZ_SWEEP = [
    (125, 96, 3, (3, 6, 3), ("u8", "s8", "s16", "f32"), "s8"),
    (625, 384, 3, (6, 12, 6), ("u8", "s8", "s16", "f32"), "s16"),
    (129, 128, 3, (2, 4, 2), ("u8", "s8", "s16", "f32"), "f32"),
    (3125, 384, 3, (6, 12, 6), ("u8", "s8", "s16", "f32"), "s8"),
    (735, 512, 3, (8, 16, 8), ("u8", "s8", "s16", "f32"), "s16"),
    (1537, 1536, 3, (24, 24), ("u8", "s8", "s16", "f32"), "f32"),
    (15359, 1536, 2, (24, 24), ("u8", "s16"), "s16"),
]
KHZ_SWEEP_IDS = ["%d/%d" % r[:2] for r in KHZ_SWEEP]
KHZ_SWEEP_BY_RATE = {r[:2]: r for r in KHZ_SWEEP}


def khz_sweep_tunes(p, q, fmt):
    """Per stream; at the two rates whose tunes overflow a 64-bit numerator, those tunes."""
    if (p, q) == (15359, 1536):
        return (7000001, 0) if fmt == "u8" else (0, -699051)
    return (6249999 if (p, q) == (3125, 384) else 1234, 0, -123457)


def khz_sweep_rows(fmt, p, q):
    _, _, n_streams, sizes, _, _ = KHZ_SWEEP_BY_RATE[p, q]
    return sweep_rows(fmt, p, q, n_streams, sum(sizes))


def khz_sweep_stage0(fmt, p, q, tuned):
    _, _, n_streams, sizes, _, _ = KHZ_SWEEP_BY_RATE[p, q]
    return sweep_stage0(fmt, p, q, khz_sweep_tunes(p, q, fmt) if tuned else (0,) * n_streams, sum(sizes))


# the scenes of the whole-kHz end-to-end tests: 2.0 and 12.5 MS/s
KHZ_SCENE_RATES = [(125, 96), (3125, 384)]


@functools.lru_cache(maxsize=None)
def khz_scene(p, q, n_blocks=SCENE_BLOCKS):
    """rate_scene (read-only), its streams generated beside each other: at P = 3125 the generator makes 2.4 GB per stream before
    the decimation by Q."""
    with ThreadPoolExecutor(len(SCENE_STREAMS)) as ex:
        iq = np.stack(list(ex.map(lambda a: rate_stream(p, q, a[0], a[1], n_blocks), SCENE_STREAMS)))
    iq.setflags(write=False)
    return iq
