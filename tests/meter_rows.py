"""The inputs of the side outputs' and the input corrections' tests that need no GPU -- the level meter's crafted samples, the scan
file, the spectrum's rows, the scenes with a DC offset, the balancer's guard rows and ghost scene -- and their restated expectations.
Imported as a plain module (`import meter_rows`) from the CPU and the GPU test modules; the tests that hold these inputs to what
they are there for are in the CPU modules of each feature."""
import functools
import itertools
import os

import numpy as np

import parity
from input_rows import THRESH, TYPES
from oracle import oracle as O
from tfrec_amd import api, formats, iqbal, levels, resample, spectrum, synth, tune

B = levels.BLOCK_DEC
BB = api.BLOCK_BYTES
GOLDEN = os.path.join(parity.ROOT, "tests", "golden")

# ---- the level meter
TYPE_BITS = (0x01, 0x02, 0x04, 0x08, 0x20)
SUBSETS = [sum(c) for k in range(1, 6) for c in itertools.combinations(TYPE_BITS, k)]


def crafted_dec(W, seed, n_blocks=3):
    """Quiet noise with single loud samples (pwr 6000 > any threshold here): one at the last sample of block 0; pairs whose
    distances are W - 1, W, W + 1 and W + 2 -- gaps of W - 2 .. W + 1 quiet samples between two triggers, the ones around the
    point where the first trigger's window ends --; one W / 2 ahead of the boundary between blocks 1 and 2, whose window
    straddles it, and the one at the end of block 0, whose window lies wholly in block 1; a few at random."""
    rng = np.random.default_rng(seed)
    dec = rng.integers(-40, 41, size=(n_blocks * B, 2)).astype(np.int16)
    loud = [B - 1, 2 * B - W // 2]
    pos = 200
    for d in (W - 1, W, W + 1, W + 2):
        loud += [pos, pos + d]
        pos += d + W + 100  # the next pair starts in the open again
    assert pos < B - W, "W %d: the pairs end at %d, beyond block 0's last window" % (W, pos)
    loud += [int(v) for v in rng.integers(2 * B + W, n_blocks * B - 1, 3)]
    loud.append(n_blocks * B - 1)  # ... and one whose window is cut by the end of the input
    for p in loud:
        dec[p] = (3000, -3000)
    return dec, sorted(loud)


def scan_file():
    """262144 bytes at 2.048 MS/s: the first three blocks of the golden TFA_2 scene, brought from 1.536 MS/s to 4/3 of it (zero
    stuffing by 4, a windowed-sinc low-pass, every third sample) and moved to +600 kHz."""
    z = np.load(os.path.join(GOLDEN, "iq_tfa_2.npz"))
    u = z["iq"][:3 * api.BLOCK_BYTES].astype(np.float64).reshape(-1, 2) - 128.0
    x = np.zeros(4 * len(u), dtype=np.complex128)
    x[::4] = u[:, 0] + 1j * u[:, 1]
    t = np.arange(-64, 65)
    h = np.sinc(t / 4.0 * 0.8) * np.hamming(len(t))
    h *= 4.0 / h.sum()
    y = np.convolve(x, h, mode="same")[::3]
    y = y * np.exp(2j * np.pi * 600000.0 / 2048000.0 * np.arange(len(y)))
    out = np.empty((len(y), 2), dtype=np.uint8)
    out[:, 0] = np.clip(np.rint(y.real) + 128, 0, 255)
    out[:, 1] = np.clip(np.rint(y.imag) + 128, 0, 255)
    assert out.size == 2 * resample.input_samples(3, 4, 3) == 262144, "the scan file has %d bytes" % out.size
    return out.reshape(-1)


# ---- the power spectrum
def assert_spectrum(got, want, label=""):
    for name, g, w in zip(("sum", "peak", "n_frames"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, "%s %s: %s %s, want %s %s" % (label, name, g.dtype, g.shape, w.dtype, w.shape)
        if not np.array_equal(g, w):
            bad = np.argwhere(g != w)
            raise AssertionError("%s %s: %d values differ, first at %s: got %d, want %d" % (
                label, name, len(bad), tuple(bad[0]), g[tuple(bad[0])], w[tuple(bad[0])]))


def tone(n, f_rel, amp):
    ph = 2.0 * np.pi * f_rel * np.arange(n)
    return np.stack([amp * np.cos(ph), amp * np.sin(ph)], axis=1).reshape(-1)


@functools.lru_cache(maxsize=None)
def u8_rows(n_blocks=2):
    """[3, n_blocks] u8: random full-range bytes plus a tone, all bytes 0, samples alternating 0 and 255."""
    n = n_blocks * BB // 2
    rng = np.random.default_rng(11)
    a = np.clip(rng.integers(0, 256, 2 * n) + np.rint(tone(n, 0.1337, 60.0)), 0, 255).astype(np.uint8)
    z = np.zeros(2 * n, dtype=np.uint8)
    y = np.repeat(np.tile(np.array([0, 255], dtype=np.uint8), n // 2), 2)
    rows = np.stack([a, z, y])
    rows.setflags(write=False)
    return rows


@functools.lru_cache(maxsize=None)
def want_u8(n_bins, g, n_blocks=2, first=0):
    return [spectrum.spectrum(row[first * BB:(first + n_blocks) * BB], n_bins, g, fmt="u8") for row in u8_rows(max(2, first + n_blocks))]


@functools.lru_cache(maxsize=None)
def golden():
    """[1, 3 blocks]: the start of the golden TFA_2 scene."""
    z = np.load(os.path.join(GOLDEN, "iq_tfa_2.npz"))
    x = np.ascontiguousarray(z["iq"][:3 * BB]).reshape(1, -1)
    x.setflags(write=False)
    return x


# ---- the DC blocker's acceptance table: the golden scenes with a DC offset, behind the oracle
OFFSET = (8, -4)  # the acceptance test's offset in u8 LSB: +d on I, -d / 2 on Q


@functools.lru_cache(maxsize=None)
def golden_scene(name):
    z = np.load(os.path.join(GOLDEN, "iq_%s.npz" % name))
    iq = z["iq"][:len(z["iq"]) // api.BLOCK_BYTES * api.BLOCK_BYTES]  # whole blocks
    o = O.Oracle(0x2F, 500)
    o.process(iq)
    return iq, o.text()


def offset_scene(name, d=OFFSET):
    """The scene's u8 bytes with +d[0] on I and d[1] on Q, clipped to 0 .. 255."""
    iq, _ = golden_scene(name)
    v = iq.astype(np.int32).reshape(-1, 2) + np.asarray(d)
    return np.clip(v, 0, 255).astype(np.uint8).reshape(-1)


# ---- the IQ balancer
IDENT = (0, 16384)


def impair(x, gain, deg):
    """x (interleaved int16) with Q <- gain (Q cos(deg) + I sin(deg)), rounded and clamped to the rails."""
    v = np.asarray(x, dtype=np.int16).reshape(-1, 2).astype(np.float64)
    ph = np.deg2rad(deg)
    out = np.asarray(x, dtype=np.int16).reshape(-1, 2).copy()
    out[:, 1] = np.clip(np.rint(gain * (v[:, 1] * np.cos(ph) + v[:, 0] * np.sin(ph))), -8192, 8191).astype(np.int16)
    return out.reshape(-1)


def guard_rows(n_win=4):
    """name -> interleaved int16 x of n_win windows that trips exactly that guard; `fine` trips none."""
    rng = np.random.default_rng(4)
    i = rng.integers(-3000, 3000, n_win * iqbal.L)
    q0 = rng.integers(-3000, 3000, n_win * iqbal.L)
    rows = {"silence": (0 * i, 0 * i), "correlated": (i, i), "t": (i, i // 2 + rng.integers(-40, 40, n_win * iqbal.L)), "g": (i, 2 * q0),
            "fine": (i, q0 + i // 8)}
    return {k: np.stack(v, axis=1).astype(np.int16).reshape(-1) for k, v in rows.items()}


# the ghost telegrams
GHOST_RATE = (25, 16)  # 2.4 MS/s
# burst j: protocol j.  (With burst 1 at -500 kHz the restatement's receiver at +500 kHz does not decode the raw image -- a
# TFA_2 ghost is there at +500, -600 and +450 kHz and not at -400 or -550 -- so that burst sits at +500 kHz.)
GHOST_FREQS = (300000, 500000, 700000, -900000)
GHOST_BLOCKS = 6
GHOST_K = 2048
GHOST_IMPAIRMENT = (1.12, 8.0)  # an image at about -21 dBc


@functools.lru_cache(maxsize=None)
def ghost_scene():
    """(raw, x): the S16 row (read-only bytes) of the 2.4 MS/s scene with a burst of protocol j at GHOST_FREQS[j], its Q rail
    impaired by GHOST_IMPAIRMENT, and its x."""
    p, q = GHOST_RATE
    n = GHOST_BLOCKS * api.BLOCK_BYTES // 2 * p
    bursts = [dict(proto=j, start=(40000 * p + j * (n - 100000 * p) // len(GHOST_FREQS)) // q * q, payload_seed=21 + j, f0_hz=f, amp=50)
              for j, f in enumerate(GHOST_FREQS)]
    u = np.ascontiguousarray(synth.gen_scene(77, GHOST_BLOCKS, bursts, rate_mult=p).reshape(-1, 2)[::q]).reshape(-1)
    x = impair(tune.s16_of_u8(u), *GHOST_IMPAIRMENT)
    raw = formats.encode("s16", x)
    raw.setflags(write=False)
    x.setflags(write=False)
    return raw, x


def receiver_oracle(x, hz):
    """The oracle of the receiver with the input-rate tune hz on the input-rate samples x."""
    p, q = GHOST_RATE
    o = O.Oracle(TYPES, THRESH, 0)
    o.process_s16(resample.resample_x16(tune.mix_in_s16(x, hz, p, q), p, q))
    return o


@functools.lru_cache(maxsize=None)
def ghost_oracles(balanced):
    """The eight receivers' oracles, in the order +f0, -f0, +f1, ...: on the raw scene, or behind the balancer (K = GHOST_K)."""
    raw, x = ghost_scene()
    z = iqbal.iq_balance(raw, "s16", 0, GHOST_K)[0] if balanced else x
    return [receiver_oracle(z, sgn * f) for f in GHOST_FREQS for sgn in (1, -1)]
