"""A CPU restatement of the biquad passes' speculate-and-repair ladder (tfrec_amd/csrc/biquad.h: K3a speculative run, K3b
repair, K3b' second repair, K3c serial repair) beside the true trajectory -- one iir2 run over a chain's in-window samples.
From a stream's decimated samples, the submit cuts, the types, the threshold and a segment length it gives, per biquad chain
(slots 1-3: the TFA_2 family, slot 4: WHB stage 1) and per submit, the windows, the window-relative output row as the ladder
leaves it, the true row, which pass wrote each slot last, and a census of what every rung did.  The rungs decide as the kernels
do; the inner loops are tests/ladder_core.c.  Imported as a plain module (`import ladder_model`) like parity and segments."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

from oracle import oracle as O
from oracle import scenes as S

HERE = os.path.dirname(os.path.abspath(__file__))
CORE_C = os.path.join(HERE, "ladder_core.c")
BUILD = os.path.join(os.path.dirname(HERE), "oracle", "_build")
CORE_SO = os.path.join(BUILD, "ladder_core.so")
GCC_FLAGS = ["-O2", "-ffp-contract=off", "-std=c11", "-Wall"]

BAUD = {1: 17240, 2: 9600, 3: 8842, 4: 6000}  # main.cpp:173-218
BIQUAD_SLOTS = (1, 2, 3, 4)
NAMES = {1: "TFA_2", 2: "TFA_3", 3: "TX22", 4: "WHB"}
CK_EVERY = 4  # biquad.h: TFREC_AMD_CK_EVERY
CENSUS = ("segments", "k3b_unconverged", "k3b2_run", "k3b2_unconverged", "serial", "serial_joined", "serial_to_end",
          "serial_hops", "k3b_slots")
RUNGS = ("none", "K3a", "K3b", "K3b'", "K3c")
# tfrec_amd_stats field -> census entry
STATS = {"biquad_segments": "segments", "biquad_unconverged": "k3b_unconverged", "biquad_serial": "serial",
         "biquad_repair_slots": "k3b_slots"}


class State(C.Structure):
    _fields_ = [("dn1", C.c_double), ("dn2", C.c_double), ("yn", C.c_double), ("yn1", C.c_double)]

    def bits(self):
        return bytes(self)


def type_bit(slot):
    return 1 << (slot if slot < 4 else 5)


def cutoff(slot):
    """iir2's argument: tfa2.cpp:321 (0.5 / spb), whb.cpp:610 (2.0 / spb); spb = 384000 / baud."""
    spb = (1536000 / 4.0) / BAUD[slot]
    return (2.0 if slot == 4 else 0.5) / spb


def coefficients(slot):
    c = (C.c_double * 5)()
    O.lib().orc_iir_coeffs(cutoff(slot), c)
    return c


_core = None


def core():
    global _core
    if _core is None:
        O.lib()  # (makes oracle/_build)
        if not os.path.exists(CORE_SO) or os.path.getmtime(CORE_SO) < os.path.getmtime(CORE_C):
            tmp = "%s.%d" % (CORE_SO, os.getpid())
            subprocess.check_call(["gcc"] + GCC_FLAGS + ["-shared", "-fPIC", "-o", tmp, CORE_C])
            os.replace(tmp, CORE_SO)
        L = C.CDLL(CORE_SO)
        L.lm_inputs.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.lm_inputs.restype = None
        L.lm_chain.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_double), C.c_int, C.c_int,
                               C.c_int, C.c_int, C.POINTER(State), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(State),
                               C.POINTER(State), C.POINTER(C.c_long)]
        _core = L
    return _core


def chain_input(dec, slot):
    """The chain's input at every decimated sample of a stream from its start or a restart (dec: interleaved int16): the TFA_2
    family's fm_dev (dsp_stuff.cpp:284-292) as the int16 the discriminator pass stores, WHB's fm_dev_nrzs (:269-279); the sample
    ahead of the first one is zero, and across submits it is the sample before (T.prevdec)."""
    d = np.ascontiguousarray(dec, dtype=np.int16)
    x = np.empty(len(d) // 2, dtype=np.int32)
    fn = O.lib().orc_fm_dev_nrzs if slot == 4 else O.lib().orc_fm_dev
    core().lm_inputs(C.cast(fn, C.c_void_p), d.ctypes.data, len(x), 0, 0, int(slot != 4), x.ctypes.data)
    return x


def submit_windows(wins, lo, hi):
    """The windows [(open, close)] of a chain as the submit [lo, hi) sees them -> [(first sample, samples)] relative to lo: a
    window left open by the submit before continues as window 0 from sample 0 (windows.h: timeout_carry)."""
    out = []
    for a, b in wins:
        if b < lo or a >= hi:
            continue
        og = max(a, lo) - lo
        out.append((og, min(b, hi - 1) - lo - og + 1))
    return out


class ChainSubmit:
    """One chain in one submit: windows [(og, n)], row / true_row (int32 [row_slots * 32]), rung (uint8 [row_slots]), census
    (dict), start / ladder_end / true_end (State), index (the row positions of the in-window samples, in order)."""

    def __init__(self, slot, k, windows, row_slots):
        self.slot, self.k, self.windows = slot, k, windows
        self.row = np.full(row_slots * 32, -(1 << 31), dtype=np.int32)
        self.true_row = self.row.copy()
        self.rung = np.zeros(row_slots, dtype=np.uint8)
        self.index = (np.concatenate([((og >> 5) + j) * 32 + np.arange(n) for j, (og, n) in enumerate(windows)])
                      if windows else np.zeros(0, dtype=np.int64))

    def where(self, pos):
        """Row position -> "window j slot i (row slot r) sample g, last written by <rung>"."""
        r = int(pos) // 32
        for j, (og, n) in enumerate(self.windows):
            s0 = (og >> 5) + j
            if s0 <= r < s0 + (n + 31) // 32:
                return "%s submit %d window %d slot %d (row slot %d) sample %d, last written by %s" % (
                    NAMES[self.slot], self.k, j, r - s0, r, og + int(pos) - 32 * s0, RUNGS[self.rung[r]])
        return "%s submit %d row slot %d: outside every window" % (NAMES[self.slot], self.k, r)

    def first_difference(self, got):
        """None, or where the in-window values of a row differ first from the true trajectory."""
        d = np.nonzero(np.asarray(got)[self.index] != self.true_row[self.index])[0]
        return None if not len(d) else "%s: %d values differ" % (self.where(self.index[d[0]]), len(d))


def run_chain(x, windows, slot, seg_slots, row_slots, start, k=0, ck_every=CK_EVERY):
    """The ladder over one submit of one chain.  x: the chain's input per sample of the submit; start: the carried State."""
    res = ChainSubmit(slot, k, windows, row_slots)
    x = np.ascontiguousarray(x, dtype=np.int32)
    og = np.array([w[0] for w in windows], dtype=np.int32)
    nn = np.array([w[1] for w in windows], dtype=np.int32)
    census = (C.c_long * len(CENSUS))()
    res.start, res.ladder_end, res.true_end = State.from_buffer_copy(bytes(start)), State(), State()
    rc = core().lm_chain(x.ctypes.data, len(x), len(windows), og.ctypes.data, nn.ctypes.data, coefficients(slot), int(slot == 4),
                         seg_slots, ck_every, row_slots, C.byref(res.start), res.row.ctypes.data, res.true_row.ctypes.data,
                         res.rung.ctypes.data, C.byref(res.ladder_end), C.byref(res.true_end), census)
    assert rc == 0, "lm_chain: %d" % rc
    res.census = dict(zip(CENSUS, (int(v) for v in census)))
    return res


def run_stream(dec, cuts, types, thresh, seg_slots, max_blocks=None, ck_every=CK_EVERY, inputs=None):
    """A stream from its start or a restart.  dec: its decimated samples (interleaved int16, sum(cuts) blocks); cuts: the blocks of
    each submit; a fixed threshold.  -> {slot: [ChainSubmit per submit]} for the biquad chains among the types.  The state
    carried from submit to submit is the TRUE end state (the ladder's own is beside it in every ChainSubmit).  inputs: {slot:
    chain_input(dec, slot)} where they are at hand."""
    assert thresh > 0
    dec = np.ascontiguousarray(dec, dtype=np.int16)
    assert len(dec) == 2 * S.BLOCK_DEC * sum(cuts)
    row_slots = S.table_sizes(S.BLOCK_DEC * (max_blocks or max(cuts)))["slots"]
    trig = S.trigger_samples(dec, thresh)
    bounds = np.cumsum([0] + list(cuts)) * S.BLOCK_DEC
    out = {}
    for slot in BIQUAD_SLOTS:
        if not types & type_bit(slot):
            continue
        x = inputs[slot] if inputs is not None else chain_input(dec, slot)
        wins = S.windows(trig, S.WINDOW[slot])
        state, out[slot] = State(), []
        for k, (lo, hi) in enumerate(zip(bounds, bounds[1:])):
            res = run_chain(x[lo:hi], submit_windows(wins, int(lo), int(hi)), slot, seg_slots, row_slots, state, k, ck_every)
            out[slot].append(res)
            state = res.true_end
    return out


def total_census(results):
    """Sum of the census over an iterable of ChainSubmit."""
    tot = dict.fromkeys(CENSUS, 0)
    for r in results:
        for key in CENSUS:
            tot[key] += r.census[key]
    return tot


def expected_stats(models):
    """models: run_stream results (one per stream) -> the four tfrec_amd_stats counters the biquad passes add up."""
    tot = total_census(r for m in models for chain in m.values() for r in chain)
    return {name: tot[key] for name, key in STATS.items()}


def dump_chain(path, x, windows, slot, seg_slots, row_slots, start, ck_every=CK_EVERY):
    """One chain submit as the stand-alone build of ladder_core.c reads it (-DLADDER_MAIN)."""
    with open(path, "wb") as f:
        f.write(np.array([len(x), len(windows), int(slot == 4), seg_slots, ck_every, row_slots], dtype=np.int32).tobytes())
        f.write(bytes(coefficients(slot)))
        f.write(bytes(start))
        f.write(np.array([w[0] for w in windows], dtype=np.int32).tobytes())
        f.write(np.array([w[1] for w in windows], dtype=np.int32).tobytes())
        f.write(np.ascontiguousarray(x, dtype=np.int32).tobytes())


# ------------------------------------------------------------------------------------------------ the frozen inputs
N_BLOCKS = 6
THRESH = 500
CUTS = (1, 3, 2)


def _noise(rng, level, n):
    """The sum of four uniform integers in [-level, level]: integer-only and bell-shaped."""
    return rng.integers(-level, level + 1, (4, n)).sum(0)


def _row(kind, seed, n):
    """One input row of n bytes, from a generator of its own:
    ("noise", level)           128 + _noise: in a trigger window at every decimated sample at the levels used;
    ("bytes",)                 uniform random bytes;
    ("gate", period, k, level) uniform random bytes while (byte // period) % k == 0, 128 + _noise(level) (level 0: 128) between:
                               the gated rows of test_gpu_parity._stress_batch, windows that switch every period / 2 input samples;
    ("burst", stream)          an ordinary burst stream;  ("silence",)"""
    from tfrec_amd import synth

    rng = np.random.default_rng(seed)
    if kind[0] == "noise":
        return np.clip(128 + _noise(rng, kind[1], n), 0, 255).astype(np.uint8)
    if kind[0] == "bytes":
        return rng.integers(0, 256, n, dtype=np.uint8)
    if kind[0] == "gate":
        _, period, k, level = kind
        r = rng.integers(0, 256, n, dtype=np.uint8)
        back = np.clip(128 + _noise(rng, level, n), 0, 255) if level else 128
        return np.where((np.arange(n) // period) % k == 0, r, back).astype(np.uint8)
    if kind[0] == "burst":
        return synth.gen_stream(seed, kind[1], n // 65536, 0x1F, 256)
    assert kind[0] == "silence"
    return np.full(n, 128, np.uint8)


# The rows and seeds are chosen so that the model's census at 16 slots meets the conditions of tests/test_biquad_ladder_cpu.py: the
# TFA_3 and TX22 chains of every always-triggered row send half their segments to the serial repair; WHB's serial repairs are rare
# (about one per six always-triggered rows, nearly all of which join a checkpoint), so the noise seeds 49 and 129 and the gated
# rows with seeds 101 and 71 are ones whose WHB chain has a serial repair that runs to its segment's end, and the rows gated every
# 2500 samples are ones whose WHB chain has a serial repair across a window boundary.
FROZEN = ((("noise", 24), 49), (("noise", 24), 129), (("noise", 24), 3), (("noise", 48), 4), (("noise", 48), 5),
          (("noise", 96), 6), (("noise", 96), 7),
          (("bytes",), 8), (("bytes",), 9), (("bytes",), 10),
          (("gate", 3000, 2, 0), 11), (("gate", 1700, 3, 1), 101), (("gate", 2400, 2, 6), 71),
          (("gate", 5000, 2, 0), 0), (("gate", 5000, 2, 0), 5), (("gate", 5000, 2, 0), 6),
          (("burst", 0), 77), (("burst", 1), 77), (("silence",), 0))
ALWAYS_TRIGGERED = tuple(range(10))  # rows of FROZEN inside a window at every decimated sample ahead of their silent tail
TAIL_BYTES = 8 * 1024               # 1024 decimated samples of silence: longer than every chain's window


def frozen_batch():
    """[19, 6 blocks] u8 (read-only): the inputs of tests/test_biquad_ladder_cpu.py and tests/test_biquad_ladder_gpu.py."""
    iq = np.stack([_row(kind, seed, N_BLOCKS * 65536) for kind, seed in FROZEN])
    iq[list(ALWAYS_TRIGGERED), -TAIL_BYTES:] = 128  # their windows close once, so that every chain of them flushes
    iq.setflags(write=False)
    return iq


@functools.lru_cache(maxsize=None)
def frozen_oracles():
    """One oracle per row of frozen_batch (every type, THRESH, its decimated samples kept) and the rows' chain inputs."""
    import parity

    orcs = [parity.fresh_oracle(x, 0x2F, THRESH, keep_dec=True) for x in frozen_batch()]
    decs = [o.dec() for o in orcs]
    return orcs, decs, [{slot: chain_input(d, slot) for slot in BIQUAD_SLOTS} for d in decs]


@functools.lru_cache(maxsize=None)
def frozen_models(seg_slots, types=0x2F, cuts=CUTS, rows=None):
    """run_stream over the rows of frozen_batch (all, or the tuple given) -> one result per row."""
    _, decs, xs = frozen_oracles()
    return [run_stream(decs[s], cuts, types, THRESH, seg_slots, inputs=xs[s]) for s in (range(len(decs)) if rows is None else rows)]
