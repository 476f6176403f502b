"""The harness the HIP-path tests share: feeding a Receiver through its submit FIFO, fresh oracles, and the comparisons of
drained events with the oracle's -- every field, per slot in order, seq, the bit log --; the runner of rate and format
receivers with its cutter, stage-0 comparison and input builders; the table of receiver modes; building and running tfrec_gpu;
the golden vectors' records and digests; the imports of a file, for the rule that no test module imports another.
Imported as a plain module (`import parity`) from the test modules and from tests/stress_gpu.py."""
import ast
import functools
import hashlib
import os
import subprocess

import numpy as np

from oracle import oracle as O
from tfrec_amd import api, formats, resample, synth, tune

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tfrec_amd", "host")
CLI = os.path.join(HOST, "tfrec_gpu")

MIN_BYTES = (10, 7, 7, 7, 11)  # per slot: the shortest flush the default mode reports
PREFIX = {0: "TFA1 ", 1: "TFA2 ", 2: "TFA3 ", 3: "TX22 ", 4: "WHB"}  # per slot: how its telegram lines start


def cut(iq, sizes, block=api.BLOCK_BYTES):
    """iq[n_streams, bytes] -> consecutive parts (views) of sizes[k] blocks each."""
    parts, pos = [], 0
    for nb in sizes:
        parts.append(iq[:, pos * block:(pos + nb) * block])
        pos += nb
    return parts


def cut_input(rows, sizes, fmt="u8", p=1, q=1):
    """rows[rows, bytes] -> consecutive contiguous parts of sizes[k] blocks each at the input rate p / q in the format; the rows
    are used up."""
    parts, pos = [], 0
    for nb in sizes:
        n = formats.bytes_per_sample(fmt) * resample.input_samples(nb, p, q)
        parts.append(np.ascontiguousarray(rows[:, pos:pos + n]))
        pos += n
    assert pos == rows.shape[1]
    return parts


def to_device(parts):
    import torch

    return [torch.from_numpy(h).to("cuda:0") for h in parts]


def device_parts(iq, sizes, block=api.BLOCK_BYTES):
    hosts = [np.ascontiguousarray(p) for p in cut(iq, sizes, block)]
    return to_device(hosts), hosts


def run_fifo(r, parts, depth=api.FIFO_DEPTH, before=None, after=None):
    """Submit parts[k] (numpy arrays or device tensors) in order with up to `depth` submits in flight: the oldest is drained
    only when `depth` are pending, the rest once every part is submitted.  before(k) runs ahead of submit k while the FIFO
    is still full, after(k) right after it.  depth=1 alternates submit and drain.  -> one drained array per submit, in
    order."""
    out = []
    for k, p in enumerate(parts):
        if before:
            before(k)
        if k - len(out) == depth:
            out.append(r.drain())
        r.submit(p)
        if after:
            after(k)
    while len(out) < len(parts):
        out.append(r.drain())
    return out


def sort_events(ev):
    return ev[np.lexsort((ev["seq"], ev["slot"], ev["stream"]))]


def reported(slot, byte_cnt):
    """Whether the default mode reports a flush: at least a telegram long, TX22 shorter than 64 bytes, WHB at most 60."""
    return byte_cnt >= MIN_BYTES[slot] and not (slot == 3 and byte_cnt >= 64) and not (slot == 4 and byte_cnt > 60)


def reported_mask(ev):
    """reported() over an event array (fields slot, byte_cnt)."""
    slot, n = ev["slot"], ev["byte_cnt"]
    return (n >= np.array(MIN_BYTES)[slot]) & ~((slot == 3) & (n >= 64)) & ~((slot == 4) & (n > 60))


def fresh_oracle(x, types, thresh, wide=0, in10x=False, log_bits=False, keep_dec=False):
    """A new oracle receiver run over one stream's input x (u8 bytes; in10x: 10x-rate bytes through oracle.decim10)."""
    o = O.Oracle(types, thresh, wide, log_bits=log_bits, keep_dec=keep_dec)
    if in10x:
        o.process_s16(O.decim10(x))
    else:
        o.process(x)
    return o


def by_slot(evs):
    d = {}
    for e in evs:
        d.setdefault(e[0], []).append(e)
    return d


def assert_stream(ev, s, orc, label=None, default_mode=False):
    """Stream s of the drained events against the oracle in every field -- rssi_raw (the accumulator itself, not only its
    dB value: BASELINE.md 3 "raw RSSI and offset integers identical") and status (the decoder's CRC / sanity verdict,
    computed on the GPU) included: the same slots, and per slot the same events in the same order.  default_mode: only the
    oracle's flushes the default mode reports.  -> events compared."""
    label = "stream %d" % s if label is None else label
    want = orc.events_full()
    if default_mode:
        want = [e for e in want if reported(e[0], e[2])]
    g, o = by_slot(api.event_tuples_full(ev, s)), by_slot(want)
    assert sorted(g) == sorted(o), label
    for slot in o:
        assert g[slot] == o[slot], "%s slot %d" % (label, slot)
    return sum(len(v) for v in o.values())


def assert_all_streams(ev, iq, types, thresh, all_flushes=True, wide=0, orc=None):
    """every stream of the batch against the oracle (OpenMP, one receiver per stream): vectorised comparison.
    orc: the oracle's events if they were computed already (one ORC_EVENT_DTYPE array per stream)"""
    if orc is None:
        orc = O.process_many(iq, types, thresh, wide)
    gs, gm = api.events_canon(ev)
    order = np.argsort(gs, kind="stable")  # (several drains concatenated: each is ordered by stream)
    gs, gm = gs[order], gm[order]
    bounds = np.searchsorted(gs, np.arange(len(orc) + 1))
    total = 0
    for s in range(len(orc)):
        e = orc[s]
        if not all_flushes:
            e = e[reported_mask(e)]
        wm = O.canon(e)
        wm = wm[np.lexsort((wm[:, 1], wm[:, 0]))]
        g = gm[bounds[s]:bounds[s + 1]]
        g = g[np.lexsort((g[:, 1], g[:, 0]))]
        assert g.shape == wm.shape and np.array_equal(g, wm), "stream %d" % s
        total += len(wm)
    return total


def oracle_bits(orc):
    """Oracle(log_bits=True).bits_text() ("W slot nbits bits": one record per flush, in flush order) -> {slot: [bits of
    each flush]}."""
    want = {}
    for ln in orc.bits_text().splitlines():
        p = ln.split()
        want.setdefault(int(p[1]), []).append(p[3] if len(p) > 3 else "")
    return want


def assert_bits(ev, s, orc, label):
    """TFREC_AMD_F_BITS: stream s's bits handed to decoder::store_bit, flush by flush, against the oracle's bit log.  -> bits
    compared."""
    got = api.bits_by_flush(ev, s)
    n = 0
    for slot, recs in oracle_bits(orc).items():
        for seq, bits in enumerate(recs):
            assert got.get((slot, seq), "") == bits, "%s slot %d flush %d" % (label, slot, seq)
            n += len(bits)
    return n


def assert_segment(ev, s, orc, label, bits=False):
    """Stream s's events of one segment (from its start or a restart on) against a fresh oracle over that segment's input,
    every flush reported: the events, seq = the flush ordinal since the restart, and with bits the bit log.  -> events
    compared."""
    n = assert_stream(ev, s, orc, label)
    flushes = ev[(ev["stream"] == s) & (ev["status"] != api.STATUS_BITS)]
    for slot in set(flushes["slot"].tolist()):
        seq = flushes[flushes["slot"] == slot]["seq"]
        assert np.array_equal(seq, np.arange(len(seq))), "%s slot %d seq" % (label, slot)
    if bits:
        assert_bits(ev, s, orc, label)
    return n


def status_pinned_by_text(full, text, label):
    """The per-event verdict (status, the 8th field of events_full tuples) against a telegram text: every flush the decoder
    accepts prints exactly one telegram line (tfa1.cpp:89, tfa2.cpp:169/249, whb.cpp:126-475), per protocol; a flush the
    default mode would not report is 0, everything else 2."""
    lines = text.splitlines()
    for slot, prefix in PREFIX.items():
        n = len([ln for ln in lines if ln.startswith(prefix) and not ln.startswith("WHB:")])
        assert sum(1 for e in full if e[0] == slot and e[7] == 1) == n, (label, prefix)
    for e in full:
        assert (e[7] == 0) == (not reported(e[0], e[2])), label


# ---- rate and format receivers
def run_input(rows, sizes, p=1, q=1, fmt=None, *, types, thresh, host=False, before=None, n_streams=None, stage0=True, **kw):
    """A receiver of the format at the input rate p / q over the rows cut into `sizes` -> (one drained array per submit, the
    receiver's stage 0 per submit and stream).  fmt None: the receiver of the older constructors (u8; input_rate only, or
    neither at 1/1).  before(r, k) runs ahead of submit k.  stage0=False: nothing is read back between the submits, and they
    queue up to the FIFO's depth."""
    parts = cut_input(rows, sizes, fmt or "u8", p, q)
    n = len(rows) if n_streams is None else n_streams
    y0 = []
    if fmt is not None:
        kw["input_format"] = fmt
    if fmt is not None or (p, q) != (1, 1):
        kw["input_rate"] = (p, q)
    with api.Receiver(n, types, thresh, 0, max_blocks=max(sizes), **kw) as r:
        assert r.input_rate == (p, q) and r.input_format == (fmt or "u8")
        for k, nb in enumerate(sizes):
            assert r.input_bytes(nb) == parts[k].shape[1] and parts[k].shape[1] % 16 == 0

        def after(k):
            y0.append([r.stage0(s, sizes[k] * 4 * api.BLOCK_DEC) for s in range(n)])

        evs = run_fifo(r, parts if host else to_device(parts), before=(lambda k: before(r, k)) if before else None,
                       after=after if stage0 else None)
    return evs, y0


def first_difference(got, want, tile):
    """Where two stage-0 arrays first differ, as the output index and its place in the tile and in the lane's eight outputs."""
    d = np.nonzero(got != want)[0] if len(got) == len(want) else ()
    if not len(d):
        return "lengths %d and %d" % (len(got), len(want))
    m = int(d[0]) // 2
    return "first differing output %d (mod %d: %d, mod 8: %d), %d values differ" % (m, tile, m % tile, m % 8, len(d))


def assert_stage0(y0, sizes, want, s, label="", tile=None, first=0):
    """Stage 0 of stream s, submit by submit from submit `first` on, against `want`: the restatement from that submit on, used
    up by the last.  tile: the kernel's tile, for the message."""
    pos = 0
    for k in range(first, len(sizes)):
        n = 2 * sizes[k] * 4 * api.BLOCK_DEC
        got, w = y0[k][s], want[pos:pos + n]
        assert np.array_equal(got, w), "%s stream %d submit %d%s" % (
            label, s, k, ": " + first_difference(got, w, tile) if tile else "")
        pos += n
    assert pos == len(want), "%s stream %d: %d values expected behind submit %d" % (label, s, len(want) - pos, len(sizes) - 1)


# mode -> (what it sets among the Receiver's keywords, the expected layout(), the flags for the harness)
MODES = {"deep": ({}, 6, {}), "shallow": ({"experiments": True}, 4, {}), "serial_chains": ({"serial_chains": True}, 2, {}),
         "default_mode": ({"all_flushes": False}, 6, {"default_mode": True}), "bits": ({"bits": True}, 6, {"bits": True}),
         "host": ({}, 6, {"host": True})}


def mode_kwargs(mode, monkeypatch):
    """-> (Receiver keywords, the expected layout(), harness flags: bits, default_mode, host).  shallow is the experiments
    build of the library with TFREC_AMD_DEEP=0 (only that build reads the variable)."""
    own, layout, flags = MODES[mode]
    if mode == "shallow":
        monkeypatch.setenv("TFREC_AMD_DEEP", "0")
    kw = dict(dict(all_flushes=True, bits=False, serial_chains=False, experiments=False), **own)
    return kw, layout, dict(dict(bits=False, default_mode=False, host=False), **flags)


def loud_and_quiet(p, q, sizes, n_streams, seed):
    """[streams, bytes] u8 for a stage-0 test: near-silence with stretches of full-scale random bytes at the start and across
    every boundary between two submits, so that the history carry moves samples that matter and every rail value occurs."""
    rng = np.random.default_rng(seed)
    n = resample.input_samples(sum(sizes), p, q)
    x = rng.integers(125, 132, (n_streams, 2 * n), dtype=np.uint8)
    pos = 0
    for nb in (0,) + tuple(sizes[:-1]):
        pos += 2 * resample.input_samples(nb, p, q) if nb else 0
        lo, hi = max(0, pos - 3000), min(2 * n, pos + 3000)
        x[:, lo:hi] = rng.integers(0, 256, (n_streams, hi - lo), dtype=np.uint8)
    x[:, 2 * n - 400:] = rng.integers(0, 256, (n_streams, 400), dtype=np.uint8)
    return x


def full_scale_row(fmt, n, seed):
    """[1, bytes]: n complex samples that use the format's whole range (f32: beyond it, so that the clamp works)."""
    rng = np.random.default_rng(seed)
    if fmt == "s8":
        return rng.integers(0, 256, (1, 2 * n), dtype=np.uint8)
    if fmt == "s16":
        return rng.integers(-32768, 32768, (1, 2 * n)).astype("<i2").view(np.uint8)
    return (rng.random((1, 2 * n), dtype=np.float32) * np.float32(2.4) - np.float32(1.2)).astype("<f4").view(np.uint8)


@functools.lru_cache(maxsize=None)
def tuned_row(p, q, freqs, fmt="u8", n_blocks=6):
    """[1, bytes] (read-only): one u8 or s16 recording at 1536000 p / q with a burst of its own protocol at each of freqs (Hz from
    the centre)."""
    n = n_blocks * api.BLOCK_BYTES // 2 * p
    bursts = [dict(proto=j, start=(40000 * p + j * (n - 100000 * p) // len(freqs)) // q * q, payload_seed=21 + j, f0_hz=f, amp=50)
              for j, f in enumerate(freqs)]
    u = np.ascontiguousarray(synth.gen_scene(77, n_blocks, bursts, rate_mult=p).reshape(-1, 2)[::q]).reshape(-1)
    if fmt == "u8":
        row = u.reshape(1, -1)
    else:
        assert fmt == "s16"
        v = ((u.astype(np.int32) - 128) << 8) + np.random.default_rng(9).integers(-128, 128, u.shape)
        row = np.clip(v, -32768, 32767).astype("<i2").view(np.uint8).reshape(1, -1)
    row.setflags(write=False)
    return row


@functools.lru_cache(maxsize=None)
def tuned_oracle(p, q, freqs, fmt="u8", input_hz=0, narrow_hz=0, *, types, thresh):
    """The oracle behind the restatement of one receiver on tuned_row: the mixer at the input rate, the stage, the tune behind it."""
    x = formats.to_x(fmt, tuned_row(p, q, freqs, fmt)[0])
    o = O.Oracle(types, thresh, 0)
    o.process_s16(tune.mix_s16(resample.resample_x16(tune.mix_in_s16(x, input_hz, p, q), p, q), narrow_hz, 0))
    return o


def decoded(orc):
    """The slots of the telegrams an oracle decoded, in order."""
    return [e[0] for e in orc.events_full() if e[7] == 1]


# ---- tfrec_gpu
def telegram_lines(text):
    return [ln for ln in text.splitlines() if ln.startswith(tuple(PREFIX.values())) and not ln.startswith("WHB:")]


def build_cli():
    """Build the device library and tfrec_gpu -> the CLI's path."""
    from tfrec_amd import _build
    _build.build_device_lib()
    subprocess.check_call(["make", "-s", "-C", HOST])
    return CLI


def run_cli(args, timeout=120):
    """tfrec_gpu, whatever its exit status -> the CompletedProcess."""
    return subprocess.run([CLI] + args, capture_output=True, text=True, timeout=timeout)


def cli_stdout(args, timeout=600):
    out = subprocess.run([CLI] + args, capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stderr
    return out.stdout


def cli(args, sink, timeout=600):
    """tfrec_gpu with the batched sink -E writing to `sink` -> (stdout, the sink's records split in fields, without the time
    stamp)."""
    out = subprocess.run([CLI] + args + ["-E", "cat > %s" % sink], capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stderr
    return out.stdout, [ln.split()[:-1] for ln in open(sink).read().splitlines()]


# ---- the golden vectors (tests/golden/*.json)
def golden_data(recs):
    return [(r[0], r[1], int(r[2], 16), float.fromhex(r[3]), float.fromhex(r[4]), r[5], r[6], r[7], r[8]) for r in recs]


def sha256_of(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


# ---- the import rule
def imports_of(path, source=None):
    """The top-level names of every module a file imports, anywhere in it (source: the text to parse in the file's place)."""
    out = set()
    for node in ast.walk(ast.parse(open(path).read() if source is None else source, path)):
        if isinstance(node, ast.Import):
            out |= {a.name.split(".")[0] for a in node.names}
        elif isinstance(node, ast.ImportFrom) and node.module and node.level == 0:
            out.add(node.module.split(".")[0])
    return out
