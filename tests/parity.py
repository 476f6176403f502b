"""The harness the HIP-path tests share: feeding a Receiver through its submit FIFO, fresh oracles, and the comparisons of
drained events with the oracle's -- every field, per slot in order, seq, the bit log -- plus building and running tfrec_gpu.
Imported as a plain module (`import parity`) from the test modules and from tests/stress_gpu.py."""
import os
import subprocess

import numpy as np

from oracle import oracle as O
from tfrec_amd import api

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


def fresh_oracle(x, types, thresh, wide=0, in10x=False, log_bits=False):
    """A new oracle receiver run over one stream's input x (u8 bytes; in10x: 10x-rate bytes through oracle.decim10)."""
    o = O.Oracle(types, thresh, wide, log_bits=log_bits)
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


def build_cli():
    """Build the device library and tfrec_gpu -> the CLI's path."""
    from tfrec_amd import _build
    _build.build_device_lib()
    subprocess.check_call(["make", "-s", "-C", HOST])
    return CLI


def cli(args, sink, timeout=600):
    """tfrec_gpu with the batched sink -E writing to `sink` -> (stdout, the sink's records split in fields, without the time
    stamp)."""
    out = subprocess.run([CLI] + args + ["-E", "cat > %s" % sink], capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stderr
    return out.stdout, [ln.split()[:-1] for ln in open(sink).read().splitlines()]
