"""Deterministic synthetic 8-bit IQ streams (ctypes binding of iqgen.c).

Test/bench signal source only: produces the raw u8 interleaved IQ format the reference records
with ``-S`` and replays with ``-L`` (sdr.cpp:233-234, engine.cpp:67-81).  Recipes: SURVEY.md App. C.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_HERE, "libiqgen.so")
_SRC = os.path.join(_HERE, "iqgen.c")

PROTO_NAMES = ("TFA_1", "TFA_2", "TFA_3", "TX22", "WHB")
BLOCK_BYTES = 65536


class Truth(C.Structure):
    _fields_ = [
        ("proto", C.c_int32),
        ("nbytes", C.c_int32),
        ("start", C.c_int64),
        ("length", C.c_int64),
        ("amp_q4", C.c_int32),
        ("f0_hz", C.c_int32),
        ("frame", C.c_uint8 * 64),
    ]


class Burst(C.Structure):
    _fields_ = [
        ("proto", C.c_int32),
        ("corrupt", C.c_int32),
        ("start", C.c_int64),
        ("amp_q4", C.c_int32),
        ("f0_hz", C.c_int32),
        ("baud_ppm", C.c_int32),
        ("fdev_hz", C.c_int32),
        ("repeats", C.c_int32),
        ("repeat_gap", C.c_int32),
        ("nbytes", C.c_int32),
        ("pad", C.c_int32),
        ("payload_seed", C.c_uint64),
        ("frame", C.c_uint8 * 64),
    ]


def build(force: bool = False) -> str:
    if force or not os.path.exists(_SO) or os.path.getmtime(_SO) < os.path.getmtime(_SRC):
        subprocess.check_call(
            ["gcc", "-O2", "-std=c11", "-fopenmp", "-fPIC", "-shared", "-Wall", "-o", _SO, _SRC]
        )
    return _SO


_lib = None


def _load():
    global _lib
    if _lib is None:
        build()
        lib = C.CDLL(_SO)
        lib.iqgen_stream.restype = C.c_int
        lib.iqgen_stream.argtypes = [C.c_uint64, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                     C.POINTER(Truth), C.c_int]
        lib.iqgen_stream_rate.restype = C.c_int
        lib.iqgen_stream_rate.argtypes = [C.c_uint64, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                          C.POINTER(Truth), C.c_int, C.c_int]
        lib.iqgen_stream_ex.restype = C.c_int
        lib.iqgen_stream_ex.argtypes = [C.c_uint64, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                        C.POINTER(Truth), C.c_int, C.c_int, C.c_int]
        lib.iqgen_scene.restype = C.c_int
        lib.iqgen_scene.argtypes = [C.c_uint64, C.c_int, C.POINTER(Burst), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                    C.c_void_p, C.POINTER(Truth), C.c_int]
        lib.iqgen_batch.restype = C.c_int
        lib.iqgen_batch.argtypes = [C.c_uint64, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
        _lib = lib
    return _lib


def gen_stream(seed: int, stream: int, n_blocks: int, proto_mask: int = 0x1F, noise_q8: int = 256,
               with_truth: bool = False, rate_mult: int = 1, corrupt_every: int = 0):
    """One stream of ``n_blocks`` blocks of 65536*rate_mult bytes -> uint8 array (and the planted bursts).
    rate_mult 10 = the 15.36 MS/s input of BASELINE config 5.  corrupt_every = c > 0: every c-th burst carries a planted
    fault (wrong checksum / right checksum but a field the decoder's sanity test rejects / frame cut short, in turn)."""
    lib = _load()
    out = np.empty(n_blocks * BLOCK_BYTES * rate_mult, dtype=np.uint8)
    cap = 4096
    truth = (Truth * cap)()
    n = lib.iqgen_stream_ex(seed, stream, n_blocks, proto_mask, noise_q8, out.ctypes.data, truth, cap, rate_mult,
                            corrupt_every)
    if not with_truth:
        return out
    recs = []
    for k in range(min(n, cap)):
        t = truth[k]
        recs.append(dict(proto=t.proto, start=t.start, length=t.length, amp=t.amp_q4 / 16.0, f0_hz=t.f0_hz,
                         frame=bytes(t.frame[: t.nbytes])))
    return out, recs


def _truth_records(truth, n):
    return [dict(proto=t.proto, start=t.start, length=t.length, amp=t.amp_q4 / 16.0, f0_hz=t.f0_hz,
                 frame=bytes(t.frame[: t.nbytes])) for t in truth[:n]]


def gen_scene(seed: int, n_blocks: int, bursts, noise_q8: int = 256, dc_iq=(0, 0), rate_mult: int = 1,
              with_truth: bool = False):
    """One stream of ``n_blocks`` blocks holding an explicit list of bursts (dicts) -> uint8 array (and one truth record
    per planted copy, as gen_stream(with_truth=True)).  Burst keys: proto, start (input sample); payload ``frame`` (bytes,
    sync and checksum included) or ``payload_seed``; amp (LSB, default 60), f0_hz (0), baud_ppm (0: the nominal bit rate;
    +N: N ppm faster), fdev_hz (45000, FSK protocols), corrupt (0; the faults of gen_stream's corrupt_every), repeats (1)
    and repeat_gap (input samples from the end of one copy to the start of the next).  Overlapping bursts add up before
    the quantiser clips; dc_iq shifts the I / Q rails by whole LSB.  Integer arithmetic only: the bytes are the same on
    every machine."""
    lib = _load()
    bursts = list(bursts)
    arr = (Burst * max(1, len(bursts)))()
    for k, b in enumerate(bursts):
        unknown = set(b) - {"proto", "start", "frame", "payload_seed", "amp", "f0_hz", "baud_ppm", "fdev_hz", "corrupt",
                            "repeats", "repeat_gap"}
        assert not unknown, unknown
        t = arr[k]
        t.proto = int(b["proto"])
        t.start = int(b["start"])
        t.amp_q4 = int(round(b.get("amp", 60) * 16))
        t.f0_hz = int(b.get("f0_hz", 0))
        t.baud_ppm = int(b.get("baud_ppm", 0))
        t.fdev_hz = int(b.get("fdev_hz", 45000))
        t.corrupt = int(b.get("corrupt", 0))
        t.repeats = int(b.get("repeats", 1))
        t.repeat_gap = int(b.get("repeat_gap", 0))
        t.payload_seed = int(b.get("payload_seed", 0))
        fr = bytes(b.get("frame", b""))
        assert len(fr) <= 64
        t.nbytes = len(fr)
        for i, v in enumerate(fr):
            t.frame[i] = v
    out = np.empty(n_blocks * BLOCK_BYTES * rate_mult, dtype=np.uint8)
    cap = 4096
    truth = (Truth * cap)()
    n = lib.iqgen_scene(seed, n_blocks, arr, len(bursts), noise_q8, int(dc_iq[0]), int(dc_iq[1]), rate_mult,
                        out.ctypes.data, truth, cap)
    return (out, _truth_records(truth, min(n, cap))) if with_truth else out


def burst_length(proto: int, nbytes: int, baud_ppm: int = 0, rate_mult: int = 1) -> int:
    """Input samples of one copy of a burst carrying an nbytes frame (iqgen.c burst_bits + burst_len)."""
    nbits = {0: 200 + 8 * nbytes + 48, 1: 8 + 8 * nbytes + 2, 2: 24 + 8 * nbytes + 2, 3: 16 + 8 * nbytes + 2,
             4: 200 + 8 * nbytes + 24}[proto]
    baud = (38400, 17240, 9600, 8842, 6000)[proto]
    den = baud * (1000000 + baud_ppm)
    return (nbits * 1536000 * rate_mult * 1000000 + den - 1) // den


def gen_batch(seed: int, first_stream: int, n_streams: int, n_blocks: int, proto_mask: int = 0x1F,
              noise_q8: int = 256, out: np.ndarray | None = None) -> np.ndarray:
    """``n_streams`` streams, shape [n_streams, n_blocks*65536] uint8 (OpenMP over streams)."""
    lib = _load()
    if out is None:
        out = np.empty((n_streams, n_blocks * BLOCK_BYTES), dtype=np.uint8)
    assert out.dtype == np.uint8 and out.flags.c_contiguous and out.size == n_streams * n_blocks * BLOCK_BYTES
    lib.iqgen_batch(seed, first_stream, n_streams, n_blocks, proto_mask, noise_q8, out.ctypes.data)
    return out
