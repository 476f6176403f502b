"""Save / load of a stream's state without a GPU: the exports and the blob header's layout against tfrec_amd/state.py,
the argument checks that need no device, tfrec_gpu's -k / -K usage errors (exit status 2 before a device is opened) and the byte plan of
tfrec_amd/host/job.h -- tests/state_plan_driver.cpp, compiled here with the address and undefined-behaviour sanitizers and run as a
child process."""
import ctypes as C
import os
import random
import re
import subprocess

import numpy as np
import pytest

import parity
from tfrec_amd import api, state

ROOT = parity.ROOT
HEADER = os.path.join(ROOT, "include", "tfrec_amd.h")


def test_the_three_calls_are_declared_exported_and_bound():
    hdr = open(HEADER).read()
    L = api.load_library()
    for name in ("tfrec_amd_stream_state_bytes", "tfrec_amd_save_streams", "tfrec_amd_load_streams"):
        assert re.search(r"\bint %s\s*\(" % name, hdr) and name in api.EXPORTS
        assert getattr(L, name) is not None and getattr(api.load_library(experiments=True), name) is not None
    for name in ("state_bytes", "save_streams", "load_streams"):
        assert hasattr(api.Receiver, name)
    # no context: refused before anything is touched
    n = C.c_size_t(7)
    idx = np.zeros(1, dtype=np.int32)
    buf = np.zeros(256, dtype=np.uint8)
    assert L.tfrec_amd_stream_state_bytes(None, C.byref(n)) == api.E_INVAL and n.value == 7
    assert L.tfrec_amd_save_streams(None, idx.ctypes.data, 1, buf.ctypes.data, buf.nbytes) == api.E_INVAL
    assert L.tfrec_amd_load_streams(None, idx.ctypes.data, 1, buf.ctypes.data, buf.nbytes) == api.E_INVAL


def test_header_layout_in_the_c_header_equals_state_py(tmp_path):
    """sizeof and every offsetof of tfrec_amd_state_header, printed by a C program, against state.HEADER_DTYPE; the magic and the
    format too."""
    names = [n for n in state.HEADER_DTYPE.names]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "tfrec_amd.h"\nint main(void)\n{\n'
                   '\tprintf("SIZE %zu\\nMAGIC %u\\nFORMAT %u\\n", sizeof(tfrec_amd_state_header), TFREC_AMD_STATE_MAGIC, TFREC_AMD_STATE_FORMAT);\n'
                   + "".join('\tprintf("%s %%zu %%zu\\n", offsetof(tfrec_amd_state_header, %s), sizeof(((tfrec_amd_state_header *)0)->%s));\n'
                             % (n, n, n) for n in names)
                   + "\treturn 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)])
    out = dict(ln.split(None, 1) for ln in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(out.pop("SIZE")) == state.HEADER_BYTES == state.HEADER_DTYPE.itemsize == 128
    assert int(out.pop("MAGIC")) == state.MAGIC == int.from_bytes(b"TFST", "little") and int(out.pop("FORMAT")) == state.FORMAT
    for n in names:
        dt, off = state.HEADER_DTYPE.fields[n][:2]
        assert tuple(int(v) for v in out[n].split()) == (off, dt.itemsize), n
    # the signature is one run of fields between the version hash and the payload size
    sig = [state.HEADER_DTYPE.fields[n][1] for n in state.SIGNATURE_FIELDS]
    assert sig == list(range(16, 68, 4)) and state.HEADER_DTYPE.fields["payload_bytes"][1] == 68
    assert C.sizeof(api.StreamConfig) == state.HEADER_DTYPE.fields["config"][0].itemsize == 16


def test_parser_and_version_hash():
    assert state.version_hash(b"") == 0xCBF29CE484222325 and state.version_hash(b"a") == 0xAF63DC4C8601EC8C  # FNV-1a's vectors
    h = np.zeros(1, dtype=state.HEADER_DTYPE)
    h["magic"], h["format"], h["payload_bytes"], h["samples_since_restart"] = state.MAGIC, state.FORMAT, 32, 5 * api.BLOCK_DEC
    h["version_hash"] = state.version_hash(api.load_library().tfrec_amd_version())
    h["types_mask"], h["rate_p"], h["rate_q"], h["tune_input_hz"] = 0x2F, 4, 3, -250000
    h["config"]["thresh"] = 700
    blob = h.tobytes() + bytes(32)
    p = state.parse_header(blob)
    assert p["samples_since_restart"] == 5 * api.BLOCK_DEC and p["config"]["thresh"] == 700 and p["tune_input_hz"] == -250000
    assert p["signature"][3:5] == (4, 3) and p["signature"][7] == 0x2F and len(p["signature"]) == len(state.SIGNATURE_FIELDS)
    assert state.parse_header(np.frombuffer(blob, dtype=np.uint8)) == p
    for bad in (blob[:100], b"XFST" + blob[4:], blob[:4] + b"\x02" + blob[5:], blob + b"\0"):
        with pytest.raises(ValueError):
            state.parse_header(bad)


def test_cli_usage_errors_exit_2_before_a_device_is_opened(tmp_path):
    cli = parity.build_cli()
    dump = tmp_path / "a.iq"
    dump.write_bytes(bytes([128]) * 4096)
    other = tmp_path / "b.iq"
    other.write_bytes(bytes([128]) * 4096)
    pfx = str(tmp_path / "keep")

    def run(*args):
        out = subprocess.run([cli] + [str(a) for a in args], capture_output=True, text=True, timeout=60)
        return out.returncode, out.stderr

    for flag in ("-k", "-K"):
        for extra in (["-n", "2"], ["-s", "100"], ["-A"], ["-P", "64"], ["-S", str(tmp_path / "cap")], ["-M"]):
            rc, err = run(flag, pfx, *extra, "-L", dump)
            assert rc == 2 and "-k and -K" in err, (flag, extra, err)
        assert run(flag, pfx, "-X", dump)[0] == 2
        assert run(flag, pfx, "-R", str(tmp_path / "cap"))[0] == 2
        rc, err = run(flag, pfx, "-L", dump, "-L", other, "-L", dump)
        assert rc == 2 and "more than one -L" in err
        assert run(flag, "", "-L", dump)[0] == 2
    rc, err = run("-K", pfx, "-L", dump)  # no keep.0.state
    assert rc == 2 and "keep.0.state" in err
    (tmp_path / "keep.0.state").write_bytes(b"")
    rc, err = run("-K", pfx, "-L", dump, "-L", other)  # ... and none for the second file
    assert rc == 2 and "keep.1.state" in err
    assert "-k prefix" in run("-h")[1] and "-K prefix" in run("-h")[1] and "not carried" in run("-h")[1]
    assert not [f for f in os.listdir(str(tmp_path)) if f.endswith(".rest")]  # nothing was written


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("state_plan") / "state_plan_driver")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(ROOT, "tests", "state_plan_driver.cpp")])

    def run(cmd, lines):
        out = subprocess.run([exe, cmd], input="".join(ln + "\n" for ln in lines), capture_output=True, text=True, timeout=120)
        assert out.returncode == 0 and not out.stderr, out.stderr  # (a sanitizer report goes to stderr and fails the run)
        assert "bad case" not in out.stdout
        return out.stdout.splitlines()

    return run


def unit_of(q):
    g = 64
    while q % g:
        g //= 2
    return q // g


def test_byte_plan_the_rest_the_pieces_and_the_unit(driver):
    """Every byte of (head, file) is in exactly one place: a whole piece, or the rest -- at Q = 1 (unit 1), Q = 3 (unit 3), Q = 1536
    (a whole-kHz rate: unit 24), with the formats' sample sizes and the 10x blocks."""
    rng = random.Random(5)
    cases = []
    for p, q, fmt, wide in ((1, 1, 0, 0), (4, 3, 0, 0), (2500, 1536, 0, 0), (25, 16, 2, 0), (4, 3, 3, 0), (1, 1, 0, 1), (1, 1, 3, 0)):
        unit = unit_of(q)
        piece = 655360 if wide else 65536 * p * unit // q * {0: 2, 1: 2, 2: 4, 3: 8}[fmt] // 2
        for head, file in [(0, 0), (0, piece), (0, piece - 1), (piece - 1, 1), (piece - 1, 0), (5, 3 * piece - 5), (piece + 7, 2), (1, 1)] + \
                [(rng.randrange(0, piece), rng.randrange(0, 6 * piece)) for _ in range(20)]:
            cases.append((head, file, p, q, fmt, wide, unit, piece))
    out = driver("bytes", ["%d %d %d %d %d %d" % c[:6] for c in cases])
    assert len(out) == len(cases)
    for c, ln in zip(cases, out):
        head, file, p, q, fmt, wide, unit, piece = c
        got = tuple(int(v) for v in ln.split())
        pieces = (head + file) // piece
        used_head = min(head, pieces * piece)
        want = (1 if wide else unit, piece, pieces * (1 if wide else unit), used_head, pieces * piece - used_head, head - used_head,
                file - (pieces * piece - used_head))
        assert got == want, (c, got)
        assert got[5] + got[6] == (head + file) % piece < piece and (got[5] == 0 or got[4] == 0)
    assert unit_of(3) == 3 and unit_of(1536) == 24


def test_batches_under_k_never_reach_past_a_files_end(driver):
    rng = random.Random(6)
    cases = [(16, [40]), (16, [16, 16]), (4, [9, 2, 5]), (6, [0, 7, 0, 3])] + \
            [(rng.randrange(1, 9), [rng.randrange(0, 30) for _ in range(rng.randrange(1, 6))]) for _ in range(30)]
    out = driver("batches", ["%d %s" % (bps, " ".join(str(b) for b in blocks)) for bps, blocks in cases])
    pos = 0
    for bps, blocks in cases:
        done = [0] * len(blocks)
        while out[pos] != "end":
            v = [int(x) for x in out[pos].split()]
            nb, files = v[0], v[1:]
            assert 1 <= nb <= bps and len(files) == len(blocks)
            for f in files:
                if f >= 0:
                    done[f] += nb
                    assert done[f] <= blocks[f], "a batch reaches past the end of file %d" % f
            pos += 1
        pos += 1
        assert done == blocks
    assert pos == len(out)
