"""Shared inputs and the wideband tune (tfrec_amd_map_streams, tfrec_amd_tune_streams_wide, tfrec_gpu -x) without a
GPU: the numpy restatement of the 10:1 stage and of the mixer at the input rate (tfrec_amd/tune.py) against the oracle, the
definition receiving planted bursts out of ONE 15.36 MS/s scene, the C ABI's exports and the argument errors that need no
device, and tfrec_gpu's usage errors."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import parity
from input_rows import EMPTY_HZ, WIDE_BURSTS, wide_scene
from oracle import oracle as O
from tfrec_amd import api, tune

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def receive(x16, f):
    o = O.Oracle(0x2F, 500, 0)
    o.process_s16(tune.decim10_s16(tune.mix10_s16(x16, f)))
    return o.events_full()


def test_decim10_s16_equals_the_oracle():
    iq = wide_scene()
    assert np.array_equal(tune.decim10_s16(tune.s16_of_u8(iq)), O.decim10(iq))


def test_decim10_s16_continues_with_history():
    x = tune.s16_of_u8(wide_scene(n_blocks=1))
    cut = 2 * 10 * 12345
    whole = tune.decim10_s16(x)
    assert np.array_equal(np.concatenate([tune.decim10_s16(x[:cut]), tune.decim10_s16(x[cut:], hist=x[cut - 100:cut])]), whole)


def test_inc10_corners():
    assert tune.inc10(0) == 0
    assert tune.inc10(1) == 280 and tune.inc10(-1) == 2 ** 32 - 280  # floor(2^33 / 30720000 + 1/2) = 280, and its negative
    for f in (1, -1, 7679999, -7679999, 3300000, 7):
        want = ((f << 33) + 15360000) // 30720000 % 2 ** 32  # the definition, in Python's exact integers and floor division
        assert tune.inc10(f) == want
        assert tune.inc10(-f) == (2 ** 32 - tune.inc10(f)) % 2 ** 32 or (f << 33) % 15360000 == 0
    assert tune.inc10(7679999) == 2 ** 31 - 280 and tune.inc10(-7679999) == 2 ** 31 + 280
    assert tune.inc10(7) % 2 == 1  # an odd increment: the phase runs through all 2^32 values
    assert tune.inc10(1000) == tune.inc(100)  # the same frequency at a tenth of the rate
    for f in (7680000, -7680000, 10 ** 9):
        with pytest.raises(ValueError):
            tune.inc10(f)


def test_mix10_zero_is_a_copy_and_phase_continues():
    x = tune.s16_of_u8(wide_scene(n_blocks=1))[:40000]
    y = tune.mix10_s16(x, 0)
    assert np.array_equal(y, x) and y is not x
    whole = tune.mix10_s16(x, 3300000)
    assert np.array_equal(np.concatenate([tune.mix10_s16(x[:10002], 3300000), tune.mix10_s16(x[10002:], 3300000, 5001)]), whole)
    assert not np.array_equal(whole, x)


def test_the_definition_receives_every_planted_burst_and_nothing_else():
    x16 = tune.s16_of_u8(wide_scene())
    for f, slot in WIDE_BURSTS:
        ev = receive(x16, f)
        ok = [e for e in ev if e[7] == 1]
        assert [e[0] for e in ok] == [slot], (f, [(e[0], e[2], e[7]) for e in ev])
    assert [e for e in receive(x16, EMPTY_HZ) if e[7] == 1] == []
    assert [e for e in receive(x16, 0) if e[7] == 1] == []  # an untuned receiver sees the centre: nothing planted there


def test_header_declares_and_library_exports_the_calls():
    hdr = open(os.path.join(ROOT, "include", "tfrec_amd.h")).read()
    two = r"\s*\(\s*tfrec_amd_ctx\s*\*\s*\w+\s*,\s*const\s+int32_t\s*\*\s*\w+\s*,\s*const\s+int32_t\s*\*\s*\w+\s*,\s*int\s+\w+\s*\)"
    get = r"\s*\(\s*tfrec_amd_ctx\s*\*\s*\w+\s*,\s*int\s+\w+\s*,\s*int32_t\s*\*\s*\w+\s*\)"
    assert re.search(r"int\s+tfrec_amd_map_streams" + two, hdr)
    assert re.search(r"int\s+tfrec_amd_tune_streams_wide" + two, hdr)
    assert re.search(r"int\s+tfrec_amd_get_stream_input" + get, hdr)
    assert re.search(r"int\s+tfrec_amd_get_stream_tune_wide" + get, hdr)
    L = api.load_library()
    for name in ("tfrec_amd_map_streams", "tfrec_amd_get_stream_input", "tfrec_amd_tune_streams_wide",
                 "tfrec_amd_get_stream_tune_wide"):
        assert hasattr(L, name) and name in api.EXPORTS
    for name in ("map_streams", "stream_input", "tune_streams_wide", "stream_tune_wide"):
        assert callable(getattr(api.Receiver, name, None))


def test_null_arguments_are_refused():
    L = api.load_library()
    idx = (ctypes.c_int32 * 1)(0)
    v = ctypes.c_int32(0)
    for fn in (L.tfrec_amd_map_streams, L.tfrec_amd_tune_streams_wide):
        assert fn(None, ctypes.cast(idx, ctypes.c_void_p), ctypes.cast(idx, ctypes.c_void_p), 1) == api.E_INVAL
        assert fn(None, None, None, 0) == api.E_INVAL
    for fn in (L.tfrec_amd_get_stream_input, L.tfrec_amd_get_stream_tune_wide):
        assert fn(None, 0, ctypes.byref(v)) == api.E_INVAL
        assert fn(None, 0, None) == api.E_INVAL


@pytest.fixture(scope="module")
def cli():
    return parity.build_cli()


@pytest.mark.parametrize("args", [["-f", "869100"], ["-p", "f=869018"], ["-x", "-f", "875930"], ["-x", "-p", "f=860570"]],
                         ids=["f_beyond_767_without_x", "p_f_beyond_767_without_x", "x_f_beyond_7679", "x_p_f_beyond_7679"])
def test_tfrec_gpu_refuses_bad_wide_frequencies(cli, tmp_path, args):
    p = tmp_path / "x.iq"
    p.write_bytes(b"\x80" * 655360)
    # HIP_VISIBLE_DEVICES=-1: had it tried to open a device, it would have failed differently (exit status 2)
    out = subprocess.run([cli] + args + ["-L", str(p)], capture_output=True, text=True, timeout=60,
                         env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    assert out.returncode == 1, out.stderr
    assert "tfrec_gpu:" in out.stderr


def test_tfrec_gpu_usage_lists_x(cli):
    out = subprocess.run([cli, "-h"], capture_output=True, text=True, timeout=60)
    assert "-x" in out.stderr and "15.36" in out.stderr and "7679" in out.stderr
