"""Per-stream settings without a GPU: the C ABI declares and exports tfrec_amd_configure_streams and
tfrec_amd_get_stream_config, the binding has StreamConfig and Receiver.configure_streams / stream_config, and tfrec_gpu
knows -p (and refuses a bad spec before it opens a device)."""
import ctypes
import os
import re
import subprocess

import pytest

import parity
from tfrec_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cli():
    return parity.build_cli()


def test_header_declares_and_library_exports_the_stream_config_calls():
    hdr = open(os.path.join(ROOT, "include", "tfrec_amd.h")).read()
    assert re.search(r"int\s+tfrec_amd_configure_streams\s*\(\s*tfrec_amd_ctx\s*\*\s*\w+\s*,\s*const\s+int32_t\s*\*\s*\w+\s*,"
                     r"\s*const\s+tfrec_amd_stream_config\s*\*\s*\w+\s*,\s*int\s+\w+\s*\)", hdr)
    assert re.search(r"int\s+tfrec_amd_get_stream_config\s*\(\s*tfrec_amd_ctx\s*\*\s*\w+\s*,\s*int\s+\w+\s*,"
                     r"\s*tfrec_amd_stream_config\s*\*\s*\w+\s*\)", hdr)
    L = api.load_library()
    for name in ("tfrec_amd_configure_streams", "tfrec_amd_get_stream_config"):
        assert hasattr(L, name)
        assert name in api.EXPORTS


def test_stream_config_is_16_bytes():
    assert ctypes.sizeof(api.StreamConfig) == 16
    assert [f[0] for f in api.StreamConfig._fields_] == ["types_mask", "thresh", "filter_type", "reserved"]


def test_receiver_has_the_methods():
    assert callable(getattr(api.Receiver, "configure_streams", None))
    assert callable(getattr(api.Receiver, "stream_config", None))


def test_null_context_is_refused():
    L = api.load_library()
    cfg = api.StreamConfig(1, 0, 0, 0)
    idx = (ctypes.c_int32 * 1)(0)
    assert L.tfrec_amd_configure_streams(None, ctypes.cast(idx, ctypes.c_void_p), ctypes.byref(cfg), 1) == api.E_INVAL
    assert L.tfrec_amd_configure_streams(None, None, None, 0) == api.E_INVAL
    assert L.tfrec_amd_get_stream_config(None, 0, ctypes.byref(cfg)) == api.E_INVAL


@pytest.mark.parametrize("spec", ["T=40", "T=0", "T=10", "t=-1", "W=2", "x=1", "T=2f,T=1", "T=zz", "T=1,", "", "T",
                                  "t=5x"])
def test_tfrec_gpu_refuses_bad_specs(cli, tmp_path, spec):
    p = tmp_path / "x.iq"
    p.write_bytes(b"\x80" * 65536)
    # HIP_VISIBLE_DEVICES=-1: had it tried to open a device, it would have failed differently (exit status 2)
    out = subprocess.run([cli, "-p", spec, "-L", str(p)], capture_output=True, text=True, timeout=60,
                         env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    assert out.returncode == 1
    assert "-p" in out.stderr


def test_tfrec_gpu_refuses_p_with_x(cli, tmp_path):
    p = tmp_path / "t.txt"
    p.write_text("")
    out = subprocess.run([cli, "-p", "T=1", "-X", str(p)], capture_output=True, text=True, timeout=60,
                         env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    assert out.returncode == 1
    assert "-p" in out.stderr


def test_tfrec_gpu_usage_lists_p(cli):
    out = subprocess.run([cli, "-h"], capture_output=True, text=True, timeout=60)
    assert "-p" in out.stderr
    assert "T=<hex>" in out.stderr
