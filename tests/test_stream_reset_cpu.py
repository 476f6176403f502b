"""Per-stream reset without a GPU: the C ABI exports and declares tfrec_amd_reset_streams, the binding has
Receiver.reset_streams, and tfrec_gpu knows -n (and refuses a count below one before it opens a device)."""
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


def test_library_exports_and_header_declares_reset_streams():
    L = api.load_library()
    assert hasattr(L, "tfrec_amd_reset_streams")
    hdr = open(os.path.join(ROOT, "include", "tfrec_amd.h")).read()
    assert re.search(r"int\s+tfrec_amd_reset_streams\s*\(\s*tfrec_amd_ctx\s*\*\s*\w+\s*,\s*const\s+int32_t\s*\*\s*\w+\s*,\s*int\s+\w+\s*\)",
                     hdr)
    assert "tfrec_amd_reset_streams" in api.EXPORTS


def test_receiver_has_reset_streams():
    assert callable(getattr(api.Receiver, "reset_streams", None))


@pytest.mark.parametrize("n", ["0", "-1"])
def test_tfrec_gpu_refuses_fewer_than_one_stream(cli, tmp_path, n):
    p = tmp_path / "x.iq"
    p.write_bytes(b"\x80" * 65536)
    # HIP_VISIBLE_DEVICES=-1: had it tried to open a device, it would have failed differently (exit status 2)
    out = subprocess.run([cli, "-n", n, "-L", str(p)], capture_output=True, text=True, timeout=60,
                         env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    assert out.returncode == 1
    assert "-n" in out.stderr


def test_tfrec_gpu_usage_lists_n(cli):
    out = subprocess.run([cli, "-h"], capture_output=True, text=True, timeout=60)
    assert "-n" in out.stderr
