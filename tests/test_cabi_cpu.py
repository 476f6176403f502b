"""CPU tests of the C-ABI shared library and the host-side logic: the library loads, exports every symbol
include/tfrec_amd.h declares, validates arguments, and fails LOUDLY without a GPU (no CPU fallback)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tfrec_amd import api, shard, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _no_gpu():
    import torch
    return not torch.cuda.is_available()


def test_library_exports_every_declared_symbol():
    hdr = open(os.path.join(ROOT, "include", "tfrec_amd.h")).read()
    declared = sorted(set(re.findall(r"\b(tfrec_amd_[a-z0-9_]+)\s*\(", hdr)))
    assert set(declared) == set(api.EXPORTS)
    L = api.load_library()
    for name in declared:
        assert getattr(L, name) is not None
    assert L.tfrec_amd_version().startswith(b"tfrec_amd")
    assert C.sizeof(api.Config) == 32 and api.EVENT_DTYPE.itemsize == 96


def test_product_library_has_no_knobs_and_the_experiments_build_has_only_the_kept_ones_and_the_same_abi():
    """csrc/knobs.h: the library bench.py and the adapter load is built without TFREC_AMD_EXPERIMENTS -- no getenv import, no knob
    name, no test hook in the binary; libtfrec_amd_exp.so (same sources) has them and the same C ABI, and no retired knob."""
    import subprocess
    from tfrec_amd import _build

    api.load_library()
    Lx = api.load_library(experiments=True)
    for name in api.EXPORTS:
        assert getattr(Lx, name) is not None
    prod = open(_build.LIB_SO, "rb").read()
    expl = open(_build.LIB_EXP_SO, "rb").read()
    for knob in (b"TFREC_AMD_SKIP", b"TFREC_AMD_WHB_FORCE_FAIL", b"TFREC_AMD_WHB_TEST_PERTURB", b"TFREC_AMD_LANES_", b"_DIV",
                 b"TFREC_AMD_LDS_PAD", b"TFREC_AMD_DEEP", b"TFREC_AMD_"):
        assert knob not in prod, knob
    assert b"TFREC_AMD_DEEP" in expl and b"TFREC_AMD_WHB_FORCE_FAIL" in expl
    # the A/B variants of rounds 1-6 are retired (profiles/NOTES.md, "retired knobs"): not even the experiments build reads them
    for knob in (b"TFREC_AMD_SKIP", b"TFREC_AMD_LANES_", b"_DIV", b"TFREC_AMD_LDS_PAD", b"TFREC_AMD_FE_LDS_PAD", b"TFREC_AMD_WHB_LDS",
                 b"TFREC_AMD_COOP_", b"TFREC_AMD_HEAD_CHUNKS", b"TFREC_AMD_FMDEV_", b"TFREC_AMD_WHB_EXACT",
                 b"TFREC_AMD_WHB_CHECK_ROWS", b"TFREC_AMD_T1_EARLY", b"TFREC_AMD_SCAN_KW", b"TFREC_AMD_SPEC_OWN", b"TFREC_AMD_COPY_OWN",
                 b"TFREC_AMD_PRIO", b"TFREC_AMD_FS_CU", b"TFREC_AMD_COPY_KERNEL", b"TFREC_AMD_COPY_BLOCKS", b"TFREC_AMD_FE_PERSIST"):
        assert knob not in expl, knob
    # ... and it does not import getenv at all
    syms = subprocess.run(["nm", "-D", "--undefined-only", _build.LIB_SO], capture_output=True, text=True, check=True).stdout
    assert "getenv" not in syms
    assert "getenv" in subprocess.run(["nm", "-D", "--undefined-only", _build.LIB_EXP_SO], capture_output=True, text=True,
                                      check=True).stdout


def test_build_staleness_is_decided_by_content(tmp_path):
    """tfrec_amd/_build.py: an object is current iff its stamp equals the SHA-256 of its sources, headers and flags -- time
    stamps play no part (a snapshot copy refreshes them), and an edited header makes every object stale."""
    from tfrec_amd import _build

    src = tmp_path / "a.hip"
    hdr = tmp_path / "a.h"
    obj = tmp_path / "a.o"
    src.write_text("int f();")
    hdr.write_text("// 1")
    obj.write_text("object")
    d1 = _build._digest([str(src), str(hdr)], "-O3")
    assert not _build._current(str(obj), d1)  # no stamp yet
    _build._stamp(str(obj), d1)
    assert _build._current(str(obj), d1)
    os.utime(str(src), (10**9 * 2, 10**9 * 2))  # a newer time stamp alone changes nothing
    assert _build._current(str(obj), _build._digest([str(src), str(hdr)], "-O3"))
    hdr.write_text("// 2")
    assert not _build._current(str(obj), _build._digest([str(src), str(hdr)], "-O3"))
    assert not _build._current(str(obj), _build._digest([str(src), str(hdr)], "-O2"))  # ... nor do other flags
    _build.build_all()
    acts = _build.last_actions()
    assert any("libtfrec_amd.so" in a for a in acts) and any("libtfrec_amd_exp.so" in a for a in acts)


def test_argument_validation_precedes_device_use():
    L = api.load_library()
    h = C.c_void_p()
    bad = api.Config(0, 0x2F, 500, 0, 0, 8, 1024, 0)  # n_streams = 0
    assert L.tfrec_amd_create(C.byref(bad), C.byref(h)) == api.E_INVAL
    neg = api.Config(4, 0x2F, -1, 0, 0, 8, 1024, 0)  # negative threshold (0 = the reference's auto mode is valid)
    assert L.tfrec_amd_create(C.byref(neg), C.byref(h)) == api.E_INVAL
    assert L.tfrec_amd_create(None, C.byref(h)) == api.E_INVAL
    assert L.tfrec_amd_destroy(None) == api.E_OK
    assert L.tfrec_amd_strerror(api.E_OVERFLOW) == b"event buffer overflow"


@pytest.mark.skipif(not _no_gpu(), reason="only meaningful on a box without a GPU")
def test_no_gpu_fails_loudly_no_cpu_fallback():
    with pytest.raises(api.TfrecAmdError) as e:
        api.Receiver(4)
    assert e.value.code == api.E_HIP


def test_host_rssi_db_matches_reference_expressions():
    from oracle import oracle as O
    iq = synth.gen_stream(7, 0, 48)
    o = O.Oracle(0x2F, 500)
    o.process(iq)
    evs = o.events_raw()
    assert len(evs) > 50
    for (slot, _end, _bc, rssi_db, _off, _rd), raw in evs:
        assert api.rssi_db(slot, raw) == rssi_db
    # (int)(10*log10(0)) and negative/NaN cases behave like x86 cvttsd2si
    assert api.rssi_db(0, 0) == -2147483648
    assert api.rssi_db(1, -5) == -2147483648
    assert api.rssi_db(4, 0) == 0


def test_shard_ranges_cover_every_stream_once():
    for n in (1, 7, 8, 1024, 8192, 8191):
        for w in (1, 2, 3, 8):
            seen = []
            for r in range(w):
                a, b = shard.shard_range(r, w, n)
                seen.extend(range(a, b))
            assert seen == list(range(n))


def test_generator_is_deterministic_and_decodable():
    a = synth.gen_stream(99, 5, 8)
    b, truth = synth.gen_stream(99, 5, 8, with_truth=True)
    assert np.array_equal(a, b) and len(truth) >= 2
    c = synth.gen_batch(99, 4, 3, 8)
    assert np.array_equal(c[1], a)
    assert all(t["frame"][:2] in (b"\x2d\xd4", b"\x4b\x2d") for t in truth)
