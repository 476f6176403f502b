"""Digital tuning without a GPU: the committed table, the phase increment and tfrec_amd/tune.py's mix against the definition
(DESIGN.md 6d), the definition itself against the C oracle on planted off-centre bursts, the exported C ABI, and tfrec_gpu's
-f / -c / -p f= checks, made before any device is opened."""
import os
import re
import subprocess

import numpy as np
import pytest

import parity
from oracle import oracle as O
from tfrec_amd import api, synth, tune

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def telegrams(x16, tune_hz):
    """Status-1 events of a fresh oracle fed the stream x16 (int16 at 1.536 MS/s) tuned by tune_hz."""
    o = O.Oracle(0x2F, 500, 0)
    o.process_s16(tune.mix_s16(x16, tune_hz))
    return [e for e in o.events_full() if e[7] == 1]


def test_table_header_is_the_formula():
    text = open(os.path.join(ROOT, "tfrec_amd", "csrc", "tune_table.h")).read()
    body = text.split("#define TFREC_TUNE_COS_TABLE", 1)[1]
    got = np.array([int(v) for v in re.findall(r"-?\d+", body)])
    k = np.arange(4096)
    want = np.round(32767.0 * np.cos(2.0 * np.pi * k / 4096)).astype(np.int64)
    assert np.array_equal(got, want)
    assert "#define TFREC_TUNE_BITS 12" in text
    c, s = tune.table()
    assert np.array_equal(c, want) and np.array_equal(s, want[(k - 1024) % 4096])
    assert c[0] == 32767 and s[1024] == 32767
    v = 32767.0 * np.cos(2.0 * np.pi * k / 4096)
    assert np.min(np.abs(v - np.floor(v) - 0.5)) > 1.4e-4  # no entry near a rounding tie
    assert np.max(np.abs(c) + np.abs(s)) <= 46340  # I*C + Q*S cannot overflow int32


def test_inc_examples():
    assert tune.inc(25000) == 69905067
    assert tune.inc(-25000) == 4225062229
    assert tune.inc(767999) == 2147480852
    assert tune.inc(0) == 0
    for bad in (768000, -768000, 10 ** 6):
        with pytest.raises(ValueError):
            tune.inc(bad)


def test_mix_identity_split_and_saturation():
    rng = np.random.default_rng(3)
    x = rng.integers(-32768, 32768, 2 * 5000).astype(np.int16)
    assert np.array_equal(tune.mix_s16(x, 0), x)
    for f in (25000, -200000, 767999, -767999, 12345):
        whole = tune.mix_s16(x, f)
        for a in (1, 777, 4999):
            parts = np.concatenate([tune.mix_s16(x[:2 * a], f, 0), tune.mix_s16(x[2 * a:], f, a)])
            assert np.array_equal(whole, parts), (f, a)
        assert not np.array_equal(whole, x)
    # a full-scale 10x input saturates: (-32768, -32768) rotated by 45 degrees is -46341 before sat16
    full = np.full(2 * 4096, -32768, dtype=np.int16)
    m = tune.mix_s16(full, 767999).astype(np.int32)
    assert m.min() == -32768 and m.max() == 32767
    # u8 input never does: |I'|, |Q'| <= 11585
    u = tune.s16_of_u8(np.array([0, 0, 255, 255, 0, 255] * 1000, dtype=np.uint8))
    assert np.abs(tune.mix_s16(u, 767999).astype(np.int32)).max() <= 11585


def test_mix_matches_the_definition_sample_by_sample():
    rng = np.random.default_rng(4)
    x = rng.integers(-32768, 32768, 2 * 300).astype(np.int16)
    c, s = tune.table()
    for f, n0 in ((25000, 0), (-25000, 10 ** 9), (-767999, 3)):
        inc = tune.inc(f)
        got = tune.mix_s16(x, f, n0)
        for n in range(300):
            k = ((n0 + n) * inc) % 2 ** 32 >> 20
            i, q = int(x[2 * n]), int(x[2 * n + 1])
            wi = (i * int(c[k]) + q * int(s[k]) + 2 ** 14) >> 15
            wq = (q * int(c[k]) - i * int(s[k]) + 2 ** 14) >> 15
            assert got[2 * n] == max(-32768, min(32767, wi)) and got[2 * n + 1] == max(-32768, min(32767, wq))


def test_int16_entry_equals_u8_entry():
    x = synth.gen_scene(3, 2, [dict(proto=1, start=30000, payload_seed=5)])
    a, b = O.Oracle(0x2F, 500, 0), O.Oracle(0x2F, 500, 0)
    a.process(x)
    b.process_s16(tune.s16_of_u8(x))
    assert a.events_full() == b.events_full() and len(a.events_full()) > 0


@pytest.mark.parametrize("proto,f0,n_blocks,seed", [(1, 200000, 2, 5), (0, -250000, 2, 5), (4, 150000, 6, 11),
                                                    (4, -400000, 6, 11)], ids=["tfa2+200k", "tfa1-250k", "whb+150k", "whb-400k"])
def test_offset_burst_decodes_only_when_tuned(proto, f0, n_blocks, seed):
    x16 = tune.s16_of_u8(synth.gen_scene(3, n_blocks, [dict(proto=proto, start=30000, payload_seed=seed, f0_hz=f0)]))
    got = telegrams(x16, f0)
    assert len(got) == 1 and got[0][0] == {0: 0, 1: 1, 4: 4}[proto]
    assert telegrams(x16, 0) == []
    assert telegrams(x16, -f0) == []


def test_offset_burst_on_10x_input():
    x = synth.gen_scene(3, 2, [dict(proto=1, start=300000, payload_seed=5, f0_hz=-500000)], rate_mult=10)
    x16 = O.decim10(x)
    assert len(telegrams(x16, -500000)) == 1
    assert telegrams(x16, 0) == [] and telegrams(x16, 500000) == []


def test_tfa2_telegram_bytes():
    x16 = tune.s16_of_u8(synth.gen_scene(3, 2, [dict(proto=1, start=30000, payload_seed=5, f0_hz=200000)]))
    got = telegrams(x16, 200000)
    assert len(got) == 1 and got[0][5][:2] == b"\x2d\xd4"


def test_header_declares_and_library_exports_the_tune_calls():
    hdr = open(os.path.join(ROOT, "include", "tfrec_amd.h")).read()
    assert re.search(r"int\s+tfrec_amd_tune_streams\s*\(\s*tfrec_amd_ctx\s*\*\s*\w+\s*,\s*const\s+int32_t\s*\*\s*\w+\s*,"
                     r"\s*const\s+int32_t\s*\*\s*\w+\s*,\s*int\s+\w+\s*\)", hdr)
    assert re.search(r"int\s+tfrec_amd_get_stream_tune\s*\(\s*tfrec_amd_ctx\s*\*\s*\w+\s*,\s*int\s+\w+\s*,"
                     r"\s*int32_t\s*\*\s*\w+\s*\)", hdr)
    L = api.load_library()
    for name in ("tfrec_amd_tune_streams", "tfrec_amd_get_stream_tune"):
        assert hasattr(L, name) and name in api.EXPORTS
    assert callable(getattr(api.Receiver, "tune_streams", None)) and callable(getattr(api.Receiver, "stream_tune", None))
    assert L.tfrec_amd_tune_streams(None, None, None, 0) == api.E_INVAL
    assert L.tfrec_amd_get_stream_tune(None, 0, None) == api.E_INVAL


@pytest.fixture(scope="module")
def cli():
    return parity.build_cli()


@pytest.mark.parametrize("args", [["-f", "869100"], ["-f", "867400"], ["-c", "868000", "-f", "868768"], ["-f", "x"],
                                  ["-f", "-5"], ["-c", "0"], ["-p", "f=869018"], ["-p", "f=8682x"], ["-p", "f=868250,f=1"],
                                  ["-p", "f="]])
def test_tfrec_gpu_refuses_bad_frequencies(cli, tmp_path, args):
    p = tmp_path / "x.iq"
    p.write_bytes(b"\x80" * 65536)
    # HIP_VISIBLE_DEVICES=-1: had it tried to open a device, it would have failed differently (exit status 2)
    out = subprocess.run([cli] + args + ["-L", str(p)], capture_output=True, text=True, timeout=60,
                         env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    assert out.returncode == 1, out.stderr
    assert "tfrec_gpu:" in out.stderr


def test_tfrec_gpu_usage_lists_f_and_c(cli):
    out = subprocess.run([cli, "-h"], capture_output=True, text=True, timeout=60)
    assert "-f kHz" in out.stderr and "-c kHz" in out.stderr and "f=<kHz>" in out.stderr
