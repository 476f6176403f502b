"""Digital tuning (tfrec_amd_tune_streams / Receiver.tune_streams, tfrec_gpu -f / -c / -p f=) on the GPU, against the oracle.

A tuned stream's events equal those of a fresh oracle.Oracle fed, through its int16 entry, tune.mix_s16 of the stream's input
(x = (u8 - 128) << 6, or the 10:1 stage's output) from its start or restart on -- in every field, seq included; its decimated
samples equal the oracle's dec() and its threshold the oracle's thresh().  Untuned streams beside it equal the u8 oracle."""
import ctypes

import numpy as np
import pytest

import parity
import segments
from oracle import oracle as O
from tfrec_amd import api, synth, tune

pytestmark = pytest.mark.gpu

SIZES = (3, 2, 3)  # blocks of the three submits (ragged, the FIFO four deep)
# every tune of the definition's corners: 0, +-25 kHz (odd inc), +-200 kHz, the +-767999 limit, and odd values
TUNES = [0, 25000, -25000, 200000, -200000, 767999, -767999, 12345, -250000, 150000, 0, -400000, 31, -1, 500000, 0,
         -500000, 99999, 25000, -200000, 0, 700001, -654321, 200000]
CFGS = [None, (0x2F, 500, 1), (0x03, 0, 0), None, (0x21, 300, 0), (0x2F, 0, 1), None, (0x01, 500, 0), (0x2F, 900, 0), None,
        (0x02, 0, 1), (0x20, 500, 0), None, (0x2F, 300, 0), (0x06, 0, 0), (0x2F, 500, 1), None, (0x0C, 500, 0), (0x2F, 0, 0),
        None, (0x28, 500, 1), (0x2F, 500, 0), None, (0x01, 0, 1)]
BURST_SLOTS = (0, 1, 2, 3, 4)


def make_input(seed, tunes, n_blocks, rate_mult=1):
    """Per stream: three bursts at the stream's own tune offset (one at the centre for an untuned stream), plus one off-centre
    burst that only an untuned receiver must not see."""
    rows = []
    n = n_blocks * api.BLOCK_BYTES // 2 * rate_mult
    for s, f in enumerate(tunes):
        bursts = []
        for j in range(3):
            proto = BURST_SLOTS[(s + j) % 5]
            start = (20000 + j * (n - 40000) // 3) // rate_mult * rate_mult
            bursts.append(dict(proto=proto, start=start, payload_seed=7 + s + 11 * j, f0_hz=f, amp=50 + 10 * j))
        bursts.append(dict(proto=1, start=(n * 2) // 3 + 5000 * rate_mult, payload_seed=3 + s, f0_hz=300000 if f <= 0 else -300000))
        rows.append(synth.gen_scene(seed * 100 + s, n_blocks, bursts, rate_mult=rate_mult))
    return np.stack(rows)


def conf_op(idx, dflt):
    idx = [s for s in idx if CFGS[s] is not None]
    return ("conf", idx, [CFGS[s] for s in idx])


@pytest.mark.parametrize("in10x", [False, True], ids=["default", "input_10x"])
def test_tuned_context_parity(in10x):
    rate = 10 if in10x else 1
    sizes = (2, 1, 2) if in10x else SIZES
    n = len(TUNES)
    iq = make_input(21, TUNES, sum(sizes), rate_mult=rate)
    parts = parity.cut(iq, sizes, api.BLOCK_BYTES * rate)
    dflt = (0x2F, 500, 0)
    ops = {0: [conf_op(range(n), dflt), ("tune", list(range(n)), TUNES)],
           1: [("tune", [3, 8, 13], [-25000, 0, 767999]), ("reset", [5])]}  # a mid-run tune (and one back to 0) beside a reset
    with api.Receiver(n, dflt[0], dflt[1], dflt[2], max_blocks=max(sizes), all_flushes=True, input_10x=in10x) as r:
        total, segs = segments.run_segments(r, parts, ops, dflt, in10x=in10x)
    assert total > 5 * n
    # the planted bursts at the tune offsets decode: a telegram in most tuned segments
    tuned = [g for s in range(n) for g in segs[s] if g.tune != 0]
    assert sum(1 for g in tuned if any(e[7] == 1 for e in g.orc.events_full())) >= len(tuned) // 2


@pytest.mark.parametrize("mode", ["bits", "default_mode", "serial_chains"])
def test_tuned_modes(mode, monkeypatch):
    n = 12
    tunes = TUNES[:n]
    iq = make_input(22, tunes, sum(SIZES))
    parts = parity.cut(iq, SIZES)
    dflt = (0x2F, 500, 0)
    ops = {0: [conf_op(range(n), dflt), ("tune", list(range(n)), tunes)], 2: [("tune", [1, 2], [-200000, 150000])]}
    kw, _, flags = parity.mode_kwargs(mode, monkeypatch)
    with api.Receiver(n, dflt[0], dflt[1], dflt[2], max_blocks=max(SIZES), **kw) as r:
        total, _ = segments.run_segments(r, parts, ops, dflt, bits=flags["bits"], default_mode=flags["default_mode"])
    assert total > n


def test_restart_semantics():
    """Stream 0: tuned before the first submit.  1: tuned mid-run.  2: a tune, a configure and a reset before one submit (one
    restart, latest values).  3: tuned, then reset: the tune stays.  4: tuned, then configured: the tune stays.  5: tuned
    twice in one call (the last wins).  6-7: untuned beside them."""
    n = 8
    tunes = [200000, -250000, 150000, -400000, 25000, -200000, 0, 0]
    iq = make_input(23, tunes, 8)
    parts = parity.cut(iq, (2, 2, 2, 2))
    dflt = (0x2F, 500, 0)
    ops = {0: [("tune", [0, 5, 5], [200000, 100000, -200000])],
           1: [("tune", [1, 3, 4], [-250000, -400000, 25000])],
           2: [("tune", [2], [150000]), ("conf", [2], [(0x2F, 0, 1)]), ("reset", [2, 3]), ("conf", [4], [(0x03, 500, 1)])],
           3: [("reset", [0]), ("conf", [2], [(0x2F, 300, 0)])]}
    with api.Receiver(n, dflt[0], dflt[1], dflt[2], max_blocks=2, all_flushes=True) as r:
        total, segs = segments.run_segments(r, parts, ops, dflt)
        assert [r.stream_tune(s) for s in range(n)] == [200000, -250000, 150000, -400000, 25000, -200000, 0, 0]
    assert [len(segs[s]) for s in range(n)] == [2, 2, 3, 3, 3, 1, 1, 1]
    assert total > 4 * n


def test_two_streams_one_recording():
    """The same bytes in two streams, two planted bursts at different offsets: each stream decodes its own and not the
    other's."""
    x = synth.gen_scene(31, 4, [dict(proto=1, start=30000, payload_seed=5, f0_hz=200000),
                                dict(proto=0, start=100000, payload_seed=5, f0_hz=-250000)])
    iq = np.stack([x, x])
    with api.Receiver(2, 0x2F, 500, 0, max_blocks=4, all_flushes=True) as r:
        r.tune_streams([0, 1], [200000, -250000])
        r.submit(iq)
        ev = r.drain()
    for s, (f, own, other) in enumerate(((200000, 1, 0), (-250000, 0, 1))):
        o = O.Oracle(0x2F, 500, 0)
        o.process_s16(tune.mix_s16(tune.s16_of_u8(x), f))
        parity.assert_segment(ev, s, o, "stream %d" % s)
        ok = ev[(ev["stream"] == s) & (ev["status"] == 1)]
        assert ok["slot"].tolist() == [own], (s, ok["slot"].tolist())
        assert other not in ok["slot"].tolist()


def test_argument_errors_change_nothing():
    n_streams = 4
    iq = make_input(24, [0, 200000, 0, -250000], 6)
    parts = parity.cut(iq, (3, 3))

    def run(bad):
        with api.Receiver(n_streams, 0x2F, 500, 0, max_blocks=3, all_flushes=True) as r:
            r.tune_streams([1, 3], [200000, -250000])
            r.submit(np.ascontiguousarray(parts[0]))
            if bad:
                L = r.L

                def call(streams, hz, n=None):
                    idx = np.array(streams, dtype=np.int32)
                    t = np.array(hz, dtype=np.int32)
                    return L.tfrec_amd_tune_streams(r.h, idx.ctypes.data if len(idx) else None,
                                                    t.ctypes.data if len(t) else None, len(streams) if n is None else n)

                for streams, hz in (([1, 4], [0, 0]), ([-1], [0]), ([0, 1], [0, 768000]), ([0, 1], [0, -768000]),
                                    ([2], [2 ** 31 - 1]), ([2], [-2 ** 31])):
                    assert call(streams, hz) == api.E_INVAL, (streams, hz)
                assert call([1], [0], n=-1) == api.E_INVAL
                assert L.tfrec_amd_tune_streams(r.h, None, None, 1) == api.E_INVAL
                assert L.tfrec_amd_tune_streams(r.h, np.array([1], dtype=np.int32).ctypes.data, None, 1) == api.E_INVAL
                assert L.tfrec_amd_tune_streams(r.h, None, None, 0) == api.E_OK
                v = ctypes.c_int32(7)
                assert L.tfrec_amd_get_stream_tune(r.h, 4, ctypes.byref(v)) == api.E_INVAL and v.value == 7
                for wrong in (([4], 0), ([0], 768000), ([0], 2 ** 32)):
                    with pytest.raises(api.TfrecAmdError):
                        r.tune_streams(*wrong)
                r.tune_streams([], [])
            tunes = [r.stream_tune(s) for s in range(n_streams)]
            r.submit(np.ascontiguousarray(parts[1]))
            return tunes, np.concatenate([r.drain(), r.drain()])

    t0, none = run(False)
    t1, ev = run(True)
    assert t0 == t1 == [0, 200000, 0, -250000]
    assert len(none) > 0 and none.tobytes() == ev.tobytes()
    for s in range(n_streams):  # one segment each: seq carries on across the refused calls
        o = O.Oracle(0x2F, 500, 0)
        o.process_s16(tune.mix_s16(tune.s16_of_u8(iq[s]), t0[s]))
        parity.assert_segment(ev, s, o, "stream %d" % s)


# ---- tfrec_gpu -f / -c / -p f=
@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    parity.build_cli()
    d = tmp_path_factory.mktemp("tdump")
    x = synth.gen_scene(41, 6, [dict(proto=1, start=30000, payload_seed=5, f0_hz=-200000)])
    p = d / "d.iq"
    p.write_bytes(x.tobytes())
    return d, str(p), x


def test_tfrec_gpu_receive_frequency(dump):
    d, path, x = dump
    o = O.Oracle(0x07, 0, 0)  # tfrec_gpu's defaults: -T 7, -t 0 (auto)
    o.process_s16(tune.mix_s16(tune.s16_of_u8(x), -200000))
    want = parity.telegram_lines(o.text())
    assert len(want) == 1 and want[0].startswith("TFA2 ")
    tuned = parity.cli_stdout(["-f", "868050", "-L", path])
    assert parity.telegram_lines(tuned) == want
    assert parity.cli_stdout(["-c", "868300", "-f", "868100", "-L", path]) == tuned
    assert parity.telegram_lines(parity.cli_stdout(["-L", path])) == []
    # the same file twice: tuned for the first stream only
    _, recs = parity.cli(["-p", "f=868050", "-L", path, "-p", "f=868250", "-L", path], d / "two.out")
    assert [r[0] for r in recs] == ["0"]
    _, alone = parity.cli(["-f", "868050", "-L", path], d / "one.out")
    assert [r[1:] for r in recs] == [r[1:] for r in alone]
    # ... and through one stream as a queue (-n 1): the second file runs untuned after a restart
    _, q = parity.cli(["-n", "1", "-p", "f=868250", "-L", path, "-p", "f=868050", "-L", path], d / "q.out")
    assert [r[0] for r in q] == ["1"] and [r[1:] for r in q] == [r[1:] for r in alone]
