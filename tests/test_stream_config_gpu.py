"""Per-stream settings (tfrec_amd_configure_streams / Receiver.configure_streams) on the GPU, event by event against the
oracle.

A configured stream restarts at the next submit exactly as after a reset, but as a fresh receiver with its own -T, -t and
-W: its events equal those of oracle.Oracle(types_mask, thresh, wide) fed the input after the cut, while the streams
beside it, with other settings, carry on with theirs.  Compared in every field: slot, end_sample, byte_cnt, rssi, offset,
rdata, rssi_raw, status and seq; read_thresh against Oracle.thresh() after every submit."""
import numpy as np
import pytest

import parity
import segments
from oracle import oracle as O
from tfrec_amd import api, synth

pytestmark = pytest.mark.gpu

SIZES = (3, 2, 3)  # blocks of the three submits


def pulse_stream(seed, n_blocks, period=8000, rate_mult=1):
    """Synthetic bursts plus a short full-scale pulse every `period` bytes: about one trigger per 1000 decimated samples, so
    that how much of a block lies inside some demodulator's window -- what the auto threshold counts -- depends on the
    longest window of the stream's own demodulators (400 samples for TFA_1 alone, 694 with TX22)."""
    x = synth.gen_stream(seed, 0, n_blocks, rate_mult=rate_mult).copy()
    period *= rate_mult
    for p in range(1000 * rate_mult, len(x) - 32 * rate_mult, period):
        x[p:p + 32 * rate_mult] = 255
    return x


def make_input(seed, n_streams, n_blocks, rate_mult=1):
    rows = []
    for s in range(n_streams):  # every third stream with the pulse train, the others plain synthetic bursts
        if s % 3 == 2:
            rows.append(pulse_stream(seed * 100 + s, n_blocks, rate_mult=rate_mult))
        else:
            rows.append(synth.gen_stream(seed, s, n_blocks, rate_mult=rate_mult))
    return np.stack(rows)


# A mix for a 0x2f context: each slot alone, pairs and all five; auto and fixed thresholds; both filters; None = the defaults
MIX = [(0x04, 300, 1), (0x02, 500, 0), (0x01, 0, 0), (0x08, 900, 0), (0x20, 0, 1), (0x21, 500, 0), (0x06, 0, 0),
       (0x2F, 300, 1), (0x01, 0, 1), (0x2F, 0, 0), None, (0x20, 500, 0), (0x03, 900, 1), (0x0C, 0, 0), (0x2F, 500, 1),
       None, (0x28, 300, 0), (0x01, 500, 0), (0x2F, 900, 0), (0x21, 0, 1), None, (0x02, 0, 1), (0x2E, 500, 0), (0x01, 300, 0)]


def test_inputs_discriminate():
    """On the oracle alone: the pulse train ends a TFA_1-only auto stream at another threshold than an all-types one (a
    context-wide Wmax would be caught), and the two filters give different events on the test input."""
    iq = make_input(11, 3, sum(SIZES))
    th = {}
    for m in (0x01, 0x2F):
        o = O.Oracle(m, 0, 0)
        o.process(iq[2])
        th[m] = o.thresh()
    assert th[0x01] != th[0x2F]
    for s in range(2):
        ev = []
        for w in (0, 1):
            o = O.Oracle(0x2F, 500, w)
            o.process(iq[s])
            ev.append(sorted(o.events_full()))
        assert ev[0] != ev[1]


@pytest.mark.parametrize("dflt", [(0x2F, 500, 0), (0x2F, 0, 1)], ids=["fixed-narrow", "auto-wide"])
def test_mixed_context(dflt):
    iq = make_input(11, len(MIX), sum(SIZES))
    parts = parity.cut(iq, SIZES)
    table = [c for c in MIX]
    if dflt[1] == 0:  # the auto context: some streams fixed, the rest left at the defaults
        table = [c if c is None or c[1] else None for c in MIX]
    idx = [s for s, c in enumerate(table) if c is not None]
    ops = {0: [("conf", idx, [table[s] for s in idx])]}
    with api.Receiver(len(MIX), dflt[0], dflt[1], dflt[2], max_blocks=max(SIZES), all_flushes=True) as r:
        n, _ = segments.run_segments(r, parts, ops, dflt)
    assert n > 10 * len(MIX)


MODE_N = 12


@pytest.mark.parametrize("mode", ["serial_chains", "bits", "input_10x", "all_flushes"])
def test_modes(mode):
    rate = 10 if mode == "input_10x" else 1
    sizes = (2, 1, 2) if rate == 10 else SIZES
    iq = make_input(12, MODE_N, sum(sizes), rate_mult=rate)
    parts = parity.cut(iq, sizes, api.BLOCK_BYTES * rate)
    # (every mode with all flushes: the oracle reports every decoder::flush, and seq counts them all)
    kw = dict(max_blocks=max(sizes), all_flushes=True, serial_chains=(mode == "serial_chains"),
              input_10x=(mode == "input_10x"), bits=(mode == "bits"), max_events=1 << 17)
    table = MIX[:MODE_N]
    idx = [s for s, c in enumerate(table) if c is not None]
    # configured before the first submit, and some of them again after it
    ops = {0: [("conf", idx, [table[s] for s in idx])],
           2: [("conf", [1, 5, 8], [(0x2F, 0, 0), (0x01, 500, 1), (0x20, 300, 0)]), ("reset", [3])]}
    with api.Receiver(MODE_N, 0x2F, 0, 0, **kw) as r:
        n, _ = segments.run_segments(r, parts, ops, (0x2F, 0, 0), in10x=(rate == 10), bits=(mode == "bits"))
    assert n > 0


def test_reconfigure_mid_run():
    """With submits still queued: configure some streams before submit 2 and again before submit 4, reset a configured one
    (it keeps its settings), configure and reset one stream before one submit, duplicate indices (the last wins); streams
    never touched carry on as in a run without any call."""
    n_streams = 10
    sizes = (2, 1, 2, 2, 1, 2)
    iq = make_input(13, n_streams, sum(sizes))
    parts = parity.cut(iq, sizes)
    ops = {0: [("conf", [0], [(0x01, 0, 0)])],  # before the first submit
           2: [("conf", [1, 2, 2], [(0x21, 900, 1), (0x2F, 500, 0), (0x01, 0, 0)]),  # (duplicate: the last wins)
               ("reset", [4])],
           3: [("reset", [1])],  # a configured stream keeps its settings
           4: [("conf", [5], [(0x06, 300, 1)]), ("reset", [5]), ("reset", [6]), ("conf", [6], [(0x20, 0, 0)])]}
    dflt = (0x2F, 500, 0)
    with api.Receiver(n_streams, *dflt, max_blocks=max(sizes), all_flushes=True) as r:
        segments.run_segments(r, parts, ops, dflt)
        assert r.stream_config(2) == {"types_mask": 0x01, "thresh": 0, "filter_type": 0}
    with api.Receiver(n_streams, *dflt, max_blocks=max(sizes), all_flushes=True) as r:  # untouched streams: as without calls
        ev_plain = parity.run_fifo(r, parts, depth=1)
    with api.Receiver(n_streams, *dflt, max_blocks=max(sizes), all_flushes=True) as r:
        ev_conf = []
        for k, p in enumerate(parts):
            for op in ops.get(k, ()):
                if op[0] == "conf":
                    r.configure_streams(op[1], *zip(*op[2]))
                else:
                    r.reset_streams(op[1])
            r.submit(np.ascontiguousarray(p))
            ev_conf.append(r.drain())
    for s in (3, 7, 8, 9):
        a = np.concatenate([e[e["stream"] == s] for e in ev_plain])
        b = np.concatenate([e[e["stream"] == s] for e in ev_conf])
        assert len(a) > 0 and a.tobytes() == b.tobytes(), "stream %d" % s


@pytest.mark.parametrize("dflt", [(0x2F, 500, 0), (0x2F, 0, 1)], ids=["fixed-narrow", "auto-wide"])
def test_configuring_the_context_settings_changes_nothing(dflt):
    n_streams = 8
    iq = make_input(14, n_streams, sum(SIZES))
    parts = parity.cut(iq, SIZES)
    out = []
    for conf in (False, True):
        with api.Receiver(n_streams, *dflt, max_blocks=max(SIZES), all_flushes=True) as r:
            if conf:
                r.configure_streams(range(n_streams), *dflt)
            ev = np.concatenate(parity.run_fifo(r, parts, depth=1))
            out.append((ev, [r.thresh(s) for s in range(n_streams)]))
    assert len(out[0][0]) > 2 * n_streams
    assert out[0][0].tobytes() == out[1][0].tobytes()
    assert out[0][1] == out[1][1]


def test_argument_errors_mark_nothing():
    n_streams = 4
    iq = make_input(15, n_streams, 6)
    parts = parity.cut(iq, (3, 3))

    def run(calls):
        with api.Receiver(n_streams, 0x23, 500, 0, max_blocks=3, all_flushes=True) as r:
            r.submit(np.ascontiguousarray(parts[0]))
            for c in calls:
                c(r)
            r.submit(np.ascontiguousarray(parts[1]))
            return np.concatenate([r.drain(), r.drain()])

    def bad(r):
        L = r.L

        def conf(streams, cfgs, n=None):
            idx = np.array(streams, dtype=np.int32)
            arr = (api.StreamConfig * max(1, len(cfgs)))(*[api.StreamConfig(*c) for c in cfgs])
            return L.tfrec_amd_configure_streams(r.h, idx.ctypes.data if len(idx) else None, api.C.cast(arr, api.C.c_void_p),
                                                 len(streams) if n is None else n)

        good = (0x01, 0, 0, 0)
        for streams, cfgs in (([1, 4], [good, good]), ([-1], [good]),  # an index outside [0, 4): not even stream 1
                              ([1, 2], [good, (0x00, 0, 0, 0)]), ([1, 2], [good, (0x04, 0, 0, 0)]),  # empty / outside 0x23
                              ([1, 2], [good, (0x40, 0, 0, 0)]), ([1], [(0x01, -1, 0, 0)]), ([1], [(0x01, 0, 2, 0)]),
                              ([1], [(0x01, 0, -1, 0)]), ([1], [(0x01, 0, 0, 1)])):
            assert conf(streams, cfgs) == api.E_INVAL, (streams, cfgs)
        assert conf([1], [good], n=-1) == api.E_INVAL
        assert L.tfrec_amd_configure_streams(r.h, None, None, 1) == api.E_INVAL
        assert L.tfrec_amd_configure_streams(r.h, np.array([1], dtype=np.int32).ctypes.data, None, 1) == api.E_INVAL
        assert L.tfrec_amd_configure_streams(r.h, None, None, 0) == api.E_OK
        for wrong in ([4], [-1], [2 ** 32 + 1]):
            with pytest.raises(api.TfrecAmdError):
                r.configure_streams(wrong, thresh=0)
        with pytest.raises(api.TfrecAmdError):
            r.configure_streams([0], types_mask=0x08)
        assert r.stream_config(1) == {"types_mask": 0x23, "thresh": 500, "filter_type": 0}
        r.configure_streams([])

    none = run([])
    assert len(none) > 0
    assert none.tobytes() == run([bad]).tobytes()


# ---- tfrec_gpu -p
FILES = [  # (blocks, -p spec, the same as global options)
    (5, "T=1,t=0", ["-T", "1", "-t", "0"]),
    (7, None, ["-T", "2f", "-t", "500"]),
    (3, "T=20,W=1", ["-T", "20", "-t", "500", "-W"]),
    (6, "t=300,W=1,T=6", ["-T", "6", "-t", "300", "-W"]),
    (4, "T=2f", ["-T", "2f", "-t", "500"]),
]


@pytest.fixture(scope="module")
def dumps(tmp_path_factory):
    parity.build_cli()
    d = tmp_path_factory.mktemp("pdumps")
    files = []
    for k, (nb, _, _) in enumerate(FILES):
        p = d / ("f%d.iq" % k)
        p.write_bytes((pulse_stream(70 + k, nb) if k % 2 else synth.gen_stream(70, k, nb)).tobytes())
        files.append(str(p))
    return d, files


def p_args(files):
    a = []
    for (_, spec, _), f in zip(FILES, files):
        a += (["-p", spec] if spec else ["-p", "t=500"]) + ["-L", f]  # ("t=500" with the global -t 500: no change)
    return a


@pytest.mark.parametrize("extra", [[], ["-n", "1"], ["-n", "2"], ["-m", "1"]], ids=["default", "n1", "n2", "summary"])
def test_tfrec_gpu_per_file_settings(dumps, extra):
    d, files = dumps
    out, recs = parity.cli(["-b", "4", "-T", "2f", "-t", "500"] + extra + p_args(files), d / "p.out")
    n = 0
    for k, f in enumerate(files):
        _, alone = parity.cli(["-b", "4"] + FILES[k][2] + extra + ["-L", f], d / ("a%d.out" % k))
        got = [r[1:] for r in recs if r[0] == str(k)]
        assert got == [r[1:] for r in alone], "file %d" % k
        n += len(got)
    assert n >= 5


def test_tfrec_gpu_without_p_is_unchanged(dumps):
    d, files = dumps
    largs = sum((["-L", f] for f in files), [])
    base = parity.cli(["-b", "4", "-T", "2f", "-t", "500"] + largs, d / "b0.out")
    assert base == parity.cli(["-b", "4", "-T", "2f", "-t", "500", "-p", "T=2f,t=500,W=0"] + largs, d / "b1.out")
