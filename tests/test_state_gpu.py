"""tfrec_amd_save_streams / tfrec_amd_load_streams (Receiver.save_streams / load_streams) on the GPU.

Every case has one shape.  Context A runs the first part of its rows and saves its streams; context B -- 65 streams, another
n_streams -- loads the blobs into other streams, one of them stream 64 (the lane past a wave's end), and runs the rest.  A's events
and B's, B's relabelled with the source stream, must be the events of the uninterrupted run in every field, seq and end_sample
included: the oracle's where the oracle models the context's input, and always those of one context U that ran both parts.

The input (scene) has, per protocol, one row with a telegram whose trigger window is open at the cut: asserted on the CPU before the
GPU is used (open_at_the_cut) -- the uninterrupted oracle decodes it, a fresh receiver on the second part alone does not.  The five
protocols cannot share a row (one trigger opens every slot's window, and overlapping bursts destroy each other), so A has five
source streams, one per registered slot."""
import functools

import numpy as np
import pytest

import parity
from state_harness import DST, NB_, b_rows, continue_in_b, open_at_the_cut, relabel
from oracle import oracle as O
from recorder import raises
from tfrec_amd import api, formats, resample, state, synth, tune

pytestmark = pytest.mark.gpu

B = api.BLOCK_BYTES
TYPES = 0x2F


@functools.lru_cache(maxsize=None)
def scene_and_bursts(p=1, q=1, first=2, rest=2, f0=0, seed=80, amp=60):
    """(u8 rows [5, bytes] at 1536000 p / q, the burst across the cut per row as (start, length) in decimated samples).  Row k holds
    bursts of protocol k (at f0 Hz from the centre): one early, one whose telegram is three quarters through at the cut behind
    `first` blocks, one behind it -- the WHB row (a WHB telegram is longer than three blocks) only the one across the cut, half
    through there."""
    n_blocks = first + rest
    cut = first * (B // 2) * p  # samples at 1536000 p
    rows, across = [], []
    for k in range(5):
        probe = {"proto": k, "start": 1000 * p, "payload_seed": 2, "f0_hz": f0, "amp": amp}
        n = synth.gen_scene(seed + k, n_blocks, [probe], with_truth=True, rate_mult=p)[1][0]["length"]
        mid = {"proto": k, "start": cut - ((n * 3) // 4 if k < 4 else n // 2), "payload_seed": 2, "f0_hz": f0, "amp": amp}
        assert mid["start"] > 0 and mid["start"] + n < n_blocks * (B // 2) * p
        bursts = [mid] if k == 4 else [{"proto": k, "start": 20000 * p, "payload_seed": 1, "f0_hz": f0, "amp": amp}, mid,
                                       {"proto": k, "start": cut + 30000 * p, "payload_seed": 3, "f0_hz": f0, "amp": amp}]
        u = synth.gen_scene(seed + k, n_blocks, bursts, rate_mult=p)
        rows.append(np.ascontiguousarray(u.reshape(-1, 2)[::q]).reshape(-1))
        across.append((mid["start"] // (4 * p), n // (4 * p)))
    iq = np.stack(rows)
    iq.setflags(write=False)
    return iq, tuple(across)


def scene(*a, **kw):
    return scene_and_bursts(*a, **kw)[0]


def across(*a, **kw):
    return scene_and_bursts(*a, **kw)[1]


# ---- 1, 2, 8: the plain context
@functools.lru_cache(maxsize=None)
def plain_oracles(thresh=500):
    iq = scene()
    return open_at_the_cut(lambda x: parity.fresh_oracle(x, TYPES, thresh), [(iq[k], 2 * B) for k in range(5)], 2, across(), "plain")


def test_plain_context_continues_in_stream_64_and_the_others_run_their_own():
    orcs = plain_oracles()
    iq = scene()
    parts = [np.ascontiguousarray(v) for v in parity.cut(iq, (2, 2))]
    others = synth.gen_batch(61, 0, NB_, 2)
    ev_a, got, _, blobs, ev_b, _ = continue_in_b(parts, lambda n: api.Receiver(n, TYPES, 500, 0, max_blocks=2, all_flushes=True), others=others)
    both = np.concatenate([ev_a, got])
    for k in range(5):
        assert parity.assert_segment(both, k, orcs[k], "row %d" % k) > 0
    # B's other 60 streams ran their own input from their own start
    for s in sorted(set(range(NB_)) - set(DST)):
        parity.assert_segment(ev_b, s, parity.fresh_oracle(others[s], TYPES, 500), "B's own stream %d" % s)
    h = state.parse_header(blobs[0])
    assert h["samples_since_restart"] == 2 * api.BLOCK_DEC and h["types_mask"] == TYPES and h["input_kind"] == 0
    assert h["config"] == {"types_mask": TYPES, "thresh": 500, "filter_type": 0, "reserved": 0}
    assert h["version_hash"] == state.version_hash(api.load_library().tfrec_amd_version())
    assert h["reserved"] == bytes(20) and (h["tune_hz"], h["tune_wide_hz"], h["tune_input_hz"]) == (0, 0, 0)


def test_save_then_load_into_the_same_stream_changes_nothing():
    iq = scene()
    parts = [np.ascontiguousarray(v) for v in parity.cut(iq, (2, 2))]
    with api.Receiver(5, TYPES, 500, 0, max_blocks=2, all_flushes=True) as r:
        r.submit(parts[0])
        first = r.drain()
        blobs = r.save_streams(range(5))
        r.load_streams(range(5), blobs)
        assert r.save_streams(range(5)).tobytes() == blobs.tobytes()
        r.submit(parts[1])
        ev = np.concatenate([first, r.drain()])
    for k, o in enumerate(plain_oracles()):
        parity.assert_segment(ev, k, o, "row %d" % k)


def test_configured_streams_bring_their_settings_into_a_context_of_other_defaults():
    """The sources run with their own threshold and types (tfrec_amd_configure_streams); B was made with other ones.  The load applies
    the saved settings without a restart, B's kernels read every stream's own from then on, and B's other streams keep B's."""
    iq = scene()
    types = [TYPES & ~(1 << (5 if k == 0 else 0)) for k in range(5)]  # (each row keeps its own protocol's slot)
    orcs = [open_at_the_cut(lambda x, t=t: parity.fresh_oracle(x, t, 700), [(iq[j], 2 * B) for j in range(5)], 2, across(), "configured",
                            only=k)[0] for k, t in enumerate(types)]
    parts = [np.ascontiguousarray(v) for v in parity.cut(iq, (2, 2))]
    others = synth.gen_batch(63, 0, NB_, 2)
    ev_a, got, _, blobs, ev_b, _ = continue_in_b(parts, lambda n: api.Receiver(n, TYPES, 500, 0, max_blocks=2, all_flushes=True),
                                                 setup=lambda r, s: r.configure_streams(s, types_mask=types, thresh=700), others=others)
    both = np.concatenate([ev_a, got])
    for k in range(5):
        assert parity.assert_segment(both, k, orcs[k], "row %d" % k) > 0
    for s in (1, 5, 62):
        parity.assert_segment(ev_b, s, parity.fresh_oracle(others[s], TYPES, 500), "B's own stream %d" % s)
    assert state.parse_header(blobs[0])["config"] == {"types_mask": types[0], "thresh": 700, "filter_type": 0, "reserved": 0}


# ---- 3: the auto threshold
def test_auto_threshold_and_read_thresh_continue():
    orcs = open_at_the_cut(lambda x: parity.fresh_oracle(x, TYPES, 0), [(scene(amp=25)[k], 2 * B) for k in range(5)], 2, across(amp=25), "auto")
    parts = [np.ascontiguousarray(v) for v in parity.cut(scene(amp=25), (2, 2))]

    def side(r):
        r.sync()
        return [r.thresh(s) for s in (DST[:5] if r.n_streams == NB_ else range(5))]

    ev_a, got, _, _, _, (sa, sb, sw) = continue_in_b(parts, lambda n: api.Receiver(n, TYPES, 0, 0, max_blocks=2, all_flushes=True), side=side)
    both = np.concatenate([ev_a, got])
    for k in range(5):
        parity.assert_segment(both, k, orcs[k], "row %d" % k)
    assert sa == sw[0] and sb == sw[1]
    # fm_demod.cpp:58-73 moves the threshold behind every fourth block of a stream: behind B's second block, which is the fourth
    # only if the block count travelled, by the triggered average of all four
    assert all(v == 500 for v in sw[0]) and any(v != 500 for v in sw[1]), "the threshold does not move on this scene"


# ---- 4: the other input kinds
def test_serial_chains_context():
    orcs = plain_oracles()
    parts = [np.ascontiguousarray(v) for v in parity.cut(scene(), (2, 2))]
    ev_a, got, *_ = continue_in_b(parts, lambda n: api.Receiver(n, TYPES, 500, 0, max_blocks=2, all_flushes=True, serial_chains=True))
    both = np.concatenate([ev_a, got])
    for k in range(5):
        parity.assert_segment(both, k, orcs[k], "row %d" % k)


W10 = 3300000


def test_10x_input_with_a_wide_tune():
    iq = scene(10, 1, f0=W10)
    run = lambda x: _s16_oracle(tune.decim10_s16(tune.mix10_s16(tune.s16_of_u8(x), W10)))
    orcs = open_at_the_cut(run, [(iq[k], 2 * 10 * B) for k in range(5)], 2, across(10, 1, f0=W10), "10x")
    parts = [np.ascontiguousarray(v) for v in parity.cut(iq, (2, 2), 10 * B)]
    ev_a, got, _, blobs, *_ = continue_in_b(parts, lambda n: api.Receiver(n, TYPES, 500, 0, max_blocks=2, all_flushes=True, input_10x=True),
                                            setup=lambda r, s: r.tune_streams_wide(s, W10))
    both = np.concatenate([ev_a, got])
    for k in range(5):
        parity.assert_segment(both, k, orcs[k], "row %d" % k)
    h = state.parse_header(blobs[0])
    assert (h["tune_wide_hz"], h["tune_input_hz"], h["input_kind"]) == (W10, W10, 1)


def _s16_oracle(x16, thresh=500):
    o = O.Oracle(TYPES, thresh, 0)
    o.process_s16(x16)
    return o


def rate_case(p, q, fmt, first, rest, input_hz, narrow_hz, stage0=False):
    """A rate or format receiver over scene(p, q) in the format, its bursts at input_hz + narrow_hz."""
    iq = scene(p, q, first, rest, f0=input_hz + narrow_hz)
    raw = np.stack([formats.encode(fmt, formats.to_x("u8", row)) for row in iq]) if fmt != "u8" else iq
    cut = formats.bytes_per_sample(fmt) * resample.input_samples(first, p, q)

    def stage0_of(x):  # (at 1/1 the format conversion alone: no resampling stage, no input-rate mixer)
        return x if (p, q) == (1, 1) else resample.resample_x16(tune.mix_in_s16(x, input_hz, p, q), p, q)

    def restate(row):
        x = formats.to_x(fmt, row)
        return tune.mix_s16(stage0_of(x), narrow_hz, 0)

    # (the second part alone: a fresh receiver's mixers and histories start there)
    orcs = open_at_the_cut(lambda r: _s16_oracle(restate(r)), [(raw[k], cut) for k in range(5)], first,
                           across(p, q, first, rest, f0=input_hz + narrow_hz), "%d/%d %s" % (p, q, fmt))
    parts = parity.cut_input(raw, (first, rest), fmt, p, q)
    kw = {"input_rate": (p, q)}
    if fmt != "u8":
        kw["input_format"] = fmt

    def setup(r, s):
        if input_hz:
            r.tune_streams_input(s, input_hz)
        if narrow_hz:
            r.tune_streams(s, narrow_hz)

    def side(r):
        if not stage0:
            return None
        r.sync()
        idx = DST[:5] if r.n_streams == NB_ else range(5)
        return [r.stage0(s, r.cfg.max_blocks * 4 * api.BLOCK_DEC) for s in idx]

    ev_a, got, _, blobs, _, (sa, sb, sw) = continue_in_b(
        parts, lambda n: api.Receiver(n, TYPES, 500, 0, max_blocks=max(first, rest), all_flushes=True, **kw), setup=setup, side=side)
    both = np.concatenate([ev_a, got])
    for k in range(5):
        parity.assert_segment(both, k, orcs[k], "row %d" % k)
    if stage0:  # the phase of the input mixer and the resampler's history continue: stage 0 behind the cut, bit for bit
        n0 = 2 * first * 4 * api.BLOCK_DEC
        for k in range(5):
            want = stage0_of(formats.to_x(fmt, raw[k]))
            assert np.array_equal(sb[k], want[n0:]), "stage 0 of row %d behind the cut" % k
    return blobs


def test_rate_4_3_with_an_input_tune_and_a_narrow_tune_pins_the_phase():
    blobs = rate_case(4, 3, "u8", 3, 3, 250000, -120000, stage0=True)
    h = state.parse_header(blobs[0])
    assert (h["tune_hz"], h["tune_wide_hz"], h["tune_input_hz"], h["rate_p"], h["rate_q"]) == (-120000, 0, 250000, 4, 3)


def test_format_s16_at_25_16():
    rate_case(25, 16, "s16", 2, 2, 0, 0)


def test_format_f32_at_1_1():
    blobs = rate_case(1, 1, "f32", 2, 2, 0, 0)
    assert state.parse_header(blobs[0])["input_kind"] == 3


def test_decimated_input_with_submit_runs():
    """A channel-rate context fed sparse submits: every row as one run per submit (its pre sample the last pair of the part before)."""
    orcs = [parity.fresh_oracle(x, TYPES, 500, keep_dec=True) for x in scene()]
    plain_oracles()  # (the input condition: the decimated samples are the plain scene's)
    dec = np.stack([o.dec().reshape(-1, 2) for o in orcs])
    m = 2 * api.BLOCK_DEC
    from tfrec_amd import capture

    def table(rows_of, part):
        runs = np.zeros(len(rows_of), dtype=capture.RUN_DTYPE)
        runs["stream"] = sorted(rows_of)
        runs["start_sample"] = 0
        runs["n_samples"] = m
        runs["pool_offset"] = np.arange(len(rows_of)) * m
        order = [rows_of[s] for s in sorted(rows_of)]
        pool = np.concatenate([dec[k, part * m:(part + 1) * m] for k in order])
        pre = np.stack([dec[k, part * m - 1] if part else np.zeros(2, np.int16) for k in order])
        return runs, pool, pre

    def make(n):
        r = api.Receiver(n, TYPES, 500, 0, max_blocks=2, all_flushes=True, decimated=True)
        r.enable_runs_input(8, 5 * m)
        return r

    def submit(r, part):
        rows_of = {j: i for i, j in enumerate(DST)} if r.n_streams == NB_ else {i: i for i in range(5)}
        r.submit_runs(*table(rows_of, part), 2)

    class Part(int):  # (continue_in_b asks a part for its length: the source streams)
        def __len__(self):
            return 5

    ev_a, got, *_ = continue_in_b([Part(0), Part(1)], make, submit=submit)
    both = np.concatenate([ev_a, got])
    for k in range(5):
        parity.assert_segment(both, k, orcs[k], "row %d" % k)


# ---- 5: levels, recorder and burst meter
def test_levels_recorder_and_burst_meter_continue():
    plain_oracles()
    parts = [np.ascontiguousarray(v) for v in parity.cut(scene(), (2, 2))]

    def make(n):
        r = api.Receiver(n, TYPES, 500, 0, max_blocks=2, all_flushes=True, levels=True)
        r.enable_capture(64 * n, n * 2 * api.BLOCK_DEC)
        r.enable_burst_meter()
        return r

    def side(r):
        idx = list(DST) if r.n_streams == NB_ else list(range(5))
        back = {j: i for i, j in enumerate(idx)}
        lv = r.read_levels()[idx]
        runs, pool = r.read_captures()
        bursts = r.read_bursts()
        keep = np.isin(runs["stream"], idx)
        per = []
        for t, bu in zip(runs[keep], bursts[keep]):
            t, bu = t.copy(), bu.copy()
            t["stream"] = back[int(t["stream"])]
            if "stream" in (bu.dtype.names or ()):
                bu["stream"] = back[int(bu["stream"])]
            po = int(t["pool_offset"])
            t["pool_offset"] = 0
            per.append((int(t["stream"]), int(t["start_sample"]), t.tobytes(), bu.tobytes(), pool[po:po + int(t["n_samples"])].tobytes()))
        return lv.tobytes(), sorted(per), runs[keep]["flags"].tolist()

    *_, (sa, sb, sw) = continue_in_b(parts, make, side=side)
    assert sa[:2] == sw[0][:2], "A's records are the uninterrupted run's"
    assert sb[:2] == sw[1][:2], "B's levels, runs, pools and burst records are the uninterrupted run's"
    from tfrec_amd import capture
    assert any(f & capture.RUN_CONTINUES for f in sb[2]), "no run across the cut carries CONTINUES"


# ---- 6: DC blocker and IQ balancer
def test_dc_and_iq_context_read_dc_and_read_iq_continue():
    plain_oracles()
    parts = [np.ascontiguousarray(v) for v in parity.cut(scene(), (2, 2))]

    def side(r):
        idx = DST if r.n_streams == NB_ else range(5)
        return [(r.read_dc(s).tobytes(), r.read_iq(s).tobytes()) for s in idx]

    *_, (sa, sb, sw) = continue_in_b(
        parts, lambda n: api.Receiver(n, TYPES, 500, 0, max_blocks=2, all_flushes=True, dc_windows=96, iq_windows=160), side=side)
    assert sa == sw[0] and sb == sw[1]
    assert sw[1][0] != sw[0][0]


# ---- 7: WHB with forced failures on both sides of the cut
@pytest.mark.parametrize("deep", ["1", "0"])
def test_whb_forced_failures_on_both_sides_of_the_cut(deep, monkeypatch):
    """TFREC_AMD_WHB_FORCE_FAIL = 2 fails every (stream + submit) that is even: A's streams 0, 2, 4 in its only submit, B's 64 and 0
    in its first -- the WHB row (source 4) is redone in A, the rows behind DST 64 and 0 in B."""
    monkeypatch.setenv("TFREC_AMD_WHB_FORCE_FAIL", "2")
    monkeypatch.setenv("TFREC_AMD_DEEP", deep)
    orcs = plain_oracles()
    iq = scene()[[4, 0, 1, 2, 4]]  # the WHB row continues in B's stream 64, and as source 4
    pick = (4, 0, 1, 2, 4)
    parts = [np.ascontiguousarray(v) for v in parity.cut(iq, (2, 2))]
    redone = []

    def side(r):
        r.sync()
        redone.append(r.stats()["whb_respeculated"])

    ev_a, got, *_ = continue_in_b(parts, lambda n: api.Receiver(n, TYPES, 500, 0, max_blocks=2, all_flushes=True, experiments=True), side=side)
    both = np.concatenate([ev_a, got])
    assert not (both["status"] == 0xFF).any()
    for i, k in enumerate(pick):
        parity.assert_segment(both, i, orcs[k], "row %d" % k)
    assert redone[2] > 0 and redone[3] > 0, "no redo in A or in B"


# ---- 9: undrained submits on both sides
def test_save_and_load_with_two_undrained_submits():
    orcs = plain_oracles()
    iq = scene()
    lead = synth.gen_batch(62, 0, NB_, 2)
    p0, p1 = (np.ascontiguousarray(v) for v in parity.cut(iq, (2, 2)))
    halves = [np.ascontiguousarray(v) for v in parity.cut(p0, (1, 1))]
    with api.Receiver(5, TYPES, 500, 0, max_blocks=2, all_flushes=True) as a:
        a.submit(halves[0])
        a.submit(halves[1])
        blobs = a.save_streams(range(5))  # two undrained submits: they stay drainable
        a.submit(p1)                       # ... and A continues as if it had never saved
        ev_a = [a.drain() for _ in range(3)]
    whole = np.concatenate(ev_a)
    for k in range(5):
        parity.assert_segment(whole, k, orcs[k], "A row %d" % k)
    with api.Receiver(NB_, TYPES, 500, 0, max_blocks=2, all_flushes=True) as b:
        lp = [np.ascontiguousarray(v) for v in parity.cut(lead, (1, 1))]
        b.submit(lp[0])
        b.submit(lp[1])
        b.load_streams(DST, blobs)  # B's two undrained submits keep their own origins
        b.submit(b_rows(p1))
        ev_b = [b.drain() for _ in range(3)]
    # B's own first two submits: every stream, the loaded ones included, against its own oracle over the lead
    early = np.concatenate(ev_b[:2])
    for s in (64, 0, 5, 33):  # (end_sample from B's own start: the submits drained behind the load use the origins they ran with)
        parity.assert_segment(early, s, parity.fresh_oracle(lead[s], TYPES, 500), "B's stream %d before the load" % s)
    got = relabel(ev_b[2], {j: i for i, j in enumerate(DST)})
    both = np.concatenate([ev_a[0], ev_a[1], got])
    for k in range(5):
        parity.assert_segment(both, k, orcs[k], "row %d" % k)


# ---- 10: refusals, each followed by an exact continuation
def test_refusals_leave_both_contexts_as_they_were():
    orcs = plain_oracles()
    parts = [np.ascontiguousarray(v) for v in parity.cut(scene(), (2, 2))]
    with api.Receiver(5, TYPES, 500, 0, max_blocks=2, all_flushes=True) as a:
        a.submit(parts[0])
        ev_a = a.drain()
        L, n = a.L, a.state_bytes
        idx = np.arange(5, dtype=np.int32)
        buf = np.zeros(5 * n, dtype=np.uint8)
        assert L.tfrec_amd_save_streams(a.h, idx.ctypes.data, 5, buf.ctypes.data, 5 * n - 1) == api.E_INVAL  # a short buffer
        assert not buf.any()
        raises(api.E_INVAL, a.save_streams, [1, 1])
        with pytest.raises(api.TfrecAmdError):
            a.save_streams([5])
        twice = np.array([0, 5], dtype=np.int32)
        assert L.tfrec_amd_save_streams(a.h, twice.ctypes.data, 2, buf.ctypes.data, buf.nbytes) == api.E_INVAL
        assert L.tfrec_amd_save_streams(a.h, None, 1, buf.ctypes.data, buf.nbytes) == api.E_INVAL
        assert L.tfrec_amd_save_streams(a.h, idx.ctypes.data, -1, buf.ctypes.data, buf.nbytes) == api.E_INVAL
        blobs = a.save_streams(range(5))
        # (a pending reset: E_STATE -- on a context of its own, the reset would cut A's rows)
    with api.Receiver(2, TYPES, 500, 0, max_blocks=2, all_flushes=True) as c:
        c.submit(parts[0][:2])
        c.drain()
        c.reset_streams([1])
        raises(api.E_STATE, c.save_streams, [1])
        raises(api.E_STATE, c.load_streams, [1], blobs[:1])
        # the other stream is saved, and its header is that of A's stream 0 (the payload holds the WHB redo's scratch state, which no
        # context initialises: it need not be equal)
        assert state.parse_header(c.save_streams([0])[0]) == state.parse_header(blobs[0])
    # targets that cannot continue the blobs
    for kw in (dict(types_mask=0x0F), dict(input_rate=(4, 3)), dict(levels=True), dict(serial_chains=True)):
        args = dict(dict(types_mask=TYPES, thresh=500, filter_type=0, max_blocks=3, all_flushes=True), **kw)
        with api.Receiver(2, **args) as t:
            if t.state_bytes == blobs.shape[1]:
                raises(api.E_INVAL, t.load_streams, [0], blobs[:1])
            else:  # (the size differs already: a short or a long buffer)
                padded = np.zeros((1, max(t.state_bytes, blobs.shape[1])), dtype=np.uint8)
                padded[0, :blobs.shape[1]] = blobs[0]
                raises(api.E_INVAL, t.load_streams, [0], padded)
    with api.Receiver(2, TYPES, 500, 0, max_blocks=2, all_flushes=True, levels=True) as lv:  # a source with the level meter ...
        with_levels = lv.save_streams([0])
    with api.Receiver(NB_, TYPES, 500, 0, max_blocks=2, all_flushes=True) as b:
        fresh = b.save_streams(DST)
        raises(api.E_INVAL, b.load_streams, [64], with_levels)  # ... and the flag missing in the target
        raises(api.E_INVAL, b.load_streams, [64], with_levels[:, :blobs.shape[1]])
        bad = blobs.copy()
        bad[3, 0] ^= 1  # a wrong magic in ONE blob of five: nothing is loaded, not even the four before it
        raises(api.E_INVAL, b.load_streams, DST, bad)
        bad = blobs.copy()
        bad[4, 8] ^= 0x40  # a wrong version hash
        raises(api.E_INVAL, b.load_streams, DST, bad)
        bad = blobs.copy()
        bad[0, 4] = 2  # another format version
        raises(api.E_INVAL, b.load_streams, DST, bad)
        bad = blobs.copy()
        bad[1, 72:80] = 0xFF  # samples_since_restart < 0
        raises(api.E_INVAL, b.load_streams, DST, bad)
        assert b.L.tfrec_amd_load_streams(b.h, np.array(DST, dtype=np.int32).ctypes.data, 5, blobs.ctypes.data, blobs.nbytes - 1) == api.E_INVAL
        raises(api.E_INVAL, b.load_streams, DST[:2], blobs[:2, :-16])  # truncated blobs
        raises(api.E_INVAL, b.load_streams, [64, 64], blobs[:2])
        with pytest.raises(api.TfrecAmdError):
            b.load_streams([65], blobs[:1])
        assert b.save_streams(DST).tobytes() == fresh.tobytes(), "a refused load touched the context"
        b.load_streams(DST, blobs)
        b.submit(b_rows(parts[1]))
        got = relabel(b.drain(), {j: i for i, j in enumerate(DST)})
    both = np.concatenate([ev_a, got])
    for k in range(5):
        parity.assert_segment(both, k, orcs[k], "row %d" % k)


def test_a_mapped_stream_is_refused_and_the_staging_is_counted():
    with api.Receiver(4, TYPES, 500, 0, max_blocks=1) as r:
        before = r.memory()["device_bytes"]
        n = r.state_bytes
        assert r.memory()["device_bytes"] == before
        r.save_streams([0])
        assert r.memory()["device_bytes"] == before + 4 * n + 4 * 4
        r.save_streams([1, 2])
        assert r.memory()["device_bytes"] == before + 4 * n + 4 * 4
    with api.Receiver(4, TYPES, 500, 0, max_blocks=1) as r:
        r.map_streams([2], [1])
        r.submit(np.full((4, B), 128, dtype=np.uint8))
        r.drain()
        raises(api.E_INVAL, r.save_streams, [2])
        raises(api.E_INVAL, r.save_streams, [1])  # the row stream 2 reads
        assert r.save_streams([0, 3]).shape == (2, r.state_bytes)


# ---- 11: tfrec_gpu -k / -K
def test_cli_keep_and_continue_give_the_whole_files_telegrams(tmp_path, golden_dir):
    """The golden WHB scene (six blocks, one telegram of more than three) cut at a byte offset inside its fourth block: -k on the first
    part runs three blocks and keeps the rest, -K on the second reads the rest ahead of it and runs the other three.  The receiver's
    state crosses at the end of block three, with the telegram's window open."""
    import json
    import os

    g = np.load(os.path.join(golden_dir, "iq_whb.npz"))
    meta = json.loads(str(g["meta"]))
    iq = g["iq"]
    cut, state_cut = 3 * B + 12346, 3 * B
    assert len(iq) == 6 * B and cut % B != 0 and cut % 2 == 0
    run = lambda x: parity.fresh_oracle(x, meta["types"], meta["thresh"], meta["wide"])
    whole, head, tail = run(iq), run(iq[:state_cut]), run(iq[state_cut:])
    tel = [e for e in whole.events_full() if e[0] == 4 and e[7] == 1]
    assert len(tel) == 1 and tel[0][1] > 3 * api.BLOCK_DEC  # flushed behind the cut ...
    assert not [e for e in head.events_full() if e[7] == 1 and e[0] == 4]  # ... its window still open there ...
    assert not [e for e in tail.events_full() if e[7] == 1 and e[5] == tel[0][5]]  # ... and lost to a receiver that starts there
    assert len(parity.telegram_lines(whole.text())) > len(parity.telegram_lines(head.text())) + len(parity.telegram_lines(tail.text()))
    parity.build_cli()
    paths = [str(tmp_path / n) for n in ("whole.iq", "part1.iq", "part2.iq")]
    for p, x in zip(paths, (iq, iq[:cut], iq[cut:])):
        x.tofile(p)
    common = ["-T", "%x" % meta["types"], "-t", str(meta["thresh"])] + (["-W"] if meta["wide"] else [])
    pfx = str(tmp_path / "keep")
    want = parity.telegram_lines(parity.cli_stdout(common + ["-L", paths[0]], timeout=120))
    one = parity.telegram_lines(parity.cli_stdout(common + ["-b", "2", "-k", pfx, "-L", paths[1]], timeout=120))
    assert os.path.getsize(pfx + ".0.rest") == 12346 and open(pfx + ".0.rest", "rb").read() == iq[state_cut:cut].tobytes()
    h = state.parse_header(np.fromfile(pfx + ".0.state", dtype=np.uint8))
    assert h["samples_since_restart"] == 3 * api.BLOCK_DEC
    two = parity.telegram_lines(parity.cli_stdout(common + ["-K", pfx, "-k", pfx + "2", "-L", paths[2]], timeout=120))
    assert len(want) == len(parity.telegram_lines(whole.text())) >= 1
    assert one + two == want
    assert os.path.getsize(pfx + "2.0.rest") == 0
    assert state.parse_header(np.fromfile(pfx + "2.0.state", dtype=np.uint8))["samples_since_restart"] == 6 * api.BLOCK_DEC
    # without -K the second part is a fresh receiver: the telegram across the cut is lost
    alone = parity.telegram_lines(parity.cli_stdout(common + ["-L", paths[2]], timeout=120))
    assert one + alone != want
