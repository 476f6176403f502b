"""Per-stream reset (tfrec_amd_reset_streams / Receiver.reset_streams) on the GPU, event by event against the oracle.

A stream reset before submit k behaves, from submit k on, exactly like a fresh receiver fed only the input that follows
(seq from 0, end_sample from 0); before it, like a fresh receiver run on the old input cut at the reset (a window open at
the cut is dropped without a flush, as the reference drops it when the process exits at the end of a dump).  Every other
stream carries on untouched.  Compared in every field: slot, end_sample, byte_cnt, rssi, offset, rdata, rssi_raw, status
and seq."""
import json
import os

import numpy as np
import pytest

import parity
import segments
from tfrec_amd import api, synth

pytestmark = pytest.mark.gpu

B = api.BLOCK_BYTES


def check_resets(r, parts, resets, types=0x2F, thresh=500, wide=0, **kw):
    """resets[k]: the streams reset before submit k.  Nothing is read from the receiver between the submits: the resets arrive
    with the FIFO full.  -> events compared."""
    ops = {k: [("reset", streams)] for k, streams in resets.items()}
    return segments.run_segments(r, parts, ops, (types, thresh, wide), read_between=False, **kw)[0]


N_STREAMS = 8
SIZES = (3, 2, 4, 3, 2)  # blocks of the five submits
RESETS = {2: [1, 4, 6]}  # before the 3rd submit


LAYOUTS = pytest.mark.parametrize("layout", ["deep", "shallow", "serial"])


def make_receiver(layout, monkeypatch, **kw):
    mode, want, _ = parity.mode_kwargs("serial_chains" if layout == "serial" else layout, monkeypatch)
    r = api.Receiver(N_STREAMS, **dict(mode, **kw))
    assert r.layout() == want
    return r


@LAYOUTS
@pytest.mark.parametrize("thresh", [500, 0])
def test_reset_some_streams(layout, thresh, monkeypatch):
    iq = synth.gen_batch(71, 0, N_STREAMS, sum(SIZES))
    parts = parity.cut(iq, SIZES)
    with make_receiver(layout, monkeypatch, thresh=thresh, max_blocks=max(SIZES), all_flushes=True) as r:
        n = check_resets(r, parts, RESETS, thresh=thresh)
    assert n > 20 * N_STREAMS


@pytest.mark.parametrize("layout", ["deep", "serial"])
def test_reset_some_streams_wide_filter(layout, monkeypatch):
    iq = synth.gen_batch(72, 0, N_STREAMS, sum(SIZES))
    parts = parity.cut(iq, SIZES)
    with make_receiver(layout, monkeypatch, thresh=0, filter_type=1, max_blocks=max(SIZES), all_flushes=True) as r:
        check_resets(r, parts, RESETS, thresh=0, wide=1)


def test_reset_some_streams_bits_mode():
    iq = synth.gen_batch(73, 0, N_STREAMS, sum(SIZES))
    parts = parity.cut(iq, SIZES)
    with api.Receiver(N_STREAMS, max_blocks=max(SIZES), all_flushes=True, bits=True, max_events=1 << 17) as r:
        check_resets(r, parts, RESETS, bits=True)


@pytest.mark.parametrize("layout", ["deep", "shallow"])
def test_reset_with_whb_check_forced_to_fail(layout, monkeypatch):
    """Every other (stream + submit) is declared failed by the WHB check: the exact redo runs on reset streams too, from the
    snapshot (whbsnap / whbx0) the reset submit took of the restored state."""
    monkeypatch.setenv("TFREC_AMD_WHB_FORCE_FAIL", "2")
    if layout == "shallow":
        monkeypatch.setenv("TFREC_AMD_DEEP", "0")
    iq = synth.gen_batch(74, 0, N_STREAMS, sum(SIZES))
    parts = parity.cut(iq, SIZES)
    with api.Receiver(N_STREAMS, max_blocks=max(SIZES), all_flushes=True, experiments=True) as r:
        check_resets(r, parts, RESETS)
        assert r.stats()["whb_respeculated"] > 0


def test_reset_on_the_10x_input():
    sizes = (2, 1, 2, 1, 2)
    bb = 10 * B
    iq = np.stack([synth.gen_stream(75, s, sum(sizes), rate_mult=10) for s in range(N_STREAMS)])
    parts = parity.cut(iq, sizes, bb)
    with api.Receiver(N_STREAMS, max_blocks=max(sizes), all_flushes=True, input_10x=True) as r:
        n = check_resets(r, parts, RESETS, in10x=True)
    assert n > 0


def test_windows_open_at_the_cut_are_dropped():
    """A burst of each of the five protocols (the WHB one synced) straddles the reset point of its stream: the open trigger
    window produces no flush, and what follows equals a fresh receiver."""
    cut_blocks, n_blocks = 3, 6
    cut = cut_blocks * B // 2  # input samples
    rows = []
    for p in range(5):
        probe = {"proto": p, "start": 1000, "payload_seed": 2}
        n = synth.gen_scene(80 + p, n_blocks, [probe], with_truth=True)[1][0]["length"]  # the straddling burst's length
        bursts = [{"proto": p, "start": 20000, "payload_seed": 1},
                  {"proto": p, "start": cut - (n * 3) // 4, "payload_seed": 2},  # 3/4 of it before the cut: synced, open
                  {"proto": p, "start": cut + 30000, "payload_seed": 3}]
        rows.append(synth.gen_scene(80 + p, n_blocks, bursts))
    rows.append(synth.gen_batch(81, 0, 1, n_blocks)[0])
    iq = np.stack(rows)
    parts = parity.cut(iq, (cut_blocks, n_blocks - cut_blocks))
    resets = {1: [0, 1, 2, 3, 4]}
    with api.Receiver(len(rows), max_blocks=cut_blocks, all_flushes=True) as r:
        check_resets(r, parts, resets)
    m = cut // 4  # decimated samples before the cut
    for s in range(5):  # the cut matters: one receiver over the whole row flushes the straddling burst's window
        whole = sorted(parity.fresh_oracle(iq[s], 0x2F, 500, 0).events_full())
        before = parity.fresh_oracle(iq[s, :2 * cut], 0x2F, 500, 0).events_full()
        after = [(e[0], e[1] + m) + e[2:] for e in parity.fresh_oracle(iq[s, 2 * cut:], 0x2F, 500, 0).events_full()]
        assert whole != sorted(before + after), "stream %d: no window open at the cut" % s


@pytest.mark.parametrize("bits", [False, True], ids=["flushes", "bits"])
def test_reset_every_stream_equals_a_new_context(bits):
    """After every stream is reset, the drained events equal those of a new context fed the same input in every field, BITS
    chunks included (their end_sample is the first sample of their window, counted from the reset like a flush's)."""
    iq = synth.gen_batch(76, 0, N_STREAMS, 9)
    parts = parity.cut(iq, (3, 3, 3))
    kw = dict(max_blocks=3, all_flushes=True, bits=bits, max_events=1 << 16)
    with api.Receiver(N_STREAMS, **kw) as r:
        evs = parity.run_fifo(r, parts, before=lambda k: r.reset_streams(range(N_STREAMS)) if k == 1 else None)
    with api.Receiver(N_STREAMS, **kw) as r2:
        evs2 = parity.run_fifo(r2, parts[1:])
    got, want = np.concatenate(evs[1:]), np.concatenate(evs2)
    assert len(want) > 2 * N_STREAMS
    assert bool((want["status"] == api.STATUS_BITS).any()) == bits
    assert got.tobytes() == want.tobytes()


def test_stream_recycled_before_every_submit():
    """The recycling pattern: streams 2 and 5 get a new short input before every submit."""
    parts = [synth.gen_batch(90 + k, 10 * k, N_STREAMS, nb) for k, nb in enumerate((2, 1, 3, 2, 1, 2))]
    resets = {k: [2, 5] for k in range(1, len(parts))}
    with api.Receiver(N_STREAMS, thresh=0, max_blocks=3, all_flushes=True) as r:
        check_resets(r, parts, resets, thresh=0)


@pytest.mark.parametrize("proto", ["tfa_1", "tfa_2", "tfa_3", "tx22", "whb"])
def test_reset_stream_reproduces_the_real_reference_fixture(proto, golden_dir):
    """No oracle in between: after unrelated input, a reset stream fed tests/golden/iq_<proto>.npz yields the events the real
    reference minted for that file."""
    g = np.load(os.path.join(golden_dir, "iq_%s.npz" % proto))
    meta = json.loads(str(g["meta"]))
    fx = g["iq"]
    nb = len(fx) // B
    first = synth.gen_batch(77, 0, 3, 4)
    second = synth.gen_batch(78, 0, 3, nb)
    second[1] = fx
    with api.Receiver(3, meta["types"], meta["thresh"], meta["wide"], max_blocks=max(4, nb), all_flushes=True) as r:
        evs = parity.run_fifo(r, [first, second], before=lambda k: r.reset_streams([1]) if k == 1 else None)
    got = sorted(api.event_tuples(evs[1], 1))
    want = sorted((e[0], e[1], e[2], e[3], e[4], bytes.fromhex(e[5])) for e in meta["events"])
    assert got == want


def test_api_edge_cases():
    iq = synth.gen_batch(79, 0, 4, 6)
    parts = parity.cut(iq, (3, 3))

    def run(calls):
        with api.Receiver(4, max_blocks=3, all_flushes=True) as r:
            r.submit(np.ascontiguousarray(parts[0]))
            for c in calls:
                c(r)
            r.submit(np.ascontiguousarray(parts[1]))
            return np.concatenate([r.drain(), r.drain()])

    once = run([lambda r: r.reset_streams([0, 1, 2, 3])])
    assert once.tobytes() == run([lambda r: r.reset_streams([3, 0, 3, 1]), lambda r: r.reset_streams([2, 2, 1])]).tobytes()
    none = run([])
    assert none.tobytes() == run([lambda r: r.reset_streams([])]).tobytes()
    assert none.tobytes() != once.tobytes()

    def bad(r):
        L = r.L
        idx = np.array([1, 4], dtype=np.int32)  # 4 is out of range: nothing is marked, not even 1
        assert L.tfrec_amd_reset_streams(r.h, idx.ctypes.data, 2) == api.E_INVAL
        assert L.tfrec_amd_reset_streams(r.h, np.array([-1], dtype=np.int32).ctypes.data, 1) == api.E_INVAL
        assert L.tfrec_amd_reset_streams(r.h, idx.ctypes.data, -1) == api.E_INVAL
        assert L.tfrec_amd_reset_streams(r.h, None, 1) == api.E_INVAL
        assert L.tfrec_amd_reset_streams(r.h, None, 0) == api.E_OK
        for wrong in ([7], [-1], [2 ** 32 + 1]):  # (2**32 + 1 must not wrap to stream 1)
            with pytest.raises(api.TfrecAmdError):
                r.reset_streams(wrong)

    assert none.tobytes() == run([bad]).tobytes()
