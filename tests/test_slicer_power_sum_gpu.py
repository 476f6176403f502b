"""GPU tests of the TFA_2 family's power sum (tfa2.cpp:371-375: rssi += (rssi + I*I + Q*Q) / 100 while 4 < bitcnt < 10), which
slicer_kernel's lane-per-window walk evaluates behind the walk over the run of samples the phase covered (csrc/slicers.h:
tfa2_power_run).  Every comparison is against the oracle's full events, where the raw accumulator and the offset are fields:
- the phase beginning and ending at every position of the 32-sample chunk grid and of a 16-byte load, for TFA_2, TFA_3 and TX22;
- a submit boundary inside the phase: the window is resumed with a carried bitcnt of 5 .. 9 and a carried accumulator;
- a long window handed to coop_slicer_kernel inside the phase, which continues from the accumulator the head wrote;
- a window that closes inside the phase.
Each test first asserts, from the oracle's events alone, that its scene does what it is for: more than half of the streams flush
a TFA_2-family telegram with a non-zero accumulator, and the case's own condition where the events can show it.  The scenes were
chosen with a sample-by-sample restatement of tfa2_demod::demod that follows bitcnt (not part of the suite); what it found is
written at each builder."""
import functools

import numpy as np
import pytest

import parity
from tfrec_amd import api, synth

pytestmark = pytest.mark.gpu

N = 64            # streams of every case
FAMILY, ALL = 0x0E, 0x2F
THRESH = 500
BLOCK_DEC = api.BLOCK_DEC  # decimated samples per block; 4 input samples, 8 bytes each


def _stack(rows):
    iq = np.stack(rows)
    iq.setflags(write=False)
    return iq


def _carrier(seed, n_blocks, start_dec):
    """A weakly keyed carrier 25 kHz off the centre: it opens the family's windows, and bitcnt stays at 1 for its whole length."""
    return synth.gen_scene(seed, n_blocks, [dict(proto=2, start=4 * start_dec, payload_seed=1, amp=40, fdev_hz=200, f0_hz=25000)])


@functools.lru_cache(maxsize=None)
def alignment_scene(proto):
    """Stream s: 300 samples of carrier from sample 500 on, which open the window, then a burst of the protocol at 800 + s: the
    window begins at the same sample in every stream and the burst's fifth and tenth edge move through it sample by sample, over
    two chunks.  A TFA_1 burst follows in every stream: a foreign burst whose windows the family's slicers walk too."""
    rows = []
    for s in range(N):
        x = synth.gen_scene(100 + proto, 2, [dict(proto=proto, start=4 * (800 + s), payload_seed=10 + s, amp=50),
                                             dict(proto=0, start=4 * (9000 + s), payload_seed=80 + s, amp=40)]).copy()
        x[8 * 500:8 * 800] = _carrier(200 + s, 2, 500)[8 * 500:8 * 800]
        rows.append(x)
    return _stack(rows)


@functools.lru_cache(maxsize=None)
def cut_scene():
    """Stream s: a TFA_2 burst that starts 256 - 4 s samples ahead of the boundary between blocks 1 and 2.  Its fifth edge comes
    about 125 samples into the burst and its tenth about 150 later: for 32 of the streams the boundary lies inside the phase."""
    return _stack([synth.gen_scene(300, 2, [dict(proto=1, start=4 * (BLOCK_DEC - 256 + 4 * s), payload_seed=20 + s, amp=50)])
                   for s in range(N)])


@functools.lru_cache(maxsize=None)
def handover_scene():
    """Stream s: a TFA_3 burst keyed with a deviation of 700 + 7 s Hz, 8 + 0.06 s kHz off the centre, amplitude 30 + s.  The
    TFA_3 and TX22 slicers count seven edges in the window's first 2048 samples: their phase begins near sample 1680 of the window
    and ends near 2365, behind the head's hand-over at 64 chunks (104 of the 128 windows of the two slots).  A TFA_2 burst
    follows."""
    return _stack([synth.gen_scene(400, 3, [dict(proto=2, start=4 * (1000 + s), payload_seed=3, amp=30 + s, fdev_hz=700 + 7 * s,
                                                 f0_hz=8000 + 60 * s),
                                            dict(proto=1, start=4 * 12000, payload_seed=30 + s, amp=50)]) for s in range(N)])


@functools.lru_cache(maxsize=None)
def closing_scene(at_boundary=False):
    """Stream s: a TFA_2 burst at 1000 + s that falls silent 140 + 2 s samples in, after six to eight counted edges, for 800
    samples: the window times out in the silence with the phase still running (56 streams).  A whole TFA_2 burst follows.
    at_boundary: the burst at 7664 - s instead, so that the window times out at sample 8165 + s: in the first three samples
    of block 2 for streams 27, 28 and 29 -- parts shorter than one 16-byte load -- and further into it for the 26 streams behind."""
    rows = []
    for s in range(N):
        start = 7664 - s if at_boundary else 1000 + s
        x = synth.gen_scene(500, 2, [dict(proto=1, start=4 * start, payload_seed=40 + s, amp=50),
                                     dict(proto=1, start=4 * 12000, payload_seed=50 + s, amp=50)]).copy()
        k = 8 * (start + 140 + 2 * s)
        x[k:k + 8 * 800] = 128
        rows.append(x)
    return _stack(rows)


@functools.lru_cache(maxsize=None)
def oracle_events(scene, types, *args):
    """The oracle's events of a scene, computed once per (scene, types) and shared."""
    return tuple(parity.O.process_many(scene(*args), types, THRESH, 0))


def family_rssi(e, telegram=True):
    """The raw accumulators of one stream's TFA_2-family flushes (telegram: of those that decoded)."""
    m = (e["slot"] >= 1) & (e["slot"] <= 3)
    if telegram:
        m &= e["status"] == 1
    return e["rssi_raw"][m]


def assert_phase_entered(orc):
    n = sum(1 for e in orc if np.any(family_rssi(e) != 0))
    assert n > N // 2, "%d streams flush a TFA_2-family telegram with non-zero rssi" % n


def run(iq, sizes, types, depth=api.FIFO_DEPTH):
    parts, _hosts = parity.device_parts(iq, sizes)
    with api.Receiver(N, types, THRESH, 0, max_blocks=max(sizes), all_flushes=True, max_events=1 << 16) as r:
        ev = np.concatenate(parity.run_fifo(r, parts, depth=depth))
        assert r.fm_stats()["host_mismatch"] == 0
    return ev


@pytest.mark.parametrize("types", [FAMILY, ALL], ids=["family", "all_five"])
@pytest.mark.parametrize("proto", [1, 2, 3], ids=["tfa2", "tfa3", "tx22"])
def test_phase_at_every_alignment(proto, types):
    iq, orc = alignment_scene(proto), oracle_events(alignment_scene, types, proto)
    assert_phase_entered(orc)
    # the burst's own slot: the accumulator differs from stream to stream (the phase moved), and every stream has one
    own = [family_rssi(e[e["slot"] == proto]) for e in orc]
    assert sum(1 for v in own if len(v)) > N // 2 and len({int(v[0]) for v in own if len(v)}) > N // 4
    assert parity.assert_all_streams(run(iq, [2], types), iq, types, THRESH, orc=list(orc)) > N


@pytest.mark.parametrize("depth", [1, 4])
def test_submit_cut_inside_the_phase(depth):
    """The boundary inside the phase, shown by the oracle: the burst that falls silent at the boundary flushes another non-zero
    accumulator than the whole burst does -- the phase had begun ahead of the boundary and went on behind it."""
    iq, orc = cut_scene(), oracle_events(cut_scene, FAMILY)
    assert_phase_entered(orc)
    inside = 0
    for s in range(N):
        x = iq[s].copy()
        x[api.BLOCK_BYTES:] = 128
        cut = [e[6] for e in parity.fresh_oracle(x, FAMILY, THRESH).events_full() if e[0] == 1]  # (e[6]: the raw accumulator)
        whole = family_rssi(orc[s][orc[s]["slot"] == 1], telegram=False)
        inside += int(len(cut) > 0 and len(whole) > 0 and cut[0] != 0 and cut[0] != whole[0])
    assert inside >= 8, inside
    assert parity.assert_all_streams(run(iq, [1, 1], FAMILY, depth), iq, FAMILY, THRESH, orc=list(orc)) > N


def test_head_handed_over_inside_the_phase():
    iq, orc = handover_scene(), oracle_events(handover_scene, ALL)
    assert_phase_entered(orc)
    # the weakly keyed burst's windows are longer than the head and their flushes carry an accumulator
    n = sum(1 for e in orc if np.any((e["slot"] >= 2) & (e["slot"] <= 3) & (e["status"] != 1) & (e["rssi_raw"] != 0)))
    assert n > N // 2, n
    assert parity.assert_all_streams(run(iq, [3], ALL), iq, ALL, THRESH, orc=list(orc)) > N


def test_window_closes_inside_the_phase():
    iq, orc = closing_scene(), oracle_events(closing_scene, FAMILY)
    assert_phase_entered(orc)
    # the burst that fell silent flushes too, no telegram, with an accumulator that kept growing by a hundredth per sample
    n = sum(1 for e in orc if np.any(family_rssi(e[(e["slot"] == 1) & (e["status"] != 1)], telegram=False) > (1 << 26)))
    assert n > N // 2, n
    assert parity.assert_all_streams(run(iq, [2], FAMILY), iq, FAMILY, THRESH, orc=list(orc)) > N



@pytest.mark.parametrize("depth", [1, 4])
def test_window_closes_inside_the_phase_just_behind_a_submit_cut(depth):
    """The resumed part of the window is one, two, three and more samples long, all of them in the phase."""
    iq, orc = closing_scene(True), oracle_events(closing_scene, FAMILY, True)
    assert_phase_entered(orc)
    ends = [int(e["end_sample"][(e["slot"] == 1) & (e["status"] != 1)][0]) for e in orc]
    assert {BLOCK_DEC, BLOCK_DEC + 1, BLOCK_DEC + 2} <= set(ends) and sum(1 for g in ends if g > BLOCK_DEC + 2) > N // 4, ends
    assert parity.assert_all_streams(run(iq, [1, 1], FAMILY, depth), iq, FAMILY, THRESH, orc=list(orc)) > N
