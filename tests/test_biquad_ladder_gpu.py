"""The biquad passes' second repair (K3b') and serial repair (K3c, fix_chain) on the GPU.  At the product's 256-slot segments no
ordinary input gets past the first repair, so these tests run the short-segment build of the library (16 slots:
api.Receiver(..., short_segments=True)) on the frozen inputs of tests/ladder_model.py, for which the model says that every chain
goes through every rung (tests/test_biquad_ladder_cpu.py).  Checked: every flush event (and bit) against the oracle, every
in-window biquad output against the model's true trajectory (Receiver.biquad_row; a failure names chain, window, slot and the
rung that wrote the slot last), and the four biquad counters of stats() against the model's census -- they are deterministic
functions of the input."""
import numpy as np
import pytest

import ladder_model as LM
import parity
import segments
from oracle import oracle as O
from tfrec_amd import api

pytestmark = pytest.mark.gpu

TYPES, THRESH = 0x2F, LM.THRESH
COUNTERS = tuple(LM.STATS)


@pytest.fixture(scope="module")
def iq():
    return LM.frozen_batch()


@pytest.fixture(scope="module")
def orc(iq):
    """The oracle's events of every row, every type (read-only; shared by the cases)."""
    return O.process_many(iq, TYPES, THRESH)


def _counters(r):
    st = r.stats()
    return {k: st[k] for k in COUNTERS}


def _check_rows(r, models, k, streams=None, ks=None):
    """biquad_row of every chain of the streams against submit k of their models (ks: the models' own submit index per stream)."""
    n = 0
    for s in (range(len(models)) if streams is None else streams):
        for slot, chain in models[s].items():
            res = chain[k if ks is None else ks[s]]
            got = r.biquad_row(slot, s)
            assert len(got) == len(res.true_row), (len(got), len(res.true_row))
            diff = res.first_difference(got)
            assert diff is None, "stream %d: %s" % (s, diff)
            n += len(res.index)
    return n


def _run(iq, cuts, models, depth, **kw):
    """A receiver over iq cut into `cuts`.  depth 1: submit and drain in turn, and after every drain every biquad row against the
    models.  -> (the drained events, counters, fm_stats, in-window outputs compared)."""
    parts = parity.cut(iq, cuts)
    kw = dict(dict(all_flushes=True, max_events=1 << 16, short_segments=True), **kw)
    n = 0
    with api.Receiver(len(iq), kw.pop("types", TYPES), THRESH, 0, max_blocks=max(cuts), **kw) as r:
        if depth == 1:
            evs = []
            for k, p in enumerate(parts):
                r.submit(p)
                evs.append(r.drain())
                n += _check_rows(r, models, k)
        else:
            evs = parity.run_fifo(r, parts, depth=depth)
        return np.concatenate(evs), _counters(r), r.fm_stats(), n


def test_every_rung_events_rows_and_counters(iq, orc):
    """The main case: every type, submits of 1, 3 and 2 blocks -- submit and drain in turn with the rows read after every drain
    (first: a wrong sample is named by chain, window, slot and rung), then all in flight at once."""
    models = LM.frozen_models(16)
    want = LM.expected_stats(models)
    assert want["biquad_serial"] > 1000 and want["biquad_unconverged"] > want["biquad_serial"]
    for depth in (1, api.FIFO_DEPTH):
        ev, got, fm, n = _run(iq, LM.CUTS, models, depth)
        assert n == (depth == 1) * sum(len(res.index) for m in models for chain in m.values() for res in chain)
        assert parity.assert_all_streams(ev, iq, TYPES, THRESH, orc=orc) == sum(len(e) for e in orc) > 500
        assert fm["host_mismatch"] == 0
        assert got["biquad_serial"] > 0
        assert got == want, (depth, got, want)
    assert sum(len(res.index) for m in models for chain in m.values() for res in chain) > 10 * 4 * 6 * 8000


def test_bits_mode(iq):
    """TFREC_AMD_F_BITS: every bit handed to decoder::store_bit, flush by flush -- the slicers read the rows the repairs wrote."""
    ev, _, _, _ = _run(iq, LM.CUTS, None, api.FIFO_DEPTH, bits=True, max_events=1 << 18)
    n_bits = 0
    for s in range(len(iq)):
        o = parity.fresh_oracle(iq[s], TYPES, THRESH, log_bits=True)
        parity.assert_stream(ev, s, o)
        n_bits += parity.assert_bits(ev, s, o, "stream %d" % s)
    assert n_bits > 20000


def test_both_layouts(iq, orc, monkeypatch):
    """The shallow layout (TFREC_AMD_DEEP=0) and the deep one: byte-identical events, the oracle's."""
    got = {}
    for deep in ("1", "0"):
        monkeypatch.setenv("TFREC_AMD_DEEP", deep)
        with api.Receiver(len(iq), TYPES, THRESH, 0, max_blocks=max(LM.CUTS), all_flushes=True, max_events=1 << 16,
                          short_segments=True) as r:
            assert r.layout() == (6 if deep == "1" else 4)
            got[deep] = parity.sort_events(np.concatenate(parity.run_fifo(r, parity.cut(iq, LM.CUTS))))
    assert got["1"].tobytes() == got["0"].tobytes()
    assert parity.assert_all_streams(got["0"], iq, TYPES, THRESH, orc=orc) == sum(len(e) for e in orc) > 500


@pytest.mark.parametrize("max_blocks", [1, 6])
@pytest.mark.parametrize("types", [0x20, 0x04])
def test_one_chain_at_the_bound_of_the_item_area(iq, types, max_blocks):
    """ONE biquad chain registered and always-triggered rows: a chain's segments fill the most of its queue's item area (cap =
    m / 356 + 2 items per chain: 25 for one block, where a row has 16 segments of 16 slots; csrc/tfrec_dev.h derives the bound)."""
    rows = np.ascontiguousarray(iq[list(LM.ALWAYS_TRIGGERED)])
    cuts = (1, 1, 1) if max_blocks == 1 else (6,)
    rows = rows[:, :sum(cuts) * api.BLOCK_BYTES]
    _, decs, _ = LM.frozen_oracles()
    models = [LM.run_stream(decs[s][:2 * sum(cuts) * api.BLOCK_DEC], cuts, types, THRESH, 16) for s in LM.ALWAYS_TRIGGERED]
    for m in models:
        for chain in m.values():
            assert all(16 * c - 3 <= res.census["segments"] <= 16 * c for res, c in zip(chain, cuts))
    want = LM.expected_stats(models)
    assert want["biquad_serial"] > 0
    ev, got, fm, n = _run(rows, cuts, models, 1, types=types)
    parity.assert_all_streams(ev, rows, types, THRESH)
    assert got == want, (got, want)
    assert n == sum(len(res.index) for m in models for chain in m.values() for res in chain) > len(rows) * sum(cuts) * 8000


def test_carried_state_from_the_serial_repair(iq, orc):
    """One-block submits throughout: segment 0 of every submit starts from a state the chain walk -- often its serial repair --
    produced."""
    cuts = (1,) * LM.N_BLOCKS
    models = LM.frozen_models(16, TYPES, cuts)
    ev, got, fm, n = _run(iq, cuts, models, 1)
    assert parity.assert_all_streams(ev, iq, TYPES, THRESH, orc=orc) == sum(len(e) for e in orc) > 500
    assert fm["host_mismatch"] == 0
    assert got == LM.expected_stats(models) and got["biquad_serial"] > 1000
    assert n > 10 * 4 * 6 * 8000


def test_whb_redo_reads_repaired_rows(iq, orc, monkeypatch):
    """TFREC_AMD_WHB_FORCE_FAIL=2: every second (stream + submit) is demodulated again by the exact kernel, from dev32 rows that
    the serial repair wrote."""
    monkeypatch.setenv("TFREC_AMD_WHB_FORCE_FAIL", "2")
    with api.Receiver(len(iq), TYPES, THRESH, 0, max_blocks=max(LM.CUTS), all_flushes=True, max_events=1 << 16,
                      short_segments=True) as r:
        ev = np.concatenate(parity.run_fifo(r, parity.cut(iq, LM.CUTS)))
        assert r.stats()["whb_respeculated"] >= len(iq) * len(LM.CUTS) // 4
    assert not (ev["status"] == 0xFF).any()
    assert parity.assert_all_streams(ev, iq, TYPES, THRESH, orc=orc) == sum(len(e) for e in orc) > 500


def test_reset_restarts_the_carried_state(iq):
    """Streams reset between submits: their biquad chains restart from the zero state (and a zero previous sample), the segments'
    oracles agree, and the rows of the last submit equal the model's -- the untouched streams' as well as the restarted ones'."""
    reset = {1: [1, 9, 13], 2: [13, 4]}
    parts = parity.cut(iq, LM.CUTS)
    with api.Receiver(len(iq), TYPES, THRESH, 0, max_blocks=max(LM.CUTS), all_flushes=True, max_events=1 << 16,
                      short_segments=True) as r:
        total, segs = segments.run_segments(r, parts, {k: [("reset", v)] for k, v in reset.items()}, (TYPES, THRESH, 0))
        assert total > 500
        last = len(LM.CUTS) - 1
        touched = sorted({s for v in reset.values() for s in v})
        models, ks = LM.frozen_models(16), {}
        restarted = list(models)
        for s in touched:
            g = segs[s][-1]
            restarted[s] = LM.run_stream(g.orc.dec(), LM.CUTS[g.k:], TYPES, THRESH, 16, max_blocks=max(LM.CUTS))
            ks[s] = last - g.k
        assert _check_rows(r, models, last, [s for s in range(len(iq)) if s not in touched]) > 0
        assert _check_rows(r, restarted, last, touched, ks) > 0


def test_product_segment_length(iq, orc):
    """The same inputs on the product library (256 slots): events, rows and counters against the model at 256 slots -- the model
    and the geometry checked independently of the short-segment build."""
    models = LM.frozen_models(256)
    ev, got, fm, n = _run(iq, LM.CUTS, models, 1, short_segments=False)
    assert parity.assert_all_streams(ev, iq, TYPES, THRESH, orc=orc) == sum(len(e) for e in orc) > 500
    assert fm["host_mismatch"] == 0
    assert got == LM.expected_stats(models), (got, LM.expected_stats(models))


def test_biquad_row_refuses_what_has_no_row(iq):
    """TFREC_AMD_E_INVAL: before the first drain, TFA_1, a slot outside the context's types, a stream outside the context, a
    serial_chains context."""
    part = np.ascontiguousarray(iq[:2, :api.BLOCK_BYTES])
    for kw in ({}, {"serial_chains": True}):
        with api.Receiver(2, 0x22, THRESH, 0, max_blocks=1, all_flushes=True, **kw) as r:
            with pytest.raises(api.TfrecAmdError):
                r.biquad_row(1, 0)
            r.submit(part)
            r.drain()
            for slot, stream in ((0, 0), (2, 0), (5, 0), (-1, 0), (1, 2), (1, -1)) + (((1, 0), (4, 1)) if kw else ()):
                with pytest.raises(api.TfrecAmdError) as e:
                    r.biquad_row(slot, stream)
                assert e.value.code == api.E_INVAL
            if not kw:
                assert len(r.biquad_row(1, 0)) == len(r.biquad_row(4, 1)) == 32 * LM.S.table_sizes(api.BLOCK_DEC)["slots"]
