"""GPU tests of the decoders' carried state on the `frames` and `splices` families (oracle/scenes.py; the classes they hold are
measured on the CPU by tests/test_carried_cpu.py): TFA_1's shift register re-created for a window from the bits before it
(tfa1_sr_before), the rdata overlay under verdicts that read stale bytes, the TFA_2 family's polarity in ChainState, WHB's
descrambler at a window's first bit -- through the pipeline, the serial chains, the shallow layout, a stream reset and a save /
load into another context, and the host mirror decoders of tfrec_gpu.  tests/test_gpu_scenes.py runs the same families through
its per-family comparisons (every flush, the default mode, the bit log, the minted digests)."""
import json
import os

import numpy as np
import pytest

import parity
import segments
from oracle import scenes as S
from state_harness import DST, continue_in_b
from tfrec_amd import api

pytestmark = pytest.mark.gpu

TYPES = 0x2F
B = api.BLOCK_BYTES
FAMS = ("frames", "splices")


def both_families():
    rows = [r for fam in FAMS for r in S.family(fam)]
    return rows, S.render_batch(rows)


def assert_cut_claims():
    """Before the GPU is used: the submits of S.CARRIED_CUTS cut inside every inverted frame, between A and B of every stale pair
    and between the parts of every splice that is meant to lie across a cut."""
    claims = [c for fam in FAMS for c in S.carried_cut_claims(fam)]
    for name, cut, lo, hi in claims:
        assert lo < cut < hi and cut in S.carried_boundaries(), name
    names = {c[0] for c in claims}
    want = {r["name"] for r in S.family("frames") if r["name"].startswith("pol_") or "_stale_" in r["name"]}
    want |= {r["name"] for r in S.family("splices") if r["name"].endswith("_cut")}
    assert want <= names and len(want) == 12 + 5 + 7, sorted(want - names)
    return names


def run(iq, cuts, **kw):
    with api.Receiver(len(iq), TYPES, S.THRESH, 0, max_blocks=max(cuts), max_events=1 << 17, **kw) as r:
        ev = np.concatenate(parity.run_fifo(r, parity.cut(iq, cuts)))
        assert r.fm_stats()["host_mismatch"] == 0
        layout = r.layout()
    return parity.sort_events(ev), layout


@pytest.mark.parametrize("serial", [False, True], ids=["pipeline", "serial"])
@pytest.mark.parametrize("cuts", [S.CARRIED_CUTS, [S.CARRIED_BLOCKS]], ids=["cut", "one_submit"])
def test_both_families_cut_where_the_state_is_carried_and_in_one_submit(cuts, serial):
    """Every flush of both families in every field, with the submits cut where the carried state matters and with every row in
    one submit (every window but the first re-created from the windows before it)."""
    assert_cut_claims()
    rows, iq = both_families()
    ev, _ = run(iq, cuts, all_flushes=True, serial_chains=serial)
    n = 0
    for s, row in enumerate(rows):
        n += parity.assert_stream(ev, s, parity.fresh_oracle(iq[s], TYPES, S.THRESH), row["name"])
    assert n > 4 * len(rows)


def test_both_families_in_the_shallow_layout(monkeypatch):
    kw, layout, _ = parity.mode_kwargs("shallow", monkeypatch)
    rows, iq = both_families()
    ev, got = run(iq, S.CARRIED_CUTS, **kw)
    assert got == layout
    for s, row in enumerate(rows):
        parity.assert_stream(ev, s, parity.fresh_oracle(iq[s], TYPES, S.THRESH), row["name"])


# ---- reset and save / load: the rows whose telegram hangs on what the part before the cut left
CARRIED = (("frames", "tx22_stale_accept", 3, S.CUT_A), ("frames", "tx22_stale_over", 3, S.CUT_A),
           ("splices", "tfa1_split_bit5_submit_cut", 0, S.CUT_A), ("splices", "tfa1_split_empty_behind_cut", 0, S.CUT_A),
           ("splices", "tfa1_split_three_ways_submit_cut", 0, S.CUT_A),
           ("frames", "whb_stale_accept", 4, S.CUT_B), ("splices", "whb_cut_preamble_submit_cut", 4, S.CUT_B))


def carried_rows():
    by = {r["name"]: r for fam in FAMS for r in S.family(fam)}
    return [(name, slot, cut, S.render(by[name])) for _, name, slot, cut in CARRIED]


def telegrams(orc, slot, behind):
    return [e for e in orc.events_full() if e[0] == slot and e[7] == 1 and e[1] > behind]


def test_a_stream_reset_at_the_cut_drops_what_was_carried():
    """Every row twice: the even streams are reset at their row's cut, the odd ones run on.  The segment harness compares every
    stream's segments with oracles restarted where the stream was; those oracles say what the reset must do: B of a stale pair is
    rejected with nothing but zeros behind its own bytes, the split telegrams are not decoded."""
    assert_cut_claims()
    rows = carried_rows()
    iq = np.stack([x for _, _, _, x in rows for _ in (0, 1)])
    resets = {1: [2 * k for k, r in enumerate(rows) if r[2] == S.CUT_A], 2: [2 * k for k, r in enumerate(rows) if r[2] == S.CUT_B]}
    ops = {k: [("reset", v)] for k, v in resets.items()}
    with api.Receiver(len(iq), TYPES, S.THRESH, 0, max_blocks=max(S.CARRIED_CUTS), all_flushes=True) as r:
        n, segs = segments.run_segments(r, parity.cut(iq, S.CARRIED_CUTS), ops, (TYPES, S.THRESH, 0), read_between=False)
    assert n > 8 * len(rows)
    for k, (name, slot, cut, _) in enumerate(rows):
        fresh, whole = segs[2 * k][-1].orc, segs[2 * k + 1][-1].orc
        assert len(segs[2 * k]) == 2 and len(segs[2 * k + 1]) == 1
        assert telegrams(whole, slot, cut // 4), name
        if "_stale_" in name:
            b = [e for e in fresh.events_full() if e[0] == slot and e[2] > 0]
            assert len(b) == 1 and b[0][7] == 2 and not any(b[0][5][b[0][2]:]), name
        else:
            assert not telegrams(fresh, slot, 0), name


@pytest.mark.parametrize("cut", [S.CUT_A, S.CUT_B], ids=["cut_a", "cut_b"])
def test_saved_after_the_first_part_and_loaded_into_stream_64_the_telegram_is_decoded(cut):
    """Context A runs the rows up to their cut and saves; context B (65 streams) loads them, the first into stream 64, and runs the
    rest: B's events are the uninterrupted context's (continue_in_b), and they hold the telegram that hangs on the first part."""
    assert_cut_claims()
    rows = [r for r in carried_rows() if r[2] == cut]
    iq = np.stack([x for _, _, _, x in rows])
    first = cut // 32768
    parts = [np.ascontiguousarray(v) for v in parity.cut(iq, (first, S.CARRIED_BLOCKS - first))]
    orcs = [parity.fresh_oracle(x, TYPES, S.THRESH, keep_dec=True) for x in iq]
    for (name, slot, _, _), o in zip(rows, orcs):  # the row's own chain has no window open at the cut
        trig = S.trigger_samples(o.dec())
        assert not ((trig >= cut // 4 - S.WINDOW[slot]) & (trig < cut // 4)).any(), name
    ev_a, got, *_ = continue_in_b(parts, lambda n: api.Receiver(n, TYPES, S.THRESH, 0, max_blocks=max(first, S.CARRIED_BLOCKS - first),
                                                                 all_flushes=True))
    assert DST[0] == 64
    both = np.concatenate([ev_a, got])
    for k, (name, slot, _, _) in enumerate(rows):
        parity.assert_segment(both, k, orcs[k], name)
        tel = telegrams(orcs[k], slot, cut // 4)
        assert tel and [e for e in api.event_tuples_full(got, k) if e[0] == slot and e[7] == 1 and e[5] == tel[0][5]], name


def test_cli_prints_the_golden_text_of_the_frames_rows(tmp_path, golden_dir):
    """tfrec_gpu over the frames rows as dump files, two blocks a batch: the host mirror decoders' verdicts on the events' bytes,
    the stale-accepted telegrams included, against the real reference's text (tests/golden/scenes.json) without store_bit's own
    `Inverted SYNC` lines.  (The files' lines come in the engine's order: compared as a multiset.)"""
    cases = [c for c in json.load(open(os.path.join(golden_dir, "scenes.json")))["cases"] if c["family"] == "frames"]
    assert len(cases) == len(S.family("frames"))
    parity.build_cli()
    args, want = ["-T", "2f", "-t", str(S.THRESH), "-b", "2"], []
    for k, c in enumerate(cases):
        p = tmp_path / ("f%02d.iq" % k)
        S.render(c["spec"]).tofile(p)
        args += ["-L", str(p)]
        want += [ln for ln in c["text"].splitlines() if ln.strip() and ln != "Inverted SYNC"]
    assert sum(1 for ln in want if ln.startswith("TX22 ID 30000090")) == 2 and any(ln.startswith("WHB02 ID 2a5c3ffffff") for ln in want)
    got = [ln for ln in parity.cli_stdout(args, timeout=120).splitlines() if ln.strip() and not ln.startswith("WHB: Samples")]
    assert sorted(got) == sorted(want)
