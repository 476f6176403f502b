"""CPU tests of the scene families (oracle/scenes.py): the generator's bytes and the oracle against the real reference's
outputs pinned in tests/golden/scenes.json, and proof that each scene builds what it claims -- triggers on the intended
decimated samples, windows packed as densely as the device tables are sized for, and no table asked for more than
capi.hip gives it."""
import hashlib
import json
import os

import numpy as np
import pytest

from oracle import oracle as O
from oracle import scenes as S
from tfrec_amd import synth

import parity
from parity import golden_data, sha256_of


@pytest.fixture(scope="module")
def cases(golden_dir):
    return json.load(open(os.path.join(golden_dir, "scenes.json")))["cases"]


def test_scene_goldens_cover_every_family_and_protocol(cases):
    fams = {c["family"] for c in cases}
    assert fams == set(S.FAMILIES)
    for fam in ("repeats", "collisions", "drift", "levels"):
        text = "".join(c["text"] for c in cases if c["family"] == fam)
        for slot, p in parity.PREFIX.items():
            assert any(ln.startswith(p) and not ln.startswith("WHB:") for ln in text.splitlines()), (fam, p)
    assert any(c["thresh"] == 0 for c in cases) and any(c["wide"] == 1 for c in cases)


def test_scenes_against_reference_outputs(cases):
    for c in cases:
        tag = c["spec"]["name"]
        iq = S.render(c["spec"])
        assert sha256_of(iq) == c["iq_sha256"], "generator drifted: " + tag
        o = O.Oracle(c["types"], c["thresh"], c["wide"], log_bits=True, keep_dec=True)
        o.process(iq)
        assert sha256_of(o.dec()) == c["dec_sha256"], tag
        assert S.flush_counts(o.events()) == c["flushes"], tag
        assert S.events_digest(o.events()) == c["events_sha256"], tag
        assert o.data() == golden_data(c["data"]), tag
        assert o.text() == c["text"], tag
        assert hashlib.sha256(o.bits_text().encode()).hexdigest() == c["bits_sha256"], tag
        parity.status_pinned_by_text(o.events_full(), c["text"], tag)


def test_repeats_put_several_frames_in_one_window(cases):
    """The repeats a window apart: one flush although the window held 3 copies (the decoder re-synced while synced); the
    split ones decode every copy; the tight ones hand all their copies' bits to store_bit before one flush."""
    by = {c["spec"]["name"]: c for c in cases}
    for proto in range(5):
        name = synth.PROTO_NAMES[proto].lower()
        one, split = by["repeat_%s_one_window" % name], by["repeat_%s_split" % name]
        assert one["flushes"][proto] == 1
        assert len([ln for ln in split["text"].splitlines() if ln.startswith(parity.PREFIX[proto])]) == 3
    for name in ("repeat_whb_tight", "repeat_tfa1_tight", "repeat_tx22_tight"):
        o = O.Oracle(0x2F, 500, 0, log_bits=True)
        o.process(S.render(by[name]["spec"]))  # (the bit log itself is pinned by test_scenes_against_reference_outputs)
        assert max(int(ln.split()[2]) for ln in o.bits_text().splitlines()) > 900


def test_scene_generator_keeps_the_burst_model():
    """gen_scene's truth records: one per copy, copies repeat_gap apart, lengths from the (offset) bit clock."""
    iq, tr = synth.gen_scene(5, 8, [dict(proto=1, start=1000, payload_seed=3, repeats=3, repeat_gap=777, baud_ppm=20000),
                                    dict(proto=0, start=2000, payload_seed=4, amp=30)], with_truth=True)
    assert [t["proto"] for t in tr] == [1, 1, 1, 0]
    assert tr[0]["frame"] == tr[1]["frame"] == tr[2]["frame"]
    n = synth.burst_length(1, len(tr[0]["frame"]), 20000)
    assert [t["length"] for t in tr[:3]] == [n] * 3 and n < synth.burst_length(1, len(tr[0]["frame"]))
    assert [t["start"] for t in tr[:3]] == [1000, 1000 + n + 777, 1000 + 2 * (n + 777)]
    # overlapping bursts add before the clip: two full-scale carriers on top of each other saturate the bytes
    loud = synth.gen_scene(5, 1, [dict(proto=1, start=0, payload_seed=3, amp=100), dict(proto=1, start=0, payload_seed=3, amp=100)],
                           noise_q8=0)
    assert loud[:4000].min() == 0 and loud[:4000].max() == 255
    # a copy that would run past the end is left out, an explicit frame is sent as given
    _, tr = synth.gen_scene(1, 1, [dict(proto=2, start=30000, frame=b"\x2d\xd4\x90\x12\x34\x56\x78")], with_truth=True)
    assert tr == []
    _, tr = synth.gen_scene(1, 1, [dict(proto=2, start=100, frame=b"\x2d\xd4\x90\x12\x34\x56\x78")], with_truth=True)
    assert tr[0]["frame"] == b"\x2d\xd4\x90\x12\x34\x56\x78"


def _triggers(iq, thresh=S.THRESH, wide=0):
    o = O.Oracle(0x2F, thresh, wide, keep_dec=True, log_bits=True)
    o.process(iq)
    return o, S.trigger_samples(o.dec(), thresh)


@pytest.mark.parametrize("fam", ["dense", "edges"])
def test_combs_trigger_exactly_where_intended(fam):
    for row in S.family(fam):
        o, trig = _triggers(S.render(row))
        f = S.pulse(row["pulse"])[1]
        want = np.sort(np.concatenate([t - f + S.pulse_triggers(row["pulse"]) for t in S.comb_firsts(row)]))
        assert np.array_equal(trig, want), row["name"]
        if row["pulse"] == "dot":
            assert len(trig) == len(S.comb_firsts(row)), row["name"]  # one trigger sample per pulse


def test_edge_triggers_sit_on_block_and_submit_boundaries():
    rows = {r["name"]: r for r in S.family("edges")}
    for off in (0, 1, 2):
        _, trig = _triggers(S.render(rows["edge_dot_block_sample%d" % off]))
        assert sorted(set((trig % S.BLOCK_DEC).tolist())) == [off]
    _, trig = _triggers(S.render(rows["edge_dot_block_last"]))
    assert sorted(set((trig % S.BLOCK_DEC).tolist())) == [S.BLOCK_DEC - 1] and trig[-1] == 12 * S.BLOCK_DEC - 1


def test_dense_windows_reach_the_table_bound():
    """One 24-block submit: each chain's window count from the oracle's flushes (the model of windows() checked against
    them), and the TFA_2 chain within 2 % of T.cap = M / 356 + 2."""
    m = 24 * S.BLOCK_DEC
    cap = S.table_sizes(m)["cap"]
    reached = {}
    for row in S.family("dense"):
        o, trig = _triggers(S.render(row))
        ev = o.events_full()
        for slot in range(4):  # (an empty WHB window ends without a flush: whb.cpp flushes only what it synced on)
            wins = S.windows(trig, S.WINDOW[slot])
            assert sum(1 for w in wins if w[1] < m) == sum(1 for e in ev if e[0] == slot), (row["name"], slot)
        for slot in range(5):
            reached[slot] = max(reached.get(slot, 0), len(S.windows(trig, S.WINDOW[slot])))
        if row["name"] == "dense_w356_exact":
            assert sum(1 for e in ev if e[0] == 1) >= 0.98 * m / 356
    assert reached[1] >= 0.98 * cap and reached[1] <= cap
    for slot, w in S.WINDOW.items():
        assert reached[slot] >= m // w, slot  # every chain at its own tightest packing


FAMILY_SUBMITS = dict(dense=[24], edges=[1, 2, 5, 4], repeats=[24], collisions=[7, 25], drift=[32], levels=[16],
                      frames=S.CARRIED_CUTS, splices=S.CARRIED_CUTS)


@pytest.mark.parametrize("fam", sorted(S.FAMILIES))
def test_no_scene_needs_more_than_the_tables_hold(fam):
    """Before any of it runs on a GPU: windows, window-relative slots, bit words and WHB step records each chain needs in
    the submits tests/test_gpu_scenes.py cuts the family into, against capi.hip's formulas for that submit size."""
    cuts = FAMILY_SUBMITS[fam]
    m = max(cuts) * S.BLOCK_DEC
    size = S.table_sizes(m)
    for row in S.family(fam):
        o, trig = _triggers(S.render(row))
        nbits = {}
        for ln in o.bits_text().splitlines():
            p = ln.split()
            nbits.setdefault(int(p[1]), []).append(int(p[2]))
        for slot, w in S.WINDOW.items():
            wins = S.windows(trig, w)
            per = nbits.get(slot, []) if slot < 4 else None
            if per is not None:
                per = per + [0] * (len(wins) - len(per))
            bounds = np.cumsum([0] + cuts) * S.BLOCK_DEC
            for lo, hi in zip(bounds, bounds[1:]):
                sub = [(a - lo, b - lo) for a, b in wins]
                need = S.table_demand(sub, hi - lo, 1, bits_per_window=per)
                assert need["windows"] <= size["cap"], (row["name"], slot)
                assert need["slots"] <= size["slots"], (row["name"], slot, need, size)
                if per is not None:
                    assert need["bit_words"] <= size["bit_words"], (row["name"], slot, need, size)
                if slot == 4:
                    assert need["whbrec"] <= size["whbrec"], (row["name"], need, size)
