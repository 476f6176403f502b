"""GPU tests on the scene families (oracle/scenes.py): dense windows, block and submit edges, repeated frames, colliding
protocols, bit clock offsets, signal levels, hand-built frames and spliced bursts through the HIP path, event by event against the oracle -- and the scenes the
real reference pinned (tests/golden/scenes.json), plus the reference-minted IQ fixtures, against the golden outputs
directly, with no oracle in between."""
import hashlib
import json
import os

import numpy as np
import pytest

import parity
from oracle import scenes as S
from tfrec_amd import api, synth

pytestmark = pytest.mark.gpu

# submit cuts per family (blocks); tests/test_scenes_cpu.py checked the tables for exactly these
CUTS = dict(dense=[24], edges=[1, 2, 5, 4], repeats=[24], collisions=[7, 25], drift=[32], levels=[16],
            frames=S.CARRIED_CUTS, splices=S.CARRIED_CUTS)  # (the last two: inside inverted frames, stale pairs and splices)
# fallbacks each family reaches in the pipeline (stats() counters, observed on an MI355X for these fixed inputs; only "> 0"
# is asserted -- how the work is split is not part of the contract)
REACHES = dict(dense=["tfa2_resliced", "tfa1_scalar_groups"], edges=["biquad_unconverged"],
               repeats=["tfa2_resliced", "tfa2_scalar_groups"], collisions=["tfa2_scalar_groups", "biquad_unconverged"],
               drift=["tfa2_scalar_groups", "biquad_unconverged"], levels=["tfa2_scalar_groups"], frames=[], splices=[])


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _run(iq, cuts, thresh=500, wide=0, **kw):
    """Submit the batch cut into `cuts` blocks, up to four submits in flight, and drain; events in per-(stream, slot) order
    plus the context's counters."""
    with api.Receiver(len(iq), 0x2F, thresh, wide, max_blocks=max(cuts), max_events=1 << 18, **kw) as r:
        ev = np.concatenate(parity.run_fifo(r, parity.cut(iq, cuts)))
        stats, fm = r.stats(), r.fm_stats()
    return (ev if kw.get("bits") else parity.sort_events(ev)), stats, fm


def _oracles(iq, thresh=500, wide=0, log_bits=False):
    return [parity.fresh_oracle(row, 0x2F, thresh, wide, log_bits=log_bits) for row in iq]


def _family(fam):
    rows = S.family(fam)
    return rows, S.render_batch(rows)


SERIAL = pytest.mark.parametrize("serial", [False, True], ids=["pipeline", "serial"])


@SERIAL
def test_dense_windows_fill_the_window_table(serial):
    """Combs at W-2 .. W+2 of every chain in one 24-block submit: every flush equals the oracle's, and the TFA_2 chain's
    window count comes within 2 % of T.cap = M / 356 + 2 (the test reaches the bound it guards)."""
    rows, iq = _family("dense")
    m = 24 * S.BLOCK_DEC
    cap = m // 356 + 2
    ev, st, fm = _run(iq, CUTS["dense"], all_flushes=True, serial_chains=serial)
    orcs = _oracles(iq)
    for s, row in enumerate(rows):
        parity.assert_stream(ev, s, orcs[s], row["name"])
    per_chain = {slot: max(int(np.sum((ev["stream"] == s) & (ev["slot"] == slot))) for s in range(len(rows)))
                 for slot in range(4)}
    assert per_chain[1] >= 0.98 * cap, per_chain
    assert per_chain[0] >= m // 400 - 1 and per_chain[2] >= m // 640 - 1 and per_chain[3] >= m // 694 - 1, per_chain
    assert fm["host_mismatch"] == 0
    if not serial:
        assert all(st[k] > 0 for k in REACHES["dense"]), st


@pytest.mark.parametrize("fam", ["edges", "repeats", "collisions", "drift", "levels", "frames", "splices"])
@SERIAL
def test_scene_family_all_flushes(fam, serial):
    rows, iq = _family(fam)
    ev, st, fm = _run(iq, CUTS[fam], all_flushes=True, serial_chains=serial)
    orcs = _oracles(iq)
    total = sum(parity.assert_stream(ev, s, orcs[s], row["name"]) for s, row in enumerate(rows))
    assert total > len(rows)
    assert fm["host_mismatch"] == 0
    if not serial:
        assert all(st[k] > 0 for k in REACHES[fam]), st


@pytest.mark.parametrize("fam", ["dense", "edges", "repeats", "collisions", "drift", "levels", "frames", "splices"])
def test_scene_family_default_mode(fam):
    rows, iq = _family(fam)
    ev, st, fm = _run(iq, CUTS[fam])
    orcs = _oracles(iq)
    for s, row in enumerate(rows):
        parity.assert_stream(ev, s, orcs[s], row["name"], default_mode=True)
        n_ok = int(np.sum((ev["stream"] == s) & (ev["status"] == 1)))
        lines = [ln for ln in orcs[s].text().splitlines() if not ln.startswith("Inverted") and not ln.startswith("WHB:")]
        assert n_ok == len(lines), row["name"]
    assert fm["host_mismatch"] == 0


@pytest.mark.parametrize("thresh,wide", [(0, 0), (500, 1)], ids=["auto_thresh", "wide"])
def test_levels_with_auto_threshold_and_wide_filter(thresh, wide):
    rows, iq = _family("levels")
    ev, st, fm = _run(iq, [5, 11], thresh=thresh, wide=wide, all_flushes=True)
    orcs = _oracles(iq, thresh, wide)
    for s, row in enumerate(rows):
        parity.assert_stream(ev, s, orcs[s], row["name"])
    assert fm["host_mismatch"] == 0


@pytest.mark.parametrize("fam", ["repeats", "collisions", "drift", "frames", "splices"])
def test_scene_bits_equal_the_oracle_flush_by_flush(fam):
    """TFREC_AMD_F_BITS on the scenes with several frames per window, interference and bit clock offsets: every bit handed to
    decoder::store_bit, flush by flush, against Oracle(log_bits=True).bits_text()."""
    rows, iq = _family(fam)
    ev, st, fm = _run(iq, CUTS[fam], all_flushes=True, bits=True)
    orcs = _oracles(iq, log_bits=True)
    n_bits = 0
    for s, row in enumerate(rows):
        n_bits += parity.assert_bits(ev, s, orcs[s], row["name"])
    assert n_bits > 1000 * len(rows)


def test_minted_scenes_equal_the_reference_directly(golden_dir):
    """Every scene the real reference pinned, through the HIP path, against the golden events (no oracle in between); the
    per-event verdict against the reference's telegram lines."""
    cases = json.load(open(os.path.join(golden_dir, "scenes.json")))["cases"]
    groups = {}
    for c in cases:
        groups.setdefault((c["spec"]["n_blocks"], c["types"], c["thresh"], c["wide"]), []).append(c)
    for (n_blocks, types, thresh, wide), cs in sorted(groups.items()):
        iq = np.stack([S.render(c["spec"]) for c in cs])
        for row, c in zip(iq, cs):
            assert _sha(row) == c["iq_sha256"], c["spec"]["name"]
        sizes = [n_blocks // 2, n_blocks - n_blocks // 2] if n_blocks > 1 else [1]
        with api.Receiver(len(cs), types, thresh, wide, max_blocks=max(sizes), all_flushes=True, max_events=1 << 17) as r:
            ev = parity.sort_events(np.concatenate(parity.run_fifo(r, parity.cut(iq, sizes), depth=1)))
            assert r.fm_stats()["host_mismatch"] == 0
        for s, c in enumerate(cs):
            full = api.event_tuples_full(ev, s)
            name = c["spec"]["name"]
            assert S.flush_counts(full) == c["flushes"], name
            assert S.events_digest([e[:6] for e in full]) == c["events_sha256"], name
            parity.status_pinned_by_text(full, c["text"], name)


def _golden_events(ev, s, golden_events, text, name):
    full = api.event_tuples_full(ev, s)
    want = [(e[0], e[1], e[2], e[3], e[4], bytes.fromhex(e[5])) for e in golden_events]
    assert sorted(e[:6] for e in full) == sorted(want), name
    parity.status_pinned_by_text(full, text, name)


@pytest.mark.parametrize("name", ["tfa_1", "tfa_2", "tfa_3", "tx22", "whb"])
def test_raw_iq_fixture_through_the_hip_path(golden_dir, name):
    z = np.load(os.path.join(golden_dir, "iq_%s.npz" % name))
    meta = json.loads(str(z["meta"]))
    iq = z["iq"]
    nb = iq.size // 65536
    with api.Receiver(1, meta["types"], meta["thresh"], meta["wide"], max_blocks=nb, all_flushes=True) as r:
        r.submit(iq.reshape(1, -1))
        ev = r.drain()
        assert np.array_equal(r.decimated(0, nb * S.BLOCK_DEC), z["dec"])
        assert r.fm_stats()["host_mismatch"] == 0
    _golden_events(ev, 0, meta["events"], meta["text"], name)


def test_config5_cases_through_the_hip_path(golden_dir):
    """BASELINE config 5 (15.36 MS/s input, input_10x): the 10:1 stage's output, the decimated samples and the events, against
    the hashes and the real reference's events in config5.json."""
    for c in json.load(open(os.path.join(golden_dir, "config5.json")))["cases"]:
        iq = synth.gen_stream(c["seed"], c["stream"], c["n_blocks"], c["proto_mask"], c["noise_q8"], rate_mult=10)
        assert _sha(iq) == c["iq_sha256"]
        nb = c["n_blocks"]
        with api.Receiver(1, c["types"], c["thresh"], c["wide"], max_blocks=nb, all_flushes=True, input_10x=True) as r:
            r.submit(iq.reshape(1, -1))
            ev = r.drain()
            assert _sha(r.stage0(0, nb * 32768)) == c["stage0_sha256"]
            assert _sha(r.decimated(0, nb * S.BLOCK_DEC)) == c["dec_sha256"]
            assert r.fm_stats()["host_mismatch"] == 0
        _golden_events(ev, 0, c["events"], c["text"], "config5 seed %d stream %d" % (c["seed"], c["stream"]))
