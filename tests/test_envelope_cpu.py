"""The burst envelope without a GPU (tfrec_amd_enable_burst_envelope, tfrec_gpu -Q): the restatement
tfrec_amd/envelope.py against its per-sample form, the gaps at the mask's word boundaries, across a block boundary and across a submit
cut, the behaviour under cutting, the summary's conditions and its 128-bit product, tfrec_gpu's merge (tfrec_amd/host/job.h, compiled
into a stand-alone program under the address and undefined-behaviour sanitizers), the struct and the exports, and what tfrec_gpu
decides before it opens a device.

Everything is an exact integer; nothing here has a tolerance."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import parity
from recorder_rows import rec_line
from tfrec_amd import api, capture, envelope, levels
from meter_rows import crafted_dec

B = levels.BLOCK_DEC
GOLDEN = ("tfa_1", "tfa_2", "tfa_3", "tx22", "whb")
ZERO = [np.zeros(2, dtype=np.int16)]
W = max(levels.windows(0x2F))  # 694
CONT, OPEN = capture.RUN_CONTINUES, capture.RUN_OPEN


def golden_dec(name):
    return np.load(os.path.join(parity.ROOT, "tests", "golden", "iq_%s.npz" % name))["dec"]


def records(dec, types=0x2F, thresh=500, state=None, prev=ZERO, base=0):
    """One submit of one stream -> (records, runs, thresholds, state); state: (the recorder's, the threshold's)."""
    cs, ts = state if state is not None else (None, None)
    runs, _, cs = capture.captures(dec, types, thresh, cs)
    thr, ts = envelope.thresholds(dec, types, thresh, ts)
    return envelope.envelopes([dec], [thr], runs, prev, base=[base]), runs, thr, (cs, ts)


def submits(dec, sizes, types=0x2F, thresh=500):
    """The stream cut into submits of `sizes` blocks -> the submits' records."""
    st, prev, pos, out = None, ZERO, 0, []
    for nb in sizes:
        part = dec[2 * pos * B:2 * (pos + nb) * B]
        recs, _, _, st = records(part, types, thresh, st, prev, pos * B)
        out.append(recs)
        prev, pos = [part.reshape(-1, 2)[-1]], pos + nb
    return out


def same(a, b):
    assert a.dtype == b.dtype == envelope.ENVELOPE_DTYPE and a.tobytes() == b.tobytes()


def same_chains(got, want, label=""):
    key = lambda r: (int(r["stream"]), int(r["start_sample"]))  # noqa: E731
    got, want = sorted(got, key=key), sorted(want, key=key)
    assert len(got) == len(want), label
    for a, b in zip(got, want):
        assert a.tobytes() == b.tobytes(), (label, key(a), a, b)


def craft(n_blocks, overs, seed=1):
    """Quiet noise (pwr <= 80) with loud samples (pwr 6000) at `overs` -> int16 [2 M]."""
    dec = np.random.default_rng(seed).integers(-40, 41, size=(n_blocks * B, 2)).astype(np.int16)
    for p in overs:
        dec[p] = (3000, -3000)
    return dec.reshape(-1)


# ---- the restatement against its per-sample form
@pytest.mark.parametrize("types,thresh", [(0x2F, 500), (0x02, 0), (0x01, 60)])
def test_the_vectorised_form_equals_the_per_sample_one_on_crafted_samples(types, thresh):
    dec, _ = crafted_dec(max(levels.windows(types)), types)
    dec = dec.reshape(-1)
    recs, runs, thr, _ = records(dec, types, thresh)
    same(recs, envelope.envelopes_bruteforce([dec], [thr], runs, ZERO))
    # the bits themselves in place of the thresholds
    over = np.abs(dec.reshape(-1, 2).astype(np.int64)).sum(axis=1) > thr
    same(recs, envelope.envelopes([dec], [over], runs, ZERO))
    same(recs, envelope.envelopes_bruteforce([dec], [over], runs, ZERO))
    assert (recs["n_over"] >= 1).all() and (recs["lead_not_over"] == 0).all()  # no CONTINUES here: a run starts at an over sample
    if thresh == 60:  # the noise itself (pwr <= 80) crosses the threshold: one open run full of gaps
        assert len(runs) == 1 and recs[0]["flags"] == OPEN and recs[0]["n_gaps"] > 1000 and 1 <= recs[0]["max_gap"] < 400
        return
    assert len(runs) >= 4
    closed = (recs["flags"] & OPEN) == 0  # a run ends with the trigger's hold: W - 1 samples behind its last over sample
    assert closed.any() and (recs["last_over"][closed] + max(levels.windows(types)) == recs["n_samples"][closed]).all()


@pytest.mark.parametrize("name", GOLDEN)
def test_the_vectorised_form_equals_the_per_sample_one_on_the_golden_scenes(name):
    dec = golden_dec(name)
    recs, runs, thr, _ = records(dec)
    assert len(runs) >= 1
    same(recs, envelope.envelopes_bruteforce([dec], [thr], runs, ZERO))


@pytest.mark.parametrize("name", GOLDEN)
def test_every_golden_scene_has_a_burst_with_a_whole_tail_and_a_ratio(name):
    """What the golden scene tests here and on the GPU rely on: a chain whose tail is the trigger's whole hold, W - 1 samples for
    the largest registered window, and whose ratio_c is defined."""
    ch = envelope.chains([records(golden_dec(name))[0]])
    good = [c for c in ch if envelope.summary(c)[1] == W - 1 and envelope.summary(c)[2] is not None]
    assert len(good) >= 1
    for c in good:
        length, n_tail, ratio, snr = envelope.summary(c)
        assert length + n_tail == c["n_samples"] and ratio > 100 and snr > 0  # a burst stands above its own tail


# ---- cutting
@pytest.mark.parametrize("name,thresh", [(g, 500) for g in GOLDEN] + [("tx22", 3000), ("tfa_2", 6000), ("noise", 0)])
def test_the_merged_chains_do_not_depend_on_the_cut_into_submits(name, thresh):
    if name == "noise":  # an auto stream over noise that keeps it triggered: one chain across every cut, the threshold stepping
        dec = np.random.default_rng(11).integers(-400, 401, 2 * 8 * B).astype(np.int16)
    else:
        dec = golden_dec(name)
        dec = dec[:2 * B * min(8, len(dec) // (2 * B))]
    nb = len(dec) // (2 * B)
    whole = envelope.chains(submits(dec, (nb,), thresh=thresh))
    assert len(whole) >= 1
    for sizes in ((1,) * nb, (1, nb - 1), (nb - 1, 1)):  # every block boundary; the first and the last alone
        subs = submits(dec, sizes, thresh=thresh)
        if name == "noise":
            assert all(int(r["flags"]) & CONT for recs in subs[1:] for r in recs[:1])
        same_chains(envelope.chains(subs), whole, sizes)
    if name == "noise":
        assert len({int(r["thresh"]) for recs in submits(dec, (1,) * nb, thresh=0) for r in recs}) > 1  # the threshold did step


def shifted(dec, pad):
    """`pad` samples of silence ahead of the stream, and silence behind it up to whole blocks."""
    z = dec.reshape(-1, 2)
    n = -(-(len(z) + pad) // B) * B
    out = np.zeros((n, 2), dtype=np.int16)
    out[pad:pad + len(z)] = z
    return out.reshape(-1)


def test_a_cut_inside_a_gap_at_the_last_over_sample_and_one_sample_either_side_of_it():
    """The golden TFA_2 scene moved so that the boundary between two submits falls where merging can go wrong.  Silence ahead of a
    fixed-threshold stream moves its runs and changes nothing else.  -t 6000 cuts into the telegrams' envelope: at 500 they have no
    gap."""
    T = 6000
    dec = golden_dec("tfa_2")[:2 * 4 * B]
    recs = records(dec, thresh=T)[0]
    r = max((c for c in recs if c["n_gaps"] >= 1 and not c["flags"] & OPEN), key=lambda c: int(c["max_gap"]))
    a, last = int(r["start_sample"]), int(r["last_over"])
    z = dec.reshape(-1, 2).astype(np.int64)
    over = np.abs(z).sum(axis=1) > T
    idx = np.flatnonzero(over[a:a + last + 1])
    j = int(np.argmax(np.diff(idx)))  # the longest gap lies between over samples idx[j] and idx[j + 1]
    in_gap, gap_end = a + int(idx[j] + idx[j + 1]) // 2, a + int(idx[j + 1])
    assert idx[j + 1] - idx[j] - 1 == r["max_gap"] >= 3 and not over[in_gap - 1:in_gap + 1].any() and over[a + last]
    for where, target in (("gap", in_gap), ("gap's end", gap_end), ("last_over - 1", a + last - 1), ("last_over", a + last),
                          ("last_over + 1", a + last + 1), ("last_over + 2", a + last + 2), ("start + 1", a + 1)):
        pad = (-target) % B  # the sample `target` becomes the first of a block
        d = shifted(dec, pad)
        nb = len(d) // (2 * B)
        cut = (target + pad) // B
        assert (target + pad) % B == 0 and 0 < cut < nb
        whole = envelope.chains(submits(d, (nb,), thresh=T))
        moved = [c for c in whole if int(c["start_sample"]) == a + pad][0]
        for f in envelope.ENVELOPE_DTYPE.names:  # the run itself did not notice the move
            assert f == "start_sample" or np.array_equal(moved[f], r[f]), (where, f)
        subs = submits(d, (cut, nb - cut), thresh=T)
        pieces = [c for recs2 in subs for c in recs2 if a + pad <= int(c["start_sample"]) < a + pad + int(r["n_samples"])]
        assert len(pieces) == 2 and pieces[1]["flags"] & CONT and pieces[0]["flags"] & OPEN, where
        if where == "last_over + 1":
            assert pieces[1]["last_over"] == -1 and pieces[1]["lead_not_over"] == pieces[1]["n_samples"] == W - 1
        if where == "gap":
            assert pieces[1]["lead_not_over"] >= 1 and pieces[0]["last_over"] < pieces[0]["n_samples"] - 1
            assert pieces[0]["max_gap"] < r["max_gap"] and pieces[1]["max_gap"] < r["max_gap"]  # the longest gap is rebuilt at the cut
        if where == "gap's end":
            assert pieces[1]["lead_not_over"] == 0 and pieces[0]["n_samples"] - 1 - pieces[0]["last_over"] == r["max_gap"]
        same_chains(envelope.chains(subs), whole, where)


@pytest.mark.parametrize("name", GOLDEN)
def test_the_per_block_form_every_run_cut_anywhere_merges_back(name):
    """envelope.split: a run cut into pieces at arbitrary samples -- the block boundaries, every sample around its last over
    sample, inside its longest gap -- merges into its own record."""
    dec = golden_dec(name)
    recs, runs, thr, _ = records(dec)
    rng = np.random.default_rng(3)
    for r, run in zip(recs, runs):
        a, n, last = int(r["start_sample"]), int(r["n_samples"]), int(r["last_over"])
        want = envelope.merge([r])
        cutsets = [list(range(B, a + n, B)), [a + last], [a + last + 1], [a + last - 1, a + last, a + last + 1, a + last + 2], [a + 1],
                   [a + n - 1], sorted(int(v) for v in rng.integers(a + 1, a + n, 5))]
        for cuts in cutsets:
            pieces = envelope.split([dec], [thr], run, ZERO, cuts)
            assert int(pieces["n_samples"].sum()) == n
            assert envelope.merge(pieces).tobytes() == want.tobytes(), (a, cuts)


# ---- gaps
def one_run(dec, **kw):
    recs = records(dec, **kw)[0]
    assert len(recs) == 1
    return recs[0]


def test_gaps_of_1_63_64_and_65_samples():
    overs = [1000]
    for g in (1, 63, 64, 65):
        overs.append(overs[-1] + g + 1)
    for shift in (0, 1, 24, 63):  # the gaps against the mask's 64-sample words
        r = one_run(craft(1, [p + shift for p in overs]))
        assert (r["n_over"], r["n_gaps"], r["max_gap"], r["last_over"], r["lead_not_over"]) == (5, 4, 65, 1 + 63 + 64 + 65 + 4, 0)
        assert r["n_samples"] == r["last_over"] + 1 + W - 1 and r["start_sample"] == 1000 + shift
    r = one_run(craft(1, [1000, 1001, 1002, 1004, 1005]))  # adjacent over samples are no gap
    assert (r["n_over"], r["n_gaps"], r["max_gap"], r["last_over"]) == (5, 1, 1, 5)
    r = one_run(craft(1, [1000]))
    assert (r["n_over"], r["n_gaps"], r["max_gap"], r["last_over"], r["n_samples"]) == (1, 0, 0, 0, W)
    assert r["nprod_head"] == 0 and r["nprod_tail"] == W - 1 and r["energy_head"] == 2 * 3000 * 3000


def test_a_gap_across_a_block_boundary_and_across_a_submit_cut():
    dec = craft(2, [B - 10, B + 20, B + 21])
    whole = one_run(dec)
    assert (whole["n_over"], whole["n_gaps"], whole["max_gap"], whole["last_over"]) == (3, 1, 29, 31)
    # the per-block form: the run's pieces at the block boundary
    run = capture.captures(dec, 0x2F, 500)[0][0]
    p = envelope.split([dec], [500], run, ZERO, [B])
    assert p["n_samples"].tolist() == [10, 22 + W - 1] and p["flags"].tolist() == [OPEN, CONT]
    assert p["n_gaps"].tolist() == [0, 0] and p["last_over"].tolist() == [0, 21] and p["lead_not_over"].tolist() == [0, 20]
    assert envelope.merge(p).tobytes() == envelope.merge([whole]).tobytes()
    # ... and the submits (1, 1) give exactly those pieces
    subs = submits(dec, (1, 1))
    same(np.concatenate(subs), p)
    same_chains(envelope.chains(subs), [envelope.merge([whole])])


def test_a_trailing_stretch_becomes_a_gap_or_stays_tail_when_pieces_merge():
    # a piece that ends in 299 not-over samples, continued by a piece without an over sample: the stretch is tail, no gap
    dec = craft(2, [B - 300])
    subs = submits(dec, (1, 1))
    a, b = subs[0][0], subs[1][0]
    assert (a["n_samples"], a["last_over"], a["flags"]) == (300, 0, OPEN)
    assert (b["n_samples"], b["last_over"], b["lead_not_over"], b["n_over"], b["flags"]) == (W - 300, -1, W - 300, 0, CONT)
    assert b["energy_head"] == 0 and b["nprod_head"] == 0 and b["nprod_tail"] == W - 300  # CONTINUES: the product across the cut is b's
    m = envelope.chains(subs)[0]
    assert (m["n_samples"], m["last_over"], m["n_gaps"], m["max_gap"], m["lead_not_over"]) == (W, 0, 0, 0, 0)
    assert m.tobytes() == envelope.merge([one_run(dec)]).tobytes()
    assert m["energy_tail"] == a["energy_tail"] + b["energy_tail"] and m["energy_head"] == a["energy_head"] == 18000000
    # continued by a piece WITH one: the same stretch, tail in piece a, is a gap of the burst, and a's tail sums are head
    dec = craft(2, [B - 300, B + 50])
    subs = submits(dec, (1, 1))
    a, b = subs[0][0], subs[1][0]
    assert (a["last_over"], a["n_gaps"], b["last_over"], b["lead_not_over"], b["n_gaps"]) == (0, 0, 50, 50, 0)
    m = envelope.chains(subs)[0]
    assert (m["n_gaps"], m["max_gap"], m["last_over"], m["n_over"]) == (1, 349, 350, 2)
    assert m["energy_head"] == a["energy_head"] + a["energy_tail"] + b["energy_head"] and m["energy_tail"] == b["energy_tail"]
    assert m["nprod_head"] == a["nprod_head"] + a["nprod_tail"] + b["nprod_head"] == 350
    assert m.tobytes() == envelope.merge([one_run(dec)]).tobytes()
    # three pieces, the middle one a whole block without an over sample: the gap is rebuilt across both cuts, once
    # (W < B: no run holds such a block, so the pieces' records by hand -- over samples at 0; none; at 3 and 7)
    pieces = np.zeros(3, dtype=envelope.ENVELOPE_DTYPE)
    pieces["n_samples"], pieces["flags"] = (5, 100, 20), (OPEN, CONT | OPEN, CONT)
    pieces["n_over"], pieces["last_over"], pieces["lead_not_over"] = (1, 0, 2), (0, -1, 7), (0, 100, 3)
    pieces["n_gaps"], pieces["max_gap"] = (0, 0, 1), (0, 0, 3)
    m = envelope.merge(pieces)
    assert (m["n_samples"], m["n_over"], m["last_over"], m["n_gaps"], m["max_gap"], m["lead_not_over"]) == (125, 3, 112, 2, 107, 0)
    assert envelope.merge([envelope.merge(pieces[:2]), pieces[2]]).tobytes() == m.tobytes()  # a merged chain continues like a piece


def test_a_continues_piece_without_an_over_sample_and_one_with_a_lead():
    dec = craft(2, [B - 2, B + 100])
    subs = submits(dec, (1, 1))
    b = subs[1][0]
    assert b["flags"] == CONT and (b["lead_not_over"], b["last_over"], b["n_over"]) == (100, 100, 1)
    dec = craft(2, [B - 2])
    b = submits(dec, (1, 1))[1][0]
    assert b["flags"] == CONT and (b["last_over"], b["n_over"], b["lead_not_over"], b["n_samples"]) == (-1, 0, W - 2, W - 2)
    assert b["energy_head"] == 0 and b["energy_tail"] > 0 and b["dot_head"] == b["crs_head"] == 0
    assert envelope.summary(b)[:3] == (0, W - 2, None)  # on its own it has no burst: no ratio


# ---- the summary
def test_the_summary_its_conditions_and_the_line():
    r = one_run(craft(1, list(range(1000, 1200))))
    length, n_tail, ratio, snr = envelope.summary(r)
    et = int(r["energy_tail"])
    assert (length, n_tail) == (200, W - 1) and ratio == 100 * 200 * 18000000 * (W - 1) // (et * 200)
    assert envelope.line("f.iq", r) == "extent f.iq 1000 %d 200 200 0 0 %d.%02d %.1f" % (200 + W - 1, ratio // 100, ratio % 100, snr)
    assert 30 < snr < 50  # (3000, -3000) over noise of +-40: some 40 dB
    short = r.copy()  # n_tail < 64: a condition, whatever the tail holds
    short["n_samples"] = 200 + 63
    assert envelope.summary(short)[:3] == (200, 63, None) and envelope.line("x", short).endswith(" - -")
    short["n_samples"] = 200 + 64
    assert envelope.summary(short)[2] is not None
    silent = r.copy()  # E_tail == 0
    silent["energy_tail"] = 0
    assert envelope.summary(silent)[2] is None
    still_open = r.copy()  # open at the end of the input: its tail was cut
    still_open["flags"] = OPEN
    assert envelope.summary(still_open)[2] is None
    weak = r.copy()  # ratio_c == 0: defined, but no logarithm
    weak["energy_head"] = 1
    assert envelope.summary(weak)[2:] == (0, None) and envelope.line("x", weak).endswith(" 0.00 -")
    # a run open at the input's end, through the records: undefined
    r = one_run(craft(1, [B - 100]))
    assert r["flags"] == OPEN and envelope.summary(r)[:3] == (1, 99, None)


def long_chain():
    """A chain whose energy_head * n_tail exceeds 2^64: 4096 full-scale pieces of one block each, then the burst's end."""
    full = np.full((B, 2), 32767, dtype=np.int16).reshape(-1)
    run = np.zeros(1, dtype=capture.RUN_DTYPE)
    run["n_samples"], run["flags"], run["thresh"] = B, CONT | OPEN, 500
    mid = envelope.envelopes([full], [500], run, [np.array([32767, 32767], dtype=np.int16)])[0]
    assert mid["energy_head"] == B * 2 * 32767 ** 2 and mid["n_over"] == B and mid["last_over"] == B - 1
    end = craft(1, list(range(100)), seed=9)
    run["n_samples"], run["flags"] = 100 + W - 1, CONT
    last = envelope.envelopes([end], [500], run, [np.array([32767, 32767], dtype=np.int16)])[0]
    first = mid.copy()
    first["flags"] = OPEN
    pieces = [first] + [mid] * 4095 + [last]
    for k, p in enumerate(pieces):
        p = pieces[k] = p.copy()
        p["start_sample"] = k * B
    return pieces


def test_the_ratio_needs_128_bits():
    m = envelope.merge(long_chain())
    eh, et, n = int(m["energy_head"]), int(m["energy_tail"]), int(m["n_samples"])
    assert n == 4096 * B + 100 + W - 1 and m["last_over"] == 4096 * B + 99 and m["n_gaps"] == 0
    assert eh * (W - 1) > 1 << 64 and 100 * eh * (W - 1) > 1 << 64
    length, n_tail, ratio, _ = envelope.summary(m)
    assert (length, n_tail) == (4096 * B + 100, W - 1) and ratio == 100 * eh * (W - 1) // (et * length)
    assert ratio != (100 * eh * (W - 1) % (1 << 64)) // (et * length)  # what 64-bit arithmetic would print


# ---- tfrec_gpu's merge: job.h in a stand-alone program
@pytest.fixture(scope="module")
def merge_driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("envelope_merge") / "envelope_merge_driver")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(parity.ROOT, "tests", "merge_driver.cpp")])
    return exe


def test_the_host_merge_prints_the_restatements_lines(merge_driver):
    """Two files through one slot (-n 1), batches of 1 block: the golden TFA_2 scene's 4 blocks, then 3 blocks of noise that keeps
    an auto stream triggered up to the file's end -- its chain is flushed there, still OPEN; and a third file whose chain of 4097
    pieces needs the 128-bit product."""
    noise = np.random.default_rng(12).integers(-400, 401, 2 * 3 * B).astype(np.int16)
    files = [("a.iq", golden_dec("tfa_2")[:2 * 4 * B], 6000), ("b.iq", noise, 0)]  # (-t 6000: the telegrams get gaps)
    lines, want = [], []
    for name, dec, _ in files:
        lines.append("file %s %d" % (name, len(dec) // (2 * B)))
    lines.append("file c.iq 4097")
    for f, (name, dec, thresh) in enumerate(files):
        subs = submits(dec, (1,) * (len(dec) // (2 * B)), thresh=thresh)
        for recs in subs:
            lines.append("batch 1 %d" % f)
            lines += [rec_line(f, r) for r in recs]
        chains = envelope.chains(subs)
        assert any(int(c["n_samples"]) > B for c in chains) or f == 0
        want += [envelope.line(name, c) for c in chains]
    pieces = long_chain()
    for p in pieces:
        lines += ["batch 1 2", rec_line(2, p)]
    want.append(envelope.line("c.iq", envelope.merge(pieces)))
    out = subprocess.run([merge_driver, "envelope"], input="".join(ln + "\n" for ln in lines), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.splitlines() == want and len(want) >= 4
    assert any(ln.split()[8] != "-" and int(ln.split()[6]) >= 1 for ln in want[:-2])  # a golden burst with gaps and a ratio
    assert want[-2].endswith(" - -") and want[-2].split()[3] == str(3 * B - int(want[-2].split()[2]))  # the noise chain reaches its file's end
    assert want[-1].split()[8] != "-"


# ---- the struct, the exports, the command line
def test_the_struct_and_the_exports(tmp_path):
    D = envelope.ENVELOPE_DTYPE
    assert D.itemsize == 128 and api.ENVELOPE_DTYPE is D
    offs = [("stream", 0), ("flags", 4), ("start_sample", 8), ("n_samples", 16), ("thresh", 20), ("n_over", 24), ("last_over", 28),
            ("energy_head", 32), ("energy_tail", 40), ("n_gaps", 48), ("max_gap", 52), ("lead_not_over", 56), ("nprod_head", 60),
            ("dot_head", 64), ("crs_head", 72), ("dot_tail", 80), ("crs_tail", 88), ("nprod_tail", 96), ("reserved", 100)]
    assert [(f, D.fields[f][1]) for f in D.names] == offs
    src = tmp_path / "envelope.c"
    src.write_text('#include <stddef.h>\n#include "tfrec_amd.h"\n'
                   "_Static_assert(sizeof(tfrec_amd_envelope) == 128, \"size\");\n" +
                   "".join("_Static_assert(offsetof(tfrec_amd_envelope, %s) == %d, \"%s\");\n" % (f, o, f) for f, o in offs) +
                   "_Static_assert(sizeof(((tfrec_amd_envelope *)0)->reserved) == 28, \"reserved\");\n")
    subprocess.check_call(["cc", "-std=c11", "-fsyntax-only", "-I", os.path.join(parity.ROOT, "include"), str(src)])
    assert "tfrec_amd_enable_burst_envelope" in api.EXPORTS and "tfrec_amd_read_burst_envelopes" in api.EXPORTS
    L = api.load_library()
    for sym in ("tfrec_amd_enable_burst_envelope", "tfrec_amd_read_burst_envelopes"):
        getattr(L, sym)
    # no GPU is needed to be refused
    assert L.tfrec_amd_enable_burst_envelope(None) == api.E_INVAL
    n = C.c_uint32(7)
    assert L.tfrec_amd_read_burst_envelopes(None, None, 0, C.byref(n)) == api.E_INVAL and n.value == 7


def test_cli_envelope_usage_errors(tmp_path):
    parity.build_cli()
    f = str(tmp_path / "missing.iq")

    out = parity.run_cli(["-Q", "-X", f])
    assert out.returncode == 1 and "-Q measures" in out.stderr
    out = parity.run_cli(["-M", "-Q", "-X", f])  # -M's own refusal comes first and is what it was
    assert out.returncode == 1 and "-M measures" in out.stderr
    out = parity.run_cli(["-h"])
    assert "-Q " in out.stderr and "[-Q]" in out.stderr
    for args in (["-Q", "-k", str(tmp_path / "keep"), "-L", f], ["-Q", "-K", str(tmp_path / "keep"), "-L", f]):
        out = parity.run_cli(args)
        assert out.returncode == 2 and "not with -Q" in out.stderr, args
    for args in (["-Q", "-L", f], ["-Q", "-M", "-L", f], ["-Q", "-s", "50", "-L", f],
                 ["-Q", "-S", str(tmp_path / "cap"), "-n", "1", "-L", f]):
        out = parity.run_cli(args)  # accepted: the file is looked for
        assert out.returncode == 2 and "missing.iq" in out.stderr, args
    out = parity.run_cli(["-Q", "-R", str(tmp_path / "nothing")])  # accepted with -R: the capture is looked for
    assert out.returncode == 2 and "-R replays" not in out.stderr
