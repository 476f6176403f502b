"""The randomised campaign of tests/recorder_campaign.py on the GPU: the recorder's table and pool, the level records, and the burst
meter's, the envelope's, the clock's, the track's and the sync's records and bitmaps, byte for byte against the restatements, on
rows whose runs land on the kernels' own strides -- and the layouts no hand-aimed module reaches: more runs in a stream's submit
than a workgroup has lanes, a dense stream beside sparse ones at 65 streams, the measurements alone and together, and tracks of one
value under a sync word of one value, where every hit can be counted.  Everything is an exact integer; nothing here has a
tolerance.  tests/test_recorder_campaign_cpu.py shows that the fixed seeds reach every edge class, the sync's included.

The fixed campaign: seeds recorder_campaign.SEEDS = (12, 19, 21, 24, 35, 91), recorder_campaign.ROUNDS = 6 rounds each; about half
the rounds have a sync.  Wall times measured on an MI355X host (the restatements on the CPU dominate; the first case also loads the
library and starts the device):
  test_campaign[12] 8.5 s, [19] 0.7 s, [21] 0.5 s, [24] 0.7 s, [35] 0.3 s, [91] 0.4 s
  test_densest_runs_overrun_every_lookup_stride 1.2 s, test_dense_stream_beside_sparse_ones_at_65_streams 0.9 s,
  test_each_measurement_alone_equals_all_four_together 0.3 s,
  test_tracks_of_one_value_give_exact_hit_counts_at_every_edge 0.1 s a case; the module 15 s.
python tests/recorder_campaign.py <seed> 50, with the sync in its rounds, reported 0 mismatches for the seeds 1001 and 2002, which are
not in the list.

The track's modes (amplitude, auto-centre, phase: amplitude.h, centre.h, phase.h): seeds recorder_campaign.MODE_SEEDS = (112, 120,
122, 130, 131, 143), ROUNDS rounds each, round rnd in the mode rnd % 3; the dense tests once per mode; the head kernels' entry loop
on more table entries than their grid has workgroups; the measurements test in every mode.  Wall times on an MI355X host, after
the restatements in tfrec_amd/track.py were made to compute a stream's pairs and over bits once per call (before that the
2159-entry case took 10 s and more on the CPU alone):
  test_mode_campaign[112] 0.5 s, [120] 0.5 s, [122] 0.4 s, [130] 0.5 s, [131] 0.5 s, [143] 0.3 s
  test_densest_runs_overrun_every_lookup_stride[frequency] 0.7 s, [amplitude] 0.7 s, [auto] 0.7 s, [phase] 0.7 s
  test_dense_stream_beside_sparse_ones_at_65_streams[frequency] 0.8 s, [amplitude] 0.8 s, [auto] 0.8 s, [phase] 0.9 s
  test_the_head_kernels_entry_loop_makes_a_second_trip[auto-None] 0.1 s, [phase-None] 0.2 s, [auto-2049] 0.2 s, [phase-2049] 0.2 s
  test_each_measurement_alone_equals_all_four_together 0.7 s (with the three modes); the module 21 s.
python tests/recorder_campaign.py <seed> 50 modes reported 0 mismatches for the seeds 1001 and 2002 (50 rounds ok each), and
18 rounds each of the seeds 1, 2 and 3 did too.  No mismatch between a kernel and its restatement has been found by the modes'
campaign so far.
"""
import functools

import numpy as np
import pytest

import recorder_campaign as RC
from tfrec_amd import capture, sync, track

pytestmark = pytest.mark.gpu

B = RC.B
ALL = RC.MEASURES
SHORT = sync.Settings(96000, 0x2D, 8, 2, True)  # a span of 28 samples: most samples of a 356-sample run have their distance


@pytest.mark.parametrize("seed", RC.SEEDS)
def test_campaign(seed):
    assert RC.campaign(seed, RC.ROUNDS, verbose=False) == 0


@pytest.mark.parametrize("seed", RC.MODE_SEEDS)
def test_mode_campaign(seed):
    """The same campaign with the track in its amplitude, auto-centre and phase modes in turn (round rnd: mode rnd % 3)."""
    assert RC.campaign(seed, RC.ROUNDS, verbose=False, modes=True) == 0


def pieces(reads, m):
    return [g[m] for g in reads]


def mode_of(name, n):
    """The four modes at settings in between their limits; amplitude: a level per stream, below, at and above the dense row's one
    over sample's power of 6000 spread over L = 5 and 7."""
    return {"frequency": None, "amplitude": ("amplitude", [(0, 1200, 857, 6000, 65535)[s % 5] for s in range(n)]), "auto": ("auto", 1024),
            "phase": ("phase", 1024, 10)}[name]


MODE_NAMES = ("frequency", "amplitude", "auto", "phase")
SWAPS = (1, 4, 7, 10, 118, 241, 244)  # the dense row's periods that get a head to measure: four in block 0, F M F M F M F M ...; one
# whose run is open across the cut of (5, 7) (period 114's run crosses sample 5 B; 118's begins behind it); two in block 10


def centre_sources(reads, s):
    return np.concatenate([g["centres"]["source"][g["centres"]["stream"] == s] for g in reads])


@pytest.mark.parametrize("name", MODE_NAMES)
def test_densest_runs_overrun_every_lookup_stride(name):
    """Mask 0x02's densest legal input, one over sample every 357: 276 runs per stream in one submit of 12 blocks, so every
    `for (k = t; k < nr; k += THREADS)` makes a second trip and dozens of runs meet each block's [lo, hi) lookup; the staging has
    room for 279.  In the auto and phase modes a run of one over sample counts 0 products and falls back, so len(SWAPS) = 7
    periods of every stream hold a stretch of 358 over samples instead (recorder_campaign.dense_heads): 7 measured entries and 262
    that fall back per stream, 269 runs, alternating one by one through block 0."""
    mode = mode_of(name, 3)
    heads = mode is not None and mode[0] in ("auto", "phase")
    x = np.stack([RC.dense_heads(12, SWAPS) if heads else RC.dense(12)] * 3)
    per = 276 - len(SWAPS) if heads else 276
    centres = [0, 20000, -192000]
    whole = RC.run_plan(RC.make_plan(x, 0x02, [0x02] * 3, (12,), L=5, centres=centres, sync=SHORT, mode=mode))
    runs = whole[0]["table"][0]
    stage_cap = 12 * B // 356 + 3
    for s in range(3):
        mine = runs[runs["stream"] == s]
        assert 256 < len(mine) <= stage_cap and mine[-1]["flags"] == capture.RUN_OPEN
    for m in ALL + ("sync",):
        assert len(whole[0][m][0] if m in ("track", "sync") else whole[0][m]) == len(runs) == 3 * per
    srecs = whole[0]["sync"][0]  # five trips of the carry kernel's record loop per stream, and matches in nearly every run
    if mode is None:
        assert np.count_nonzero(srecs["n_hits"]) > 800 and (srecs["best"] <= SHORT.P // 2).all()
    if heads:
        for s in range(3):
            src = centre_sources(whole, s)
            assert len(src) == per and np.count_nonzero(src == track.MEASURED) == 7 and np.count_nonzero(src == track.FALLBACK) == per - 7
            assert src[:8].tolist() == [track.FALLBACK, track.MEASURED] * 4
        cen = whole[0]["centres"]
        assert len({int(c) for c in cen["centre_hz"][(cen["stream"] == 0) & (cen["source"] == track.MEASURED)]}) >= 6  # each its own
    # the same rows cut as (5, 7), both submits queued before the first read: the merged chains are the uncut ones
    cut = RC.run_plan(RC.make_plan(x, 0x02, [0x02] * 3, (5, 7), L=5, centres=centres, drains=[None, None], sync=SHORT, mode=mode))
    assert all(max(np.count_nonzero(g["table"][0]["stream"] == s) for s in range(3)) > 100 for g in cut)
    for m in ALL + ("sync",):
        RC.same_chains(m, RC.merged(m, pieces(cut, m)), RC.merged(m, pieces(whole, m)), "cut (5, 7)")
    if heads:  # (the run across the cut has one over sample: the fallback in both, and its continuation inherits it)
        a, b = track.centre_chains(pieces(cut, "centres")), track.centre_chains(pieces(whole, "centres"))
        assert sorted(c.tobytes() for c in a) == sorted(c.tobytes() for c in b) and len(a) == 3 * per
        assert np.count_nonzero(cut[1]["centres"]["source"] == track.INHERITED) == 3


@pytest.mark.parametrize("name", MODE_NAMES)
def test_dense_stream_beside_sparse_ones_at_65_streams(name):
    """Every fourth stream is the dense row under its own mask 0x02, the others generated rows under the context's 0x2F: the run
    lookup, a W per stream and a stream count past one wave together; two submits, both queued before the first read.  In the
    modes the sparse rows also hold the modes' kinds of stretch; in the auto and phase modes periods 1, 4, 7 and 25 of the dense
    rows hold a head to measure: 4 measured entries per dense stream, 3 of them in block 0, between entries that fall back."""
    n, nb = 65, 2
    mode = mode_of(name, n)
    heads = mode is not None and mode[0] in ("auto", "phase")
    masks = [0x02 if s % 4 == 0 else 0x2F for s in range(n)]
    x = RC.rows(np.random.default_rng(65), n, nb, [RC.window(m) for m in masks], cuts=(1,), extra=RC.MODE_KINDS if mode else ())
    x[::4] = RC.dense_heads(nb, (1, 4, 7, 25)) if heads else RC.dense(nb)
    p = RC.make_plan(x, 0x2F, masks, (1, 1), L=7, centres=[(0, 20000, -35000)[s % 3] for s in range(n)], drains=[None, None], sync=SHORT,
                     mode=mode)
    assert p["configured"] == list(range(0, n, 4))
    reads = RC.run_plan(p)
    if mode is None:
        assert all(np.count_nonzero(g["sync"][0]["n_hits"]) > len(g["sync"][0]) // 2 for g in reads)
    for g in reads:
        per = np.bincount(g["table"][0]["stream"], minlength=n)
        assert (per[::4] >= B // RC.DENSE_PERIOD - 3).all() and per[64] >= 22 - 3 * heads and np.delete(per, np.arange(0, n, 4)).min() >= 1
        assert heads or (per[::4] >= B // RC.DENSE_PERIOD).all() and per[64] >= 22
    assert (reads[1]["table"][0]["flags"] & capture.RUN_CONTINUES).any()
    if heads:
        for s in range(0, n, 4):
            src = centre_sources(reads, s)
            assert np.count_nonzero(src == track.MEASURED) == 4 and src[:6].tolist() == [track.FALLBACK, track.MEASURED] * 3
        sparse = np.concatenate([g["centres"]["source"][g["centres"]["stream"] % 4 != 0] for g in reads])
        assert {track.MEASURED, track.FALLBACK, track.INHERITED} <= set(sparse.tolist())


@functools.lru_cache(maxsize=None)
def second_trip_rows():
    """int16 [8, 12 B, 2] under mask 0x02, one submit: more table entries than the head kernels' grid of min(max_runs, 2048)
    workgroups, so their entry loop `for (e = blockIdx.x; e < ne; e += gridDim.x)` makes a second trip on the LDS the first one
    left.  A loud head (66 over samples: 65 counted products) makes its run 421 samples long, where the dense row's are 356, so the
    8 dense streams' 2208 entries cannot all stay: stream 0's first 160 runs are loud (247 runs), streams 1 .. 6 are the dense row
    (276 each: 1903 entries ahead of stream 7), and stream 7 is dense for 145 runs and loud from there on (256 runs) -- entries
    0 .. 159 and every entry from 2048 on, 111 of them, have a loud head, each at a carrier of its own, and what the workgroups
    of the second trip saw on their first is stream 0's loud heads (entries 0 .. 110)."""
    x = np.stack([RC.dense_loud(12, 0, 160, 0)] + [RC.dense(12)] * 6 + [RC.dense_loud(12, 145, 1000, 50)])
    x.setflags(write=False)
    return x


@pytest.mark.parametrize("max_runs", [None, 2049])
@pytest.mark.parametrize("name", ["auto", "phase"])
def test_the_head_kernels_entry_loop_makes_a_second_trip(name, max_runs):
    """Records and words byte for byte (run_plan's reads).  max_runs = 2049: the table overflows, 2049 entries have records, and
    one workgroup alone makes the second trip."""
    x = second_trip_rows()
    mode = ("auto", 1024) if name == "auto" else ("phase", 1024, 3)
    p = RC.make_plan(x, 0x02, [0x02] * 8, (12,), L=5, centres=[(24000, -7000, 192000, 0)[s % 4] for s in range(8)], measure=("track",), mode=mode)
    runs = p["expect"][0]["table"][0]
    per = np.bincount(runs["stream"]).tolist()
    assert per == [247] + [276] * 6 + [256] and 2048 < len(runs) == 2159 <= RC.full_cap(p)[0]
    if max_runs:
        p["cap"] = (max_runs, RC.full_cap(p)[1])
    reads = RC.run_plan(p)
    cen = reads[0]["centres"]
    assert len(cen) == (max_runs or len(runs))
    loud = np.r_[0:160, 2048:len(cen)]
    assert (cen["source"][loud] == track.MEASURED).all() and (cen["n_counted"][loud] == 65).all()
    assert (np.delete(cen["source"], loud) == track.FALLBACK).all() and not np.delete(cen["n_counted"], loud).any()
    second = cen[2048:]  # each against what its workgroup measured on its first trip
    assert (second["centre_hz"] != cen["centre_hz"][:len(second)]).all() and (second["index"] != cen["index"][:len(second)]).all()


def test_each_measurement_alone_equals_all_four_together():
    """The kernels share one low-priority lane and the recorder's buffers: what one measurement reads does not depend on which others
    run beside it, and the table and the pool are a recorder-only context's."""
    rng = np.random.default_rng(4)
    masks = [0x2F, 0x02, 0x21, 0x08, 0x2F]
    x = RC.rows(rng, 5, 3, [RC.window(m) for m in masks], cuts=(1,))
    p = RC.make_plan(x, 0x2F, masks, (1, 2), L=9, centres=[0, 192000, -192000, 20000, -35000], drains=[None, None], sync=SHORT)
    assert sum(len(e["table"][0]) for e in p["expect"]) >= 40
    plain = RC.run_plan(p, measure=())  # (no track: no sync either)
    assert "sync" not in plain[0]
    every = RC.run_plan(p, measure=ALL)
    for k, (a, b) in enumerate(zip(plain, every)):
        assert a["table"][0].tobytes() == b["table"][0].tobytes() and a["table"][1].tobytes() == b["table"][1].tobytes(), k
    for m in ALL:
        alone = RC.run_plan(p, measure=(m,))
        for k, (a, b, c) in enumerate(zip(alone, every, plain)):
            assert a["table"][0].tobytes() == c["table"][0].tobytes() and a["table"][1].tobytes() == c["table"][1].tobytes(), (m, k)
            if m == "track":  # ... and the sync with only the track beside it is the sync beside all four
                assert a[m][0].tobytes() == b[m][0].tobytes() and a[m][1].tobytes() == b[m][1].tobytes(), (m, k)
                assert a["sync"][0].tobytes() == b["sync"][0].tobytes() and a["sync"][1].tobytes() == b["sync"][1].tobytes(), ("sync", k)
                assert a["sync"][0]["n_hits"].sum() > 0
            else:
                RC.same_records(a[m], b[m], "%s alone, submit %d" % (m, k))
    # the track's modes: the table, the pool and the meter's, envelope's and clock's records are the frequency-mode context's, and
    # the mode's own track and centre records do not depend on which other measurements run beside it
    for name in MODE_NAMES[1:]:
        q = RC.make_plan(x, 0x2F, masks, (1, 2), L=9, centres=p["centres"], drains=[None, None], sync=SHORT, mode=mode_of(name, 5))
        beside, alone = RC.run_plan(q, measure=ALL), RC.run_plan(q, measure=("track",))
        for k, (a, b, c) in enumerate(zip(beside, every, alone)):
            assert a["table"][0].tobytes() == b["table"][0].tobytes() and a["table"][1].tobytes() == b["table"][1].tobytes(), (name, k)
            assert c["table"][0].tobytes() == b["table"][0].tobytes() and c["table"][1].tobytes() == b["table"][1].tobytes(), (name, k)
            for m in ("meter", "envelope", "clock"):
                RC.same_records(a[m], b[m], "%s beside the %s track, submit %d" % (m, name, k))
            for m in ("track", "sync"):
                assert a[m][0].tobytes() == c[m][0].tobytes() and a[m][1].tobytes() == c[m][1].tobytes(), (name, m, k)
            assert ("centres" in a) == (name != "amplitude") == ("centres" in c)
            if name != "amplitude":
                assert a["centres"].tobytes() == c["centres"].tobytes() and len(a["centres"]) == len(a["track"][0]), (name, k)
        assert any(a["track"][1].tobytes() != b["track"][1].tobytes() for a, b in zip(beside, every)), name  # (another track than the frequency mode's)


# ---- exact hit counts: tracks of one value under a pattern of one value
HIT_MASKS = [0x2F, 0x02, 0x20]
HIT_CENTRES = [0, -35000, 20000]


@functools.lru_cache(maxsize=None)
def hit_rows():
    """int16 [3, 2 B, 2], to be cut (1, 1): the campaign's generator with every stretch of the `const` kind -- all its samples are
    one pair, so every cross product is 0 and the track over the stretch is one value: 0 about the centre 0 (a zero sum), and
    about the centre -35000 Hz 1, about 20000 Hz 0 (the sign of -dot S[r]) -- placed by _interior and _boundary at the campaign's
    classes 1, 2, 5 (at the cut: 6), 7 and 9; stream 0 also holds a stretch of 1600 samples that is open through the cut."""
    x = RC.rows(np.random.default_rng(5), 3, 2, [RC.window(m) for m in HIT_MASKS], cuts=(1,), kind="const")
    x[0, B - 700:B + 900] = (3000, 0)
    hit = RC.classes_hit(x, HIT_MASKS, [RC.T] * 3, (1, 1))
    assert {"6", "7", "9"} <= hit and {lab[0] for lab in hit} >= {"1", "2"} and "5" in RC.classes_hit(x, HIT_MASKS, [RC.T] * 3, (2,))
    x.setflags(write=False)
    return x


def constant_stretches(st, tchain):
    """The stretches of consecutive hits that a merged track's runs of one value give, counted from the track's bits alone: over
    a maximal run [u, v] of the value w every tap of the samples u + span .. v reads w, so each of them is a hit if w is the
    pattern's one bit value (d = 0) or, under BOTH, the other (d = P) -> [(first, last sample)], chain-relative, 65 and longer."""
    w_hit = {st.bit[0]} | ({1 - st.bit[0]} if st.both else set())
    edges = np.flatnonzero(np.diff(tchain.bits.astype(np.int8))) + 1
    out = []
    for u, e in zip(np.concatenate([[0], edges]), np.concatenate([edges, [len(tchain.bits)]])):
        if int(tchain.bits[u]) in w_hit and e - (u + st.span) >= 65:
            out.append((int(u) + st.span, int(e) - 1))
    return out


@pytest.mark.parametrize("rate", [96000, 8960])
@pytest.mark.parametrize("pattern,both", [(0x00, False), (0xFF, True)])
def test_tracks_of_one_value_give_exact_hit_counts_at_every_edge(rate, pattern, both):
    """The masks j0, j1 and `mask`, the `g &=` cut-off behind a run and the two stores, at every edge at once: the all-zero
    pattern, then the all-one pattern under BOTH, with E = 0, at a span of 28 (inside one lane's word) and of 300.  The restated
    tracks of the `const` stretches are constant as hit_rows says (the CPU run of constant_stretches showed it), so the patterns
    stay all-zero and all-one.  Besides run_plan's byte-for-byte comparison: several chains have a stretch of 65 and more
    consecutive hits, whose length follows from the track's bits alone; one crosses sample B, which is a block boundary inside the
    uncut submit and the cut of (1, 1); the matches over every stretch number its length, in both."""
    st = sync.Settings(rate, pattern, 8, 0, both)
    assert st.span == (28 if rate == 96000 else 300) and st.pattern in (0, 0xFF)
    plans = [RC.make_plan(hit_rows(), 0x2F, HIT_MASKS, sizes, L=5, centres=HIT_CENTRES, drains=[None] * len(sizes), measure=("track",),
                          sync=st) for sizes in ((2,), (1, 1))]
    ref = RC.restate(plans[0], (2,), measure=("track",))
    tch, sch = RC.merged("track", [ref[0]["track"]]), RC.merged("sync", [ref[0]["sync"]])
    want = [(i, a, b) for i, t in enumerate(tch) for a, b in constant_stretches(st, t)]
    assert len({i for i, _, _ in want}) >= 3, want
    across = [(i, a, b) for i, a, b in want if int(tch[i]["start_sample"]) + a < B - 32 and int(tch[i]["start_sample"]) + b > B + 32]
    assert across and {int(tch[i]["stream"]) for i, _, _ in across} >= {0}
    if both:  # tracks of both values match
        assert {int(tch[i].bits[a]) for i, a, _ in want} == {0, 1}
    for i, a, b in want:
        assert sch[i].bits[a:b + 1].all() and int(sch[i]["n_hits"]) >= b - a + 1
    for p in plans:
        reads = RC.run_plan(p)
        if len(p["sizes"]) == 2:  # the stretch across the cut: ones at the first piece's last sample and the second's first
            first, second = reads[0]["sync"], reads[1]["sync"]
            o = first[0][(first[0]["stream"] == 0) & (first[0]["flags"] & capture.RUN_OPEN != 0)]
            c = second[0][(second[0]["stream"] == 0) & (second[0]["flags"] & capture.RUN_CONTINUES != 0)]
            assert len(o) == len(c) == 1 and sync.bits_of(o[0], first[1])[-65:].all() and sync.bits_of(c[0], second[1])[:65].all()
        got = RC.merged("sync", pieces(reads, "sync"))
        RC.same_chains("sync", got, sch, "sizes %s" % (p["sizes"],))
        for i, a, b in want:
            assert int(np.count_nonzero(got[i].bits[a:b + 1])) == b - a + 1, (p["sizes"], i, a, b)
