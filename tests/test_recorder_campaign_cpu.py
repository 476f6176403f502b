"""tests/recorder_campaign.py without a GPU: the generator is deterministic, the fixed seeds of tests/test_recorder_campaign_gpu.py
reach every edge class the campaign names (measured back from capture.captures on the generated rows, class by class) and every
class of the burst sync's (measured back from its restatement on the plans), the sync's settings leave the earlier seeds' plans as
they were, the restatements the kernels are held to equal their per-sample forms at those edges, and the campaign's own checks --
run against a model of the receiver put together from the restatements -- pass, notice one planted wrong bit, and notice a sync
that is wrong by one in each of the places where a kernel could be.  The same for the track's amplitude, auto-centre and phase modes:
MODE_SEEDS reach every label of MODE_CLASSES, at most a quarter of the auto and phase chains are exempt from the merged check, the
fast restatements of the modes equal their per-sample forms, the campaign with modes on passes on the model, notices a planted bit
in the centre records and in each mode's track, and notices each of the mistakes of MODE_WRONG."""
import functools
import hashlib

import numpy as np
import pytest

import recorder as R
import recorder_campaign as RC
from tfrec_amd import api, burst, capture, clock, decin, envelope, levels, sync, track, tune

B = RC.B


# ---- the generator
def test_the_generator_is_deterministic_per_seed():
    a, b = RC.plans(RC.SEEDS[0], 4), RC.plans(RC.SEEDS[0], 4)
    assert [RC.describe(p) for p in a] == [RC.describe(p) for p in b]
    assert all(p["x"].tobytes() == q["x"].tobytes() and p["x"].dtype == np.int16 for p, q in zip(a, b))
    assert RC.plans(RC.SEEDS[1], 1)[0]["x"].tobytes() != a[0]["x"].tobytes()
    rng = np.random.default_rng(3)
    x = RC.rows(rng, 3, 2, [694, 356, 400], cuts=(1,))
    assert x.shape == (3, 2 * B, 2) and x.dtype == np.int16
    assert RC.rows(np.random.default_rng(3), 3, 2, [694, 356, 400], cuts=(1,)).tobytes() == x.tobytes()


# SHA-256 over describe(p) and p["x"].tobytes() of plans(seed, ROUNDS), taken at the commit ahead of the sync's (3c0a152, whose
# describe() had no sync part and whose plans had none): the rows, masks, cuts, drains, resets, caps, L, centres and drawn
# measurements of the seeds that were fixed then
PLAN_DIGESTS = {12: "b4ad749eb5347b89337f100b684f854dfe01509101f120d4604363f305e73715",
                19: "b238998c57ab512ae94e1a2e9fc061dc683c491fcb0cd80cd107df31ccf7f972",
                21: "0990b32bd5749128e242964844fbe5461e9220ebf116e44228129d0251bdeea9",
                24: "0ffacbe0ffd2cd04eefb70e1984784174bb8d979b8e6eddbc06f6e504685240e"}


@pytest.mark.parametrize("seed", sorted(PLAN_DIGESTS))
def test_the_sync_leaves_the_plans_of_the_earlier_seeds_as_they_were(seed):
    assert RC.SEEDS[:4] == (12, 19, 21, 24) and RC.ROUNDS == 6
    h = hashlib.sha256()
    for p in RC.plans(seed, RC.ROUNDS):
        h.update(RC.describe(p, with_sync=False).encode())
        h.update(p["x"].tobytes())
        assert set(p["measure"]) == set(p["drawn"]) | ({"track"} if p["sync"] is not None else set())  # the one permitted change
        assert RC.describe(p).startswith(RC.describe(p, with_sync=False).rsplit(" measure ", 1)[0]) and " sync " in RC.describe(p)
    assert h.hexdigest() == PLAN_DIGESTS[seed]


@functools.lru_cache(maxsize=None)
def fixed_plans():
    return [p for seed in RC.SEEDS for p in RC.plans(seed, RC.ROUNDS)]


@functools.lru_cache(maxsize=None)
def fixed_hits():
    hit = set()
    for p in fixed_plans():
        hit |= RC.classes_hit(p["x"], p["masks"], p["thresh"], p["sizes"])
    return hit


@pytest.mark.parametrize("label", RC.CLASSES)
def test_the_fixed_seeds_reach_every_edge_class(label):
    assert label in fixed_hits()


@functools.lru_cache(maxsize=None)
def fixed_sync_hits():
    hit = set()
    for p in fixed_plans():
        hit |= RC.sync_classes_hit(p)
    return hit


@pytest.mark.parametrize("label", RC.SYNC_CLASSES)
def test_the_fixed_seeds_reach_every_sync_class(label):
    assert label in fixed_sync_hits()


def test_the_sync_draw_covers_its_settings():
    ps = fixed_plans()
    with_sync = [p for p in ps if p["sync"] is not None]
    assert all(p["sync"] is not None for k, p in enumerate(ps) if k % RC.ROUNDS % 3 == 0)  # every round with rnd % 3 == 0
    assert len(ps) // 3 < len(with_sync) < 2 * len(ps) // 3 and all("track" in p["measure"] for p in with_sync)
    assert any(8 < p["sync"].P < 64 for p in with_sync) and any(0 < p["sync"].E < (p["sync"].P - 1) // 2 for p in with_sync)
    assert any(32 <= p["sync"].span < 2047 for p in with_sync)
    assert any(p["sync"].pattern == 0xAAAAAAAAAAAAAAAA & ((1 << p["sync"].P) - 1) for p in with_sync)  # alternating
    for P in (8, 9, 12, 33, 64):  # the smallest legal rate: one less is refused
        R = RC.min_rate(P)
        assert sync.deltas(R, P)[-1] <= 2047 < sync.deltas(R - 1, P)[-1]


def test_the_fixed_seeds_draw_every_kind_of_round():
    ps = fixed_plans()
    tables = [e["table"][0] for p in ps for e in p["expect"]]
    assert {int(o) % 32 for t in tables for o in t["pool_offset"]} == set(range(32))  # the track's shift, every one
    assert {int(o) % 4 for t in tables for o in t["pool_offset"]} == set(range(4))
    flags = np.concatenate([t["flags"] for t in tables])
    assert {0, capture.RUN_OPEN, capture.RUN_CONTINUES, capture.RUN_OPEN | capture.RUN_CONTINUES} <= set(flags.tolist())
    assert any(p["nb"] == 12 and p["ctx_mask"] == 0x02 for p in ps)  # the dense row alone ...
    assert any(p["nb"] <= 4 and (p["x"] == RC.dense(p["nb"])).all(axis=(1, 2)).any() for p in ps)  # ... and beside ordinary rows
    assert max(np.count_nonzero(t["stream"] == t["stream"][0]) for t in tables if len(t)) > 256  # more runs than a workgroup has lanes
    assert any(len(set(p["windows"])) > 1 for p in ps)  # W differs per stream under one context
    assert {len(p["sizes"]) for p in ps} == {1, 2, 3, 4} and any(d is None for p in ps for d in p["drains"][:-1])
    assert any(p["reset"] for p in ps) and {p["L"] for p in ps} >= {1, 16}
    assert {-192000, 0, 192000} <= {c for p in ps if "track" in p["measure"] for c in p["centres"]}  # both limits included
    assert any(set(p["measure"]) == set(RC.MEASURES) for p in ps) and all(p["measure"] for p in ps)
    for m in RC.MEASURES:
        assert any(p["measure"] == (m,) for p in ps) or any(m not in p["measure"] for p in ps)
    full = [RC.full_cap(p) for p in ps]
    assert any(p["cap"] and p["cap"][0] < f[0] for p, f in zip(ps, full))  # max_runs tight ...
    assert any(p["cap"] and p["cap"][1] < f[1] for p, f in zip(ps, full))  # ... and max_samples
    for p in ps:
        if p["cap"]:  # a prefix is delivered, and something is cut off
            cut = [capture.prefix(e["table"][0], e["table"][1], *p["cap"]) for e in p["expect"]]
            assert any(ov for _, _, ov in cut), RC.describe(p)


def test_the_dense_row_is_the_densest_a_recorder_meets():
    """Mask 0x02 (W = 356), one over sample every 357: 276 runs in 12 blocks, three below the staging's room."""
    runs = capture.captures(RC.dense(12), 0x02, RC.T)[0]
    assert len(runs) == 276 and 256 < len(runs) <= 12 * B // 356 + 3 == 279
    assert (runs["n_samples"][:-1] == 356).all() and runs["n_samples"][-1] == 129 and runs["flags"][-1] == capture.RUN_OPEN
    assert (np.diff(runs["start_sample"]) == 357).all()
    per_block = np.bincount((runs["start_sample"] // B).astype(np.int64), minlength=12)
    assert per_block.min() >= 22  # dozens of runs meet every block


# ---- the restatements at these edges: the vectorised forms against the per-sample ones
SPAN_28 = sync.Settings(96000, 0x00, 8, 3, True)  # every comparison inside one lane's word
SPAN_2047 = sync.Settings(1313, 0xD4, 8, 2, False)  # the largest span


def brute_equals_fast(x, masks, thresh, sizes, L, centres, first=None):
    """Submit by submit, as the kernels are asked: captures, levels, bursts, envelopes, clocks, tracks and -- at a span below 32 and
    at the largest -- syncs, fast against bruteforce; first: the measurements on the table's first entries only."""
    sst, sbr = {st: None for st in (SPAN_28, SPAN_2047)}, {st: None for st in (SPAN_28, SPAN_2047)}
    n = len(x)
    dec = decin.clamp(x)
    cst, cbr, lst, lbr, tst, tbr = [None] * n, [None] * n, [None] * n, [None] * n, None, None
    prev, base, pos, total = [np.zeros(2, dtype=np.int16)] * n, [0] * n, 0, 0
    for nb in sizes:
        decs = [np.ascontiguousarray(dec[s, pos * B:(pos + nb) * B]).reshape(-1) for s in range(n)]
        per, thr = [], []
        for s in range(n):
            runs, pool, cst[s] = capture.captures(decs[s], masks[s], thresh[s], cst[s])
            bruns, bpool, cbr[s] = capture.captures_bruteforce(decs[s], masks[s], thresh[s], cbr[s])
            assert runs.tobytes() == bruns.tobytes() and pool.tobytes() == bpool.tobytes(), "captures, stream %d" % s
            lev, lst[s] = levels.levels(decs[s], masks[s], thresh[s], lst[s])
            blev, lbr[s] = levels.levels_bruteforce(decs[s], masks[s], thresh[s], lbr[s])
            assert lev.tobytes() == blev.tobytes(), "levels, stream %d" % s
            per.append((runs, pool))
            thr.append(np.repeat(lev["thresh"].astype(np.int64), B))
        table = capture.table(per)[0][:first]
        RC.same_records(burst.bursts(decs, table, prev, base=base), burst.bursts_bruteforce(decs, table, prev, base=base), "bursts")
        RC.same_records(envelope.envelopes(decs, thr, table, prev, base=base),
                        envelope.envelopes_bruteforce(decs, thr, table, prev, base=base), "envelopes")
        RC.same_records(clock.clocks(decs, table, base=base), clock.clocks_bruteforce(decs, table, base=base), "clocks")
        recs, words, tst = track.tracks(decs, thr, table, L, centres, tst, base=base)
        brecs, bwords, tbr = track.tracks_bruteforce(decs, thr, table, L, centres, tbr, base=base)
        RC.same_records(recs, brecs, "tracks")
        assert np.array_equal(words, bwords) and np.array_equal(tst["carry"], tbr["carry"]) and np.array_equal(tst["prior"], tbr["prior"])
        for st in sst:
            srecs, swords, sst[st] = sync.syncs(recs, words, st, sst[st], n)
            bsrecs, bswords, sbr[st] = sync.syncs_bruteforce(brecs, bwords, st, sbr[st], n)
            RC.same_records(srecs, bsrecs, "syncs, span %d" % st.span)
            assert np.array_equal(swords, bswords), "sync words, span %d" % st.span
            assert all(np.array_equal(u, v) for u, v in zip(sst[st]["bits"], sbr[st]["bits"])), "carried bits, span %d" % st.span
        total += len(table)
        prev, pos, base = [d.reshape(-1, 2)[-1] for d in decs], pos + nb, [v + nb * B for v in base]
    return total


def test_the_fast_restatements_equal_the_per_sample_ones_on_a_generated_round():
    rng = np.random.default_rng(RC.SEEDS[0])
    masks, sizes = [0x2F, 0x02], (1, 1)
    x = RC.rows(rng, 2, 2, [RC.window(m) for m in masks], cuts=(1,))
    assert len(RC.classes_hit(x, masks, [RC.T, 90], sizes)) >= 8
    assert brute_equals_fast(x, masks, [RC.T, 90], sizes, 7, [20000, -192000]) >= 10


def test_the_fast_restatements_equal_the_per_sample_ones_on_the_dense_rows_first_40_runs():
    assert brute_equals_fast(RC.dense(2)[None], [0x02], [RC.T], (2,), 16, [35000], first=40) == 40


# ---- what the campaign found: a run whose hold ends with a submit's last sample
def test_a_chain_that_ends_with_a_submits_last_sample_merges_into_the_uncut_runs_record(tmp_path):
    """Class 3 at a submit cut.  The piece reaches its submit's last sample, so it is OPEN, and the next submit has no CONTINUES
    piece: the chain ended exactly there.  The merged record -- burst.chains' walk for all four measurements, and tfrec_gpu's
    chain_merger (tfrec_amd/host/job.h, compiled into a stand-alone program under the address and undefined-behaviour sanitizers) --
    is the uncut run's: not OPEN, and the envelope's ratio is defined; the sync's merged record and match track are the uncut
    run's too.  Stream 0: nothing follows; stream 1: a later run does."""
    import os
    import subprocess

    import parity
    from recorder_rows import rec_line

    W = 694
    x = np.stack([RC.quiet(2, 51), RC.quiet(2, 52)])
    for s in range(2):
        x[s, B - W - 200:B - W + 1] = RC._tone(2, 22, 3)[B - W - 200:B - W + 1]  # the last over sample at B - W: the run ends with B
    x[1, B + 3000:B + 3100] = (3000, 0)
    cut, whole = (RC.make_plan(x, 0x2F, [0x2F] * 2, sizes, L=7, centres=[0, 20000], sync=SPAN_28) for sizes in ((1, 1), (2,)))
    first = cut["expect"][0]["table"][0]
    assert first["flags"].tolist() == [capture.RUN_OPEN] * 2 and (first["start_sample"] + first["n_samples"] == B).all()
    assert not (cut["expect"][1]["table"][0]["flags"] & capture.RUN_CONTINUES).any() and len(cut["expect"][1]["table"][0]) == 1
    a, b = RC.restate(cut, cut["sizes"], measure=RC.MEASURES), RC.restate(whole, whole["sizes"], measure=RC.MEASURES)
    for m in RC.MEASURES + ("sync",):  # (the sync: a span of 28, so that the 895-sample runs have their matches)
        got, want = RC.merged(m, [e[m] for e in a]), RC.merged(m, [e[m] for e in b])
        RC.same_chains(m, got, want, "cut at the run's end")
        assert len(got) == 3 and not any(int(c["flags"]) & capture.RUN_OPEN for c in got)
    assert all(int(c["n_hits"]) > 0 for c in RC.merged("sync", [e["sync"] for e in a]))
    # a restart's chain, and one behind the last submit, stay OPEN: what lies behind them is not known
    kept = envelope.chains([a[0]["envelope"]]) + envelope.chains([e["envelope"] for e in a], restarts={1: [0, 1]})[:2]
    assert all(int(c["flags"]) & capture.RUN_OPEN for c in kept) and len(kept) == 4
    exe = str(tmp_path / "envelope_merge_driver")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(parity.ROOT, "tests", "merge_driver.cpp")])
    lines = ["file a.iq 2", "file b.iq 2"]
    for e in a:
        lines.append("batch 1 0 1")
        lines += [rec_line(int(r["stream"]), r) for r in e["envelope"]]
    out = subprocess.run([exe, "envelope"], input="".join(ln + "\n" for ln in lines), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    want = [envelope.line("ab"[int(c["stream"])] + ".iq", c) for c in envelope.chains([e["envelope"] for e in b])]
    assert sorted(out.stdout.splitlines()) == sorted(want) and len(want) == 3
    assert all(ln.split()[8] != "-" for ln in want)  # a ratio: the tail is whole


# ---- the campaign's own checks, on a model of the receiver
class ModelReceiver:
    """What recorder_campaign.run_plan reads of a channel-rate context, put together from the restatements.  plant: the name of
    one read whose result is returned with one bit wrong."""
    plant = None
    syncs = staticmethod(sync.syncs)
    mode_tracks = staticmethod(R.mode_tracks)
    inherit_wrong = False

    def __init__(self, n_streams, types_mask, thresh, filter_type, max_blocks, decimated, levels):
        assert decimated and levels
        n = self.n_streams = n_streams
        self.masks, self.thr, self.on, self.q = [types_mask] * n, [thresh] * n, set(), []
        self.cst, self.lst, self.base, self.prev, self.tst = [None] * n, [None] * n, [0] * n, [np.zeros(2, dtype=np.int16)] * n, None
        self.centres = [0] * n
        self.sync, self.sst, self.mode = None, None, None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        pass

    def configure_streams(self, streams, types_mask, thresh):
        for s, m, t in zip(streams, types_mask, thresh):
            self.masks[s], self.thr[s] = m, t

    def enable_capture(self, max_runs, max_samples):
        self._capture = (max_runs, max_samples)

    def enable_burst_meter(self):
        self.on.add("meter")

    def enable_burst_envelope(self):
        self.on.add("envelope")

    def enable_burst_clock(self):
        self.on.add("clock")

    def enable_burst_track(self, smooth):
        self.on.add("track")
        self.L = smooth

    def enable_burst_track_amplitude(self, smooth):
        self.enable_burst_track(smooth)
        self.mode = ("amplitude", [0] * self.n_streams)

    def enable_burst_track_auto(self, smooth, head=1024):
        self.enable_burst_track(smooth)
        self.mode = ("auto", head)

    def enable_burst_track_phase(self, smooth, head=1024, lag=1):
        self.enable_burst_track(smooth)
        self.mode = ("phase", head, lag)

    def set_burst_track_level(self, streams, level):
        assert self.mode[0] == "amplitude"
        for s, v in zip(streams, level):
            self.mode[1][s] = v

    def enable_burst_sync(self, rate, pattern, n_bits, max_errors=0, both=False):
        assert "track" in self.on
        self.sync = sync.Settings(rate, pattern, n_bits, max_errors, both)

    def set_burst_track_centre(self, streams, hz):
        for s, v in zip(streams, hz):
            self.centres[s] = v

    def reset_streams(self, streams):
        for s in streams:
            self.cst[s] = self.lst[s] = None
            self.base[s] = 0

    def submit(self, x):
        n, nb = self.n_streams, x.shape[1] // B
        decs = [decin.clamp(x[s]).reshape(-1) for s in range(n)]
        per, lev = [], []
        for s in range(n):
            runs, pool, self.cst[s] = capture.captures(decs[s], self.masks[s], self.thr[s], self.cst[s])
            rec, self.lst[s] = levels.levels(decs[s], self.masks[s], self.thr[s], self.lst[s])
            per.append((runs, pool))
            lev.append(rec)
        runs, pool = capture.table(per)
        mr, ms = self._capture
        thr = [np.repeat(v["thresh"].astype(np.int64), B) for v in lev]
        e = dict(decs=decs, runs=runs, pool=pool, levels=np.stack(lev), prefix=capture.prefix(runs, pool, mr, ms))
        if "meter" in self.on:
            e["meter"] = burst.bursts(decs, runs[:mr], self.prev, base=self.base)
        if "envelope" in self.on:
            e["envelope"] = envelope.envelopes(decs, thr, runs[:mr], self.prev, base=self.base)
        if "clock" in self.on:
            e["clock"] = clock.clocks(decs, runs[:mr], base=self.base)
        if "track" in self.on:
            cen, recs, words, own = self.mode_tracks(self.mode, decs, thr, runs[:mr], self.L, self.centres, self.tst, base=self.base,
                                                     max_samples=ms)
            self.tst = self.mode_tracks(self.mode, decs, thr, runs, self.L, self.centres, self.tst, base=self.base)[3]
            e["track"] = (recs, words[:(len(e["prefix"][1]) + 31) // 32])
            if cen is not None:  # the carried pairs and prior: the whole table's; the carried index: the delivered records'
                e["centres"] = cen
                if not self.inherit_wrong:
                    self.tst = (self.tst[0], own[1])
            if self.sync is not None:  # on the delivered records and the runs that fit, as the header's Bits paragraph states
                srecs, swords, self.sst = self.syncs(recs, e["track"][1], self.sync, self.sst, n, max_samples=ms)
                e["sync"] = (srecs, swords[:len(e["track"][1])])
        self.q.append(e)
        self.prev, self.base = [d.reshape(-1, 2)[-1] for d in decs], [v + nb * B for v in self.base]

    def _oldest(self, name, allow_overflow, samples=False):
        if not self.q:
            raise api.TfrecAmdError(api.E_STATE, "nothing undrained")
        e = self.q[0]
        if (len(e["runs"]) > self._capture[0] or (samples and len(e["pool"]) > self._capture[1])) and not allow_overflow:
            raise api.TfrecAmdError(api.E_OVERFLOW, "overflow")
        out = e["prefix"][:2] if name == "table" else e[name]
        if self.plant == name:
            first = (out[0] if isinstance(out, tuple) else out).copy()
            if first.size:
                first.view(np.uint8).reshape(-1)[-1] ^= 1
            out = (first,) + tuple(out[1:]) if isinstance(out, tuple) else first
        return e, out

    def read_captures(self, allow_overflow=False):
        e, out = self._oldest("table", allow_overflow, samples=True)
        self.capture_totals, self.capture_overflow = (len(e["runs"]), len(e["pool"])), e["prefix"][2]
        return out

    def read_levels(self):
        return self._oldest("levels", True)[1]

    def read_bursts(self, allow_overflow=False):
        e, out = self._oldest("meter", allow_overflow)
        self.burst_total = len(e["runs"])
        return out

    def read_burst_envelopes(self, allow_overflow=False):
        e, out = self._oldest("envelope", allow_overflow)
        self.envelope_total = len(e["runs"])
        return out

    def read_burst_clocks(self, allow_overflow=False):
        e, out = self._oldest("clock", allow_overflow)
        self.clock_total = len(e["runs"])
        return out

    def read_burst_tracks(self, allow_overflow=False):
        e, out = self._oldest("track", allow_overflow, samples=True)
        self.track_total = len(e["runs"])
        return out

    def read_burst_track_centres(self, allow_overflow=False):
        e, out = self._oldest("centres", allow_overflow)
        self.centre_total = len(e["runs"])
        return out

    def read_burst_syncs(self, allow_overflow=False):
        e, out = self._oldest("sync", allow_overflow, samples=True)
        self.sync_total = len(e["runs"])
        return out

    def decimated(self, s, n_pairs):
        return self.q[-1]["decs"][s]

    def drain(self):
        self.q.pop(0)


def planted(name):
    return type("Planted", (ModelReceiver,), {"plant": name})


# ---- a sync that is wrong in one place, where a kernel could be wrong by one: the campaign notices each on the model
WRONG = {  # the mistake -> one of the fixed seeds whose campaign meets it
    "edge": 35,           # the first defined sample, k + H == span, taken for undefined
    "clamp": 91,          # 2046 bits carried where 2047 are available
    "short-open": 91,     # an OPEN piece shorter than 2047 samples leaves its bits with the oldest 31 of them lost
    "unfit-history": 35,  # a run that does not fit max_samples leaves a history behind it
    "tie": 21,            # under BOTH, the word and its complement equally near: best_at from the word's samples alone
    "last-minimum": 35}   # best_at: the last sample that has the smallest distance


def wrong_syncs(trecs, twords, st, state=None, n_streams=None, max_samples=None, wrong=None):
    """sync.syncs written out once more, on recorder_campaign._distances, with one place to be wrong at (wrong=None: nowhere)."""
    state = sync.fresh_state(n_streams) if state is None else state
    keep = sync.HISTORY - (wrong == "clamp")
    out, ms, nxt = np.zeros(len(trecs), dtype=sync.SYNC_DTYPE), [], sync.fresh_state(n_streams)
    for e, r in enumerate(trecs):
        s, n, cont = int(r["stream"]), int(r["n_samples"]), int(r["flags"]) & capture.RUN_CONTINUES
        o, m, fits = sync._copied(r), np.zeros(n, dtype=np.uint8), sync._fits(r, max_samples)
        h = np.asarray(state["bits"][s], dtype=np.uint8)[-keep:] if cont else np.zeros(0, dtype=np.uint8)
        t = track.bits_of(r, twords) if fits else np.zeros(n, dtype=np.uint8)
        if fits:
            k0, d = RC._distances(st, h, t)
            if wrong == "edge" and k0 > 0:
                k0, d = k0 + 1, d[1:]
            if len(d):
                hit = (d <= st.E) | (st.both & (d >= st.P - st.E))
                m[k0:] = hit
                f = np.minimum(d, st.P - d) if st.both else d
                cand = np.flatnonzero(f == f.min())
                if wrong == "tie" and st.both:
                    cand = np.flatnonzero(d == d.min()) if d.min() <= st.P - d.max() else np.flatnonzero(d == d.max())
                at = cand[-1] if wrong == "last-minimum" else cand[0]
                o["n_hits"], o["best"], o["best_at"] = int(np.count_nonzero(hit)), int(f.min()), k0 + int(at)
        if int(r["flags"]) & capture.RUN_OPEN and (fits or wrong == "unfit-history"):
            nxt["bits"][s] = np.concatenate([h, t])[-keep:]
            if wrong == "short-open" and n < sync.HISTORY:  # (such a piece does not continue a chain: an OPEN piece that does is a whole submit)
                nxt["bits"][s][:31] = 0
        out[e] = o
        ms.append(m)
    return out, track._pack(out, ms, max_samples), nxt


def mistaken(wrong):
    return type("Mistaken", (ModelReceiver,), {"syncs": staticmethod(functools.partial(wrong_syncs, wrong=wrong))})


def test_the_sync_written_out_once_more_is_the_restatement(capsys):
    assert sum(RC.campaign(seed, RC.ROUNDS, verbose=False, receiver=mistaken(None)) for seed in sorted(set(WRONG.values()))) == 0
    assert capsys.readouterr().out == ""


@pytest.mark.parametrize("wrong", sorted(WRONG))
def test_the_campaign_notices_a_sync_that_is_wrong_in_one_place(wrong, capsys):
    assert WRONG[wrong] in RC.SEEDS and RC.campaign(WRONG[wrong], RC.ROUNDS, verbose=False, receiver=mistaken(wrong)) >= 1
    assert "MISMATCH" in capsys.readouterr().out


def test_the_campaign_passes_on_a_model_of_the_receiver_and_notices_a_planted_bit(capsys):
    seed, rounds = RC.SEEDS[0], 6
    assert RC.campaign(seed, rounds, verbose=False, receiver=ModelReceiver) == 0
    assert capsys.readouterr().out == ""
    for name in ("table", "levels") + RC.MEASURES + ("sync",):
        ps = RC.plans(seed, rounds)
        uses = sum(1 for p in ps if name in ("table", "levels") or name in p["measure"] or (name == "sync" and p["sync"] is not None))
        bad = RC.campaign(seed, rounds, verbose=False, receiver=planted(name))
        assert 1 <= bad <= uses, name
        out = capsys.readouterr().out
        assert out.count("MISMATCH") == bad and "seed %d round" % seed in out and "streams" in out, out


# ---- the track's modes in the campaign
@functools.lru_cache(maxsize=None)
def mode_plans():
    return [p for seed in RC.MODE_SEEDS for p in RC.plans(seed, RC.ROUNDS, modes=True)]


@functools.lru_cache(maxsize=None)
def mode_hits():
    hit = set()
    for p in mode_plans():
        hit |= RC.mode_classes_hit(p)
    return hit


@pytest.mark.parametrize("label", RC.MODE_CLASSES)
def test_the_mode_seeds_reach_every_mode_class(label):
    assert label in mode_hits()


def test_the_mode_rounds_draw_their_settings_and_leave_the_old_seeds_alone():
    assert 4 <= len(RC.MODE_SEEDS) <= 6 and not set(RC.MODE_SEEDS) & set(RC.SEEDS)
    assert all(p["mode"] is None for p in fixed_plans())  # the six old seeds stay in frequency mode (their digests: above)
    ps = mode_plans()
    assert [p["mode"][0] for p in ps] == ["amplitude", "auto", "phase"] * (len(ps) // 3) and all("track" in p["measure"] for p in ps)
    with_sync = [p for p in ps if p["sync"] is not None]
    assert len(ps) // 3 < len(with_sync) < 5 * len(ps) // 6 and {p["mode"][0] for p in with_sync} == {"amplitude", "auto", "phase"}
    Ks = [p["mode"][1] for p in ps if p["mode"][0] != "amplitude"]
    lags = [p["mode"][2] for p in ps if p["mode"][0] == "phase"]
    assert {64, 4096} <= set(Ks) and any(66 < K < 4096 for K in Ks) and {1, 64} <= set(lags) and any(1 < m < 64 for m in lags)
    assert any((p["L"], p["mode"][2]) == (16, 64) for p in ps if p["mode"][0] == "phase")
    lv = [(v, t) for p in ps if p["mode"][0] == "amplitude" for v, t in zip(p["mode"][1], p["thresh"])]
    assert {0, 65535, 3000, 2999} <= {v for v, _ in lv} and any(v == t for v, t in lv)
    assert {-192000, 0, 192000} <= {c for p in ps if p["mode"][0] != "amplitude" for c in p["centres"]}
    assert all(" mode %s " % p["mode"][0] in RC.describe(p) for p in ps)
    kinds = np.random.default_rng(1)  # the default call paints what it painted: the extra kinds are drawn only where they are asked for
    assert RC.rows(kinds, 2, 2, [694, 356], cuts=(1,), extra=()).tobytes() == RC.rows(np.random.default_rng(1), 2, 2, [694, 356], cuts=(1,)).tobytes()


def test_at_most_a_quarter_of_the_auto_and_phase_chains_are_exempt_from_the_merged_check():
    """A chain whose first piece begins fewer than K samples ahead of a cut and reaches it has a shorter head than the uncut run:
    run_plan compares its flags and length alone.  The condition, counted on the plans."""
    counts = [RC.exempt_counts(p) for p in mode_plans()]
    ex, chains = sum(c[0] for c in counts), sum(c[1] for c in counts)
    assert sum(1 for c in counts if c[1]) >= 6 and ex >= 1 and 4 * ex <= chains, (ex, chains)


def test_there_is_a_tie_in_the_carrier_search_and_the_smaller_index_wins():
    ties = RC.tie_pairs()
    assert len(ties) == 1048 and ties[-1][2] == (0, 4095)
    for i, q, (r0, r1) in ties[:3] + ties[-3:]:
        for g in (1, 200 * 64):
            assert track.carrier_index(g * i, g * q) == track.carrier_index_bruteforce(g * i, g * q) == r0 < r1


def mode_brute_equals_fast(x, masks, thresh, sizes, L, centres, mode, first=None):
    """brute_equals_fast for a mode: amplitude_tracks, head_centres and tracks about them, head_carriers and phase_tracks against
    their per-sample forms, submit by submit, the carried state included."""
    n, dec = len(x), decin.clamp(x)
    mode = (mode[0], mode[1][:n]) if mode[0] == "amplitude" else mode  # (a level per stream)
    cst, lst, fast, brute, pos, base, total = [None] * n, [None] * n, None, None, 0, [0] * n, 0
    for nb in sizes:
        decs = [np.ascontiguousarray(dec[s, pos * B:(pos + nb) * B]).reshape(-1) for s in range(n)]
        per, thr = [], []
        for s in range(n):
            runs, pool, cst[s] = capture.captures(decs[s], masks[s], thresh[s], cst[s])
            lev, lst[s] = levels.levels(decs[s], masks[s], thresh[s], lst[s])
            per.append((runs, pool))
            thr.append(np.repeat(lev["thresh"].astype(np.int64), B))
        table = capture.table(per)[0][:first]
        a = R.mode_tracks(mode, decs, thr, table, L, centres, fast, base=base)
        b = R.mode_tracks(mode, decs, thr, table, L, centres, brute, base=base, brute=True)
        if a[0] is not None:
            RC.same_records(a[0], b[0], "centres")
        RC.same_records(a[1], b[1], "tracks")
        assert np.array_equal(a[2], b[2]), "words"
        fast, brute = a[3], b[3]
        for u, v in zip(fast if isinstance(fast, tuple) else (fast,), brute if isinstance(brute, tuple) else (brute,)):
            assert sorted(u) == sorted(v) and all(np.array_equal(u[f], v[f]) for f in u), "the carried state"
        total += len(table)
        pos, base = pos + nb, [v + nb * B for v in base]
    return total


MODES = (("amplitude", [3000, 100]), ("auto", 128), ("phase", 128, 7))


@pytest.mark.parametrize("mode", MODES, ids=lambda m: m[0])
def test_the_fast_mode_restatements_equal_the_per_sample_ones_on_a_generated_round(mode):
    rng = np.random.default_rng(RC.MODE_SEEDS[0])
    masks, sizes = [0x2F, 0x02], (1, 1)
    x = RC.rows(rng, 2, 2, [RC.window(m) for m in masks], cuts=(1,), extra=RC.MODE_KINDS)
    assert mode_brute_equals_fast(x, masks, [RC.T, 90], sizes, 7, [20000, -192000], mode) >= 10


@pytest.mark.parametrize("mode", MODES, ids=lambda m: m[0])
def test_the_fast_mode_restatements_equal_the_per_sample_ones_on_the_dense_rows_first_40_runs(mode):
    assert mode_brute_equals_fast(RC.dense_heads(2, (1, 4, 7))[None], [0x02], [RC.T], (2,), 16, [35000], mode, first=40) == 40


# ---- a mode's restatement that is wrong in one place, where a kernel could be wrong by one
MODE_WRONG = {  # the mistake -> what it is; a seed of MODE_SEEDS notices each
    "head:K+1": "the head takes one product too many (k <= nh)",
    "count:>64": "P > 64 instead of P >= 64",
    "occ:floor": "a bin is occupied from P // 16 on",
    "mask:one-sample": "only the later sample's over bit is tested",
    "wrap:unsigned": "lo and hi are taken without the rotation by 32",
    "zero-sums:measured": "sums of (0, 0) are measured: no candidate has a positive score, index 0 stays",
    "tie:larger-r": "of two candidates with equal |cross| the larger index is kept",
    "lag:edge": "k - cf <= lag is taken for undefined",
    "prior:ignored": "cf = the run's start in a continuing piece",
    "inherit:after-overflow": "an index is carried from an OPEN entry that had no record",
    "amp:>=": "sum >= L * level",
    "amp:prior": "a continuing piece's prior is taken one too small: the power of the chain's first sample is dropped"}
# prior:79 -- the phase track's prior clamped at 79 -- cannot be noticed in what a context returns: a product at k' >= -(L - 1) of a
# continuing piece is defined iff k' + prior >= m, and with L + m <= 80 both 79 and 80 define every one of them.  In the same way
# the amplitude track's prior of 16 taken as 15 defines every power L <= 16 reaches; amp:prior is therefore the mistake one step on


def wrong_mode_tracks(mode, decs, thr, runs, L, centres, state=None, base=None, max_samples=None, brute=False, wrong=None):
    """recorder.mode_tracks for the three modes written out once more, entry by entry on definedness masks, with one place to be
    wrong at (wrong=None: nowhere)."""
    if mode is None:
        return R.mode_tracks(mode, decs, thr, runs, L, centres, state, base, max_samples)
    name, n = mode[0], len(decs)
    heads, ahead = name != "amplitude", track.PHASE_AHEAD if name == "phase" else track.AHEAD
    tst, cst = (state if state is not None else (None, None)) if heads else (state, None)
    tst = tst if tst is not None else {"carry": np.zeros((n, ahead, 2), dtype=np.int16), "prior": np.zeros(n, dtype=np.int64)}
    cst = cst if cst is not None else track.fresh_centre_state(n)
    tc, ts = (t.astype(np.int64) for t in tune.table())
    index_of = lambda hz: (8192 * hz + 384000) // 768000 % 4096  # noqa: E731
    out, tr = np.zeros(len(runs), dtype=track.TRACK_DTYPE), []
    cen = np.zeros(len(runs), dtype=track.CENTRE_DTYPE) if heads else None
    for e, r in enumerate(runs):
        s, a, nn, cont = track._window(decs, r, base)
        z = burst._pairs(decs[s]).astype(np.int64)
        over = envelope._over(z, thr[s])
        prior = int(tst["prior"][s]) if cont else 0
        if heads:  # ---- the entry's centre
            o, K, fb = track._centre_copied(r), mode[1], int(centres[s])
            src, hz, dev, cnt, idx = track.FALLBACK, fb, 0, 0, index_of(fb)
            if cont:
                if int(cst["index"][s]) >= 0:
                    src, hz, idx = track.INHERITED, int(cst["centre_hz"][s]), int(cst["index"][s])
            else:
                nh = min(min(nn, K) + (wrong == "head:K+1"), len(z) - a)
                zz, ov = z[a:a + nh], over[a:a + nh]
                both = ov[1:] & (ov[:-1] | (wrong == "mask:one-sample"))
                dot, crs = (zz[1:, 0] * zz[:-1, 0] + zz[1:, 1] * zz[:-1, 1])[both], (zz[1:, 1] * zz[:-1, 0] - zz[1:, 0] * zz[:-1, 1])[both]
                cnt = len(dot)
                if cnt > track.COUNT_MIN - (wrong != "count:>64"):
                    if name == "auto":
                        h = np.bincount(burst._bins(dot, crs), minlength=burst.N_BINS)
                        occ = np.flatnonzero(h >= (cnt // 16 if wrong == "occ:floor" else (cnt + 15) // 16))
                        if wrong != "wrap:unsigned":
                            occ = np.where(occ < burst.N_BINS // 2, occ, occ - burst.N_BINS)
                        if len(occ):
                            src, hz, dev = track.MEASURED, 3000 * int(occ.min() + occ.max()), 3000 * int(occ.max() - occ.min())
                            idx = index_of(hz)
                    else:
                        A, Bs = int(dot.sum()), int(crs.sum())
                        if A or Bs or wrong == "zero-sums:measured":
                            cross = np.where(A * tc + Bs * ts > 0, np.abs(Bs * tc - A * ts), np.iinfo(np.int64).max)
                            best = np.flatnonzero(cross == cross.min())
                            idx = int(best[-1] if wrong == "tie:larger-r" else best[0])
                            src, hz = track.MEASURED, track.carrier_hz(idx)
            o["n_counted"], o["source"], o["centre_hz"], o["deviation_hz"], o["index"] = cnt, src, hz, dev, idx
            cen[e] = o
        # ---- the entry's track: the terms at k = -(L - 1) .. nn - 1, run-relative, each with whether it is defined
        ext = np.concatenate([np.asarray(tst["carry"][s], dtype=np.int64).reshape(ahead, 2), z])
        k = np.arange(-(L - 1), nn)
        at = a + k + ahead
        if name == "amplitude":
            val, first, limit = np.abs(ext[at, 0]) + np.abs(ext[at, 1]), int(wrong == "amp:prior" and cont), L * int(mode[1][s])
        else:
            m = mode[2] if name == "phase" else 1
            first = m + (wrong == "lag:edge" and name == "phase")
            prior = 0 if wrong == "prior:ignored" and name == "phase" else prior
            lo = np.maximum(at - m, 0)  # (a harmless index where the term is not defined)
            I, Q, Ip, Qp = ext[at, 0], ext[at, 1], ext[lo, 0], ext[lo, 1]
            if name == "phase":
                rm = idx * m % 4096
                val = (I * Ip + Q * Qp) * tc[rm] + (Q * Ip - I * Qp) * ts[rm]
            else:
                val = (Q * Ip - I * Qp) * tc[idx] - (I * Ip + Q * Qp) * ts[idx]
            limit = 0
        cs = np.concatenate([[0], np.cumsum(np.where(k + prior >= first, val, 0))])
        sums = cs[L:] - cs[:-L]
        t = sums >= limit if wrong == "amp:>=" else sums > limit
        o = track._copied(r)
        w = np.flatnonzero(over[a:a + nn])
        o["last_over"], o["n_ones"] = int(w[-1]) if len(w) else -1, int(np.count_nonzero(t))
        out[e] = o
        tr.append(t.astype(np.uint8))
    nxt = {"carry": np.array([burst._pairs(d)[-ahead:] for d in decs], dtype=np.int16), "prior": np.zeros(n, dtype=np.int64)}
    for r in runs:
        if int(r["flags"]) & capture.RUN_OPEN:
            s = int(r["stream"])
            nxt["prior"][s] = min(ahead, (int(tst["prior"][s]) if int(r["flags"]) & capture.RUN_CONTINUES else 0) + int(r["n_samples"]))
    return cen, out, track._pack(out, tr, max_samples), (nxt, track._next_centre_state(n, cen)) if heads else nxt


def mode_mistaken(wrong):
    return type("Mistaken", (ModelReceiver,), {"mode_tracks": staticmethod(functools.partial(wrong_mode_tracks, wrong=wrong)),
                                               "inherit_wrong": wrong == "inherit:after-overflow"})


def test_the_modes_written_out_once_more_are_the_restatements(capsys):
    assert sum(RC.campaign(seed, RC.ROUNDS, verbose=False, receiver=mode_mistaken(None), modes=True) for seed in RC.MODE_SEEDS) == 0
    assert capsys.readouterr().out == ""


@pytest.mark.parametrize("wrong", sorted(MODE_WRONG))
def test_the_mode_campaign_notices_a_mode_that_is_wrong_in_one_place(wrong, capsys):
    assert any(RC.campaign(seed, RC.ROUNDS, verbose=False, receiver=mode_mistaken(wrong), modes=True) for seed in RC.MODE_SEEDS)  # (the first is enough)
    assert "MISMATCH" in capsys.readouterr().out


def test_the_mode_campaign_passes_on_a_model_of_the_receiver_and_notices_a_planted_bit(capsys):
    assert sum(RC.campaign(seed, RC.ROUNDS, verbose=False, receiver=ModelReceiver, modes=True) for seed in RC.MODE_SEEDS) == 0
    assert capsys.readouterr().out == ""
    seed = RC.MODE_SEEDS[0]
    ps = RC.plans(seed, RC.ROUNDS, modes=True)
    for name, uses in (("centres", sum(1 for p in ps if p["mode"][0] != "amplitude")), ("track", len(ps))):
        bad = RC.campaign(seed, RC.ROUNDS, verbose=False, receiver=planted(name), modes=True)
        assert 1 <= bad <= uses and (name != "track" or bad >= 3), (name, bad)  # (the track: in each of the three modes)
        out = capsys.readouterr().out
        assert out.count("MISMATCH") == bad and " mode " in out, out
