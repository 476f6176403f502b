"""tests/recorder_campaign.py without a GPU: the generator is deterministic, the fixed seeds of tests/test_recorder_campaign_gpu.py
reach every edge class the campaign names (measured back from capture.captures on the generated rows, class by class) and every
class of the burst sync's (measured back from its restatement on the plans), the sync's settings leave the earlier seeds' plans as
they were, the restatements the kernels are held to equal their per-sample forms at those edges, and the campaign's own checks --
run against a model of the receiver put together from the restatements -- pass, notice one planted wrong bit, and notice a sync
that is wrong by one in each of the places where a kernel could be."""
import functools
import hashlib

import numpy as np
import pytest

import recorder_campaign as RC
from tfrec_amd import api, burst, capture, clock, decin, envelope, levels, sync, track

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

    def __init__(self, n_streams, types_mask, thresh, filter_type, max_blocks, decimated, levels):
        assert decimated and levels
        n = self.n_streams = n_streams
        self.masks, self.thr, self.on, self.q = [types_mask] * n, [thresh] * n, set(), []
        self.cst, self.lst, self.base, self.prev, self.tst = [None] * n, [None] * n, [0] * n, [np.zeros(2, dtype=np.int16)] * n, None
        self.centres = [0] * n
        self.sync, self.sst = None, None

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
            recs, words, _ = track.tracks(decs, thr, runs[:mr], self.L, self.centres, self.tst, base=self.base, max_samples=ms)
            self.tst = track.tracks(decs, thr, runs, self.L, self.centres, self.tst, base=self.base)[2]
            e["track"] = (recs, words[:(len(e["prefix"][1]) + 31) // 32])
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
