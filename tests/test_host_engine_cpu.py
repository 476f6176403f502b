"""The pure pieces of tfrec_gpu's engine (tfrec_amd/host/job.h) without a GPU: the -n planner, the far / near tune split under -r and
the grouping of -A's hits into channels.  tests/host_engine_driver.cpp puts them behind a text interface; it is compiled here with
the address and undefined-behaviour sanitizers, links nothing of the device library and runs as a child process.
"""
import os
import random
import subprocess

import pytest

from tfrec_amd import occupancy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DFLT = (0x2F, 500, 0)  # the context's -T, -t, -W


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("host_engine") / "host_engine_driver")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(ROOT, "tests", "host_engine_driver.cpp")])

    def run(cmd, lines):
        out = subprocess.run([exe, cmd], input="".join(ln + "\n" for ln in lines), capture_output=True, text=True, timeout=120)
        assert out.returncode == 0 and not out.stderr, out.stderr  # (a sanitizer report goes to stderr and fails the run)
        assert "bad case" not in out.stdout
        return out.stdout.splitlines()
    return run


def plan_cases():
    """A few hundred seeded jobs -> (nslots, bps, files), files: [(blocks, T, t, W, tune)].  Every fourth runs without -n: as many slots
    as files."""
    rng = random.Random(20)
    cases = []
    for i in range(320):
        configs = rng.sample([DFLT, (0x01, 500, 0), (0x2F, 0, 1), (0x06, 300, 0)], rng.choice((2, 3)))
        tunes = rng.sample([0, 25000, -300000, 700000], rng.choice((2, 3)))
        files = [(rng.choice((0, 0, 1, 2, 3)) if rng.random() < 0.3 else rng.randint(0, 40),) + rng.choice(configs) + (rng.choice(tunes),)
                 for _ in range(rng.randint(1, 12))]
        cases.append((len(files) if i % 4 == 0 else rng.randint(1, 4), rng.randint(1, 16), files))
    return cases


def parse_plans(lines, n_cases):
    """The driver's text -> per case a list of batches {nb, file, reset, conf: {slot: (T, t, W)}, tune: {slot: hz}}."""
    plans, at = [], 0
    for _ in range(n_cases):
        head = lines[at].split()
        assert head[0] == "plan"
        batches = []
        for ln in lines[at + 1:at + 1 + int(head[1])]:
            nb, file, reset, conf, tune = ln[2:].split(";")
            assert ln.startswith("b ")
            batches.append(dict(nb=int(nb), file=[int(v) for v in file.split()], reset=[int(v) for v in reset.split()],
                                conf={int(c.split(":")[0]): tuple(int(v) for v in c.split(":")[1:]) for c in conf.split()},
                                tune={int(t.split(":")[0]): int(t.split(":")[1]) for t in tune.split()}))
        plans.append(batches)
        at += 1 + int(head[1])
    assert at == len(lines)
    return plans


def check_plan(nslots, bps, files, plan):
    where = {}  # file -> [(batch, slot)]
    for k, b in enumerate(plan):
        assert len(b["file"]) == nslots and len(set(b["reset"])) == len(b["reset"])
        for s, f in enumerate(b["file"]):
            assert -1 <= f < len(files)
            if f >= 0:
                where.setdefault(f, []).append((k, s))
    live = [f for f, x in enumerate(files) if x[0] >= 1]
    assert sorted(where) == live  # every file with a block appears, a file of 0 blocks nowhere
    for f in live:  # on one slot, in consecutive batches that just hold its blocks
        ks, slots = [k for k, _ in where[f]], set(s for _, s in where[f])
        assert len(slots) == 1 and ks == list(range(ks[0], ks[0] + len(ks)))
        nbs = [plan[k]["nb"] for k in ks]
        assert sum(nbs) >= files[f][0] > sum(nbs[:-1])
    starts = [where[f][0] for f in live]
    assert starts == sorted(starts)  # files start in command-line order, on the free slots in order
    done = dict.fromkeys(live, 0)
    for k, b in enumerate(plan):
        most = max(files[f][0] - done[f] for f in b["file"] if f >= 0)
        assert 1 <= b["nb"] <= bps and b["nb"] == min(bps, most)  # bps blocks unless no stream needs that many
        if -1 in b["file"]:
            assert all(where[f][0][0] <= k for f in live)  # a slot stays empty only when no file waits
        for f in b["file"]:
            if f >= 0:
                done[f] += b["nb"]
    before = {}  # slot -> the settings it ran last
    for f in live:
        k, s = where[f][0]
        b = plan[k]
        T, t, W, tune = files[f][1:]
        first = s not in before
        has = before.get(s, DFLT + (0,))
        assert (s in b["conf"]) == ((T, t, W) != has[:3]) and (s in b["tune"]) == (tune != has[3])
        if s in b["conf"]:
            assert b["conf"][s] == (T, t, W)
        if s in b["tune"]:
            assert b["tune"][s] == tune
        # the first file of a slot is never reset; a later one is reset exactly when nothing of its settings changes
        assert (s in b["reset"]) == (not first and (T, t, W, tune) == has)
        before[s] = (T, t, W, tune)
    for k, b in enumerate(plan):  # ... and nothing is reset, configured or tuned but a slot that starts a file in that batch
        begins = set(where[f][0][1] for f in live if where[f][0][0] == k)
        assert set(b["reset"]) | set(b["conf"]) | set(b["tune"]) <= begins
    if nslots == len(files):  # the run without -n
        assert all(where[f][0][0] == 0 for f in live) and not any(b["reset"] for b in plan)


def test_plan_batches_on_seeded_jobs(driver):
    cases = plan_cases()
    lines = ["%d %d %d %d %d %d " % ((nslots, bps) + DFLT + (len(files),)) + " ".join("%d %d %d %d %d" % f for f in files)
             for nslots, bps, files in cases]
    plans = parse_plans(driver("plan", lines), len(cases))
    for (nslots, bps, files), plan in zip(cases, plans):
        check_plan(nslots, bps, files, plan)
    # the cases reach what the checks are about
    assert any(b["reset"] for p in plans for b in p) and any(b["conf"] for p in plans for b in p)
    assert any(b["tune"] for p in plans for b in p) and any(b["nb"] < c[1] for c, p in zip(cases, plans) for b in p)
    assert any(x[0] == 0 for c in cases for x in c[2]) and any(-1 in b["file"] for p in plans for b in p)


def test_tune_split_follows_the_written_rule(driver):
    """gpu_engine.h (set_rate) and DESIGN.md 6g: an offset of 768 kHz or more is the input-rate tune, a smaller one the tune behind the
    resampler; a stream that changes kind has the other kind cleared to 0 in the same step, and one that never had a kind is never
    sent a clear for it."""
    got = driver("tunes", ["new 2",
                           "0 300000",    # near: nothing to clear ahead of the resampler
                           "0 1100000",   # far: the near tune is cleared
                           "0 -200000",   # near again: the input-rate tune is cleared
                           "0 0",         # back to the centre: a near tune of 0, no input-rate tune left to clear
                           "0 -900000",   # far: no near tune left to clear
                           "1 767999 0 768000",  # the edge, and two streams in one batch: stream 0 was far and stays far
                           "1 -768000",   # stream 1 goes from near to far
                           "new 1", "0 800000", "0 0"])  # a stream that starts far never had a near tune to clear
    assert got == ["0:300000;", "0:0;0:1100000", "0:-200000;0:0", "0:0;", ";0:-900000", "1:767999;0:768000", "1:0;1:-768000",
                   ";0:800000", "0:0;0:0"]


def channel_cases():
    """(hits, records, n_bins, fs_in, center_khz, join_hz)"""
    cases = []
    # N = 64 at 1.536 MS/s: bins of 24 kHz, join 48 kHz = exactly two empty bins
    h = [0] * 64
    for b, v in ((-32, 3), (-31, 5), (-10, 4), (-7, 2), (-3, 1), (1, 6), (2, 7), (3, 10), (4, 2), (30, 1), (31, 4)):
        h[b % 64] = v  # groups at both edges; -10 and -7 two bins apart (joined), -3 three from -7 (not); a carrier (3) inside 1 .. 4
    cases.append((h, 16, 64, 1536000, 868250, 48000))
    cases.append((h, 16, 64, 1536000, 868250, 47999))  # one Hz less: -10 and -7 part
    cases.append((h, 16, 64, 1536000, 868250, 0))
    rng = random.Random(12)
    for n, fs in ((64, 2048000), (1024, 2400000), (1024, 15360000)):
        for _ in range(6):
            records = rng.randint(1, 40)
            hits = [rng.randint(0, records) if rng.random() < 0.08 else 0 for _ in range(n)]
            hits[n // 2] = rng.randint(0, records)  # the lowest bin, and the highest
            hits[n // 2 - 1] = rng.randint(0, records)
            cases.append((hits, records, n, fs, rng.choice((868250, 100, 433920)), rng.choice((0, 10000, 50000, 200000))))
    return cases


def test_occupancy_channels_equal_the_restatement(driver):
    cases = channel_cases()
    out = driver("channels", ["%d %d %d %d %d " % c[1:] + " ".join(map(str, c[0])) for c in cases])
    got, cur = [], []
    for ln in out:
        if ln == "end":
            got.append(cur)
            cur = []
        else:
            cur.append(tuple([ln.split()[0]] + [int(v) for v in ln.split()[1:]]))
    assert len(got) == len(cases) and not cur
    for c, g in zip(cases, got):
        want = [("carrier", w["khz"], w["bin"], w["hits"]) if w["kind"] == "carrier" else
                ("found", w["khz"], w["lo"], w["hi"], w["hits"], int(w["in_range"])) for w in occupancy.channels(*c)]
        assert g == want, c[1:]
    spans = lambda g: [(x[2], x[3]) for x in g if x[0] == "found"]  # noqa: E731
    assert spans(got[0]) == [(-32, -31), (-10, -7), (-3, -3), (1, 4), (30, 31)] and ("carrier", 868250 + 72, 3, 10) in got[0]
    assert (-10, -10) in spans(got[1]) and (-7, -7) in spans(got[1])
    assert any(x[0] == "found" and not x[5] for g in got for x in g) and any(len(g) > 3 for g in got[3:])
