"""The squelched recorder on the GPU (tfrec_amd_enable_capture, tfrec_amd_read_captures, tfrec_gpu -S), bit for bit.

The run table and the pool are compared with the restatement tfrec_amd/capture.py run on the context's OWN decimated samples
(tfrec_amd_read_decimated), so the front end ahead of the recorder is whatever the context runs; the events still equal the
oracle's.  The scene (recorder_rows.scene), eight streams of four blocks, is aimed on the CPU (the oracle's front end is the context's, bit for bit) at
the layouts the kernels can get wrong; every aim is asserted again on what the context returned.

  0  near-silence: no run, an empty entry in the scan over the streams
  1  a burst whose run starts at bit 63 of a mask word, and crosses the boundary between blocks 1 and 2
  2  TFA_2 alone (W = 356): a burst whose run ends at bit 0 of a mask word
  3, 4, 5  a burst that begins 1, 3 and 5 samples ahead of the input's end: open runs of those lengths
  6  auto threshold, noise loud enough to move it: triggered throughout
  7  TFA_1 alone (W = 400) on stream 1's input
"""
import functools
import os
import subprocess

import numpy as np
import pytest

import parity
from oracle import oracle as O
from recorder import B, assert_tables, one_submit, receiver
from recorder_rows import CTX_TYPES, M, N, THRESH, TYPES, carrier, scene, want_tables
from tfrec_amd import api, capture, levels, resample, synth

pytestmark = pytest.mark.gpu


def test_table_and_pool_equal_the_restatement():
    got, want, ev, decs, th, states = one_submit()
    assert_tables(got, want)
    assert th == [st["thresh"] for st in states] and th[6] == 502 and th[:6] == [500] * 6  # the thresholds the front end ended with
    iq = scene()
    for s in range(N):
        parity.assert_stream(ev, s, parity.fresh_oracle(iq[s], TYPES[s], THRESH[s]), "stream %d" % s)


def test_the_scene_holds_the_layouts_it_is_aimed_at():
    (runs, pool), _, _, decs, _, _ = one_submit()
    of = lambda s: runs[runs["stream"] == s]  # noqa: E731
    end = lambda r: int(r["start_sample"] + r["n_samples"])  # noqa: E731
    assert len(of(0)) == 0 and len(of(1)) == 1 and runs["stream"].tolist() == sorted(runs["stream"].tolist())
    assert np.array_equal(runs["pool_offset"], np.concatenate([[0], np.cumsum(runs["n_samples"])[:-1]]).astype(np.uint64))
    r1, r2, r7 = of(1)[0], of(2)[0], of(7)[0]
    assert r1["start_sample"] % 64 == 63 and r1["start_sample"] < 2 * B < end(r1) and r1["flags"] == 0
    assert (end(r2) - 1) % 64 == 0 and len(of(2)) == 1
    assert r7["start_sample"] == r1["start_sample"] and r1["n_samples"] - r7["n_samples"] == 694 - 400  # each stream's own W
    for s, length in ((3, 1), (4, 3), (5, 5)):
        r = of(s)[-1]
        assert r["n_samples"] == length and end(r) == M and r["flags"] == capture.RUN_OPEN and len(of(s)) == 1
        d = decs[s].reshape(-1, 2)
        assert np.array_equal(pool[int(r["pool_offset"]):int(r["pool_offset"]) + length], d[M - length:])
    r6 = of(6)
    assert end(r6[-1]) == M and r6[-1]["flags"] == capture.RUN_OPEN and r6[-1]["n_samples"] >= M - 16 and r6[-1]["thresh"] == 500
    assert len({int(o) % 4 for o in runs["pool_offset"]}) > 1


@functools.lru_cache(maxsize=None)
def queued(sizes):
    """The scene cut into `sizes`, every submit queued before the first read -> [(table, pool)] per submit, events per submit."""
    parts = parity.cut(scene(), sizes)
    with receiver(max_blocks=max(sizes)) as r:
        for p in parts:
            r.submit(p)
        last = [r.decimated(s, sizes[-1] * B) for s in range(N)]
        got, evs = [], []
        for _ in parts:
            got.append(r.read_captures())
            evs.append(r.drain())
        with pytest.raises(api.TfrecAmdError) as e:
            r.read_captures()
        assert e.value.code == api.E_STATE
    return got, evs, last


def test_one_plus_three_queued_before_the_first_read():
    got, evs, last = queued((1, 3))
    whole, _, ev, decs, _, _ = one_submit()
    for s in range(N):  # the front end does not depend on the cut: the restatement may run on the uncut context's samples
        assert np.array_equal(last[s], decs[s][2 * B:])
    states, pos = [None] * N, 0
    for k, nb in enumerate((1, 3)):
        want = want_tables([d[2 * pos * B:2 * (pos + nb) * B] for d in decs], states)
        assert_tables(got[k], want, "submit %d" % k)
        pos += nb

    def samples(tabs):
        out = set()
        for runs, pool in tabs:
            for r in runs:
                o = int(r["pool_offset"])
                out |= {(int(r["stream"]), int(r["start_sample"]) + i, int(pool[o + i][0]), int(pool[o + i][1]))
                        for i in range(int(r["n_samples"]))}
        return out

    assert samples(got) == samples([whole])
    first6 = got[0][0][got[0][0]["stream"] == 6][-1]
    second6 = got[1][0][got[1][0]["stream"] == 6]
    assert first6["flags"] & capture.RUN_OPEN
    # stream 6 in the second submit: one run of the whole submit, continued and open
    assert len(second6) == 1 and second6[0]["flags"] == capture.RUN_CONTINUES | capture.RUN_OPEN
    assert second6[0]["start_sample"] == B and second6[0]["n_samples"] == 3 * B
    cont = np.concatenate([t[0] for t in got])
    assert (cont[cont["flags"] & capture.RUN_CONTINUES != 0]["stream"] == 6).all()
    assert parity.sort_events(np.concatenate(evs)).tobytes() == parity.sort_events(ev).tobytes()


def test_a_reset_between_submits_drops_the_carried_trigger():
    parts = parity.cut(scene(), (2, 2))
    states = [None] * N
    with receiver(max_blocks=2) as r:
        r.submit(parts[0])
        want0 = want_tables([r.decimated(s, 2 * B) for s in range(N)], states)
        got0 = r.read_captures()
        r.drain()
        r.reset_streams([1, 6])
        states[1] = states[6] = None  # fresh streams on the input that follows
        r.submit(parts[1])
        want1 = want_tables([r.decimated(s, 2 * B) for s in range(N)], states)
        got1 = r.read_captures()
        r.drain()
    assert_tables(got0, want0, "before the reset")
    assert_tables(got1, want1, "after the reset")
    runs0, runs1 = got0[0], got1[0]
    for s in (1, 6, 7):  # the runs of 1, 6 and 7 were open at the cut ...
        assert runs0[runs0["stream"] == s][-1]["flags"] & capture.RUN_OPEN
    # ... 7 carries on; 1 lost its trigger (what is left of the burst is quiet) and 6 starts again, from sample 0, not continued
    r7 = runs1[runs1["stream"] == 7][0]
    assert r7["flags"] & capture.RUN_CONTINUES and r7["start_sample"] == 2 * B
    assert len(runs1[runs1["stream"] == 1]) == 0
    r6 = runs1[runs1["stream"] == 6]
    assert not (r6["flags"] & capture.RUN_CONTINUES).any() and r6[0]["start_sample"] < 16 and r6[0]["thresh"] == 500
    assert int(r6[-1]["start_sample"] + r6[-1]["n_samples"]) == 2 * B


@pytest.mark.parametrize("short", ["runs", "samples"])
def test_overflow_delivers_a_prefix_and_the_next_submit_is_exact(short):
    (runs, pool), _, _, decs, _, _ = one_submit()
    cap = (len(runs) - 1, len(pool)) if short == "runs" else (len(runs), len(pool) - 1)
    states = [None] * N
    with receiver(cap=cap) as r:
        r.submit(scene())
        want = want_tables([r.decimated(s, M) for s in range(N)], states)
        with pytest.raises(api.TfrecAmdError) as e:
            r.read_captures()
        assert e.value.code == api.E_OVERFLOW
        got = r.read_captures(allow_overflow=True)
        assert r.capture_overflow and r.capture_totals == (len(want[0]), len(want[1])) == (len(runs), len(pool))
        wr, wp, ov = capture.prefix(want[0], want[1], *cap)
        assert ov and len(wr) == len(runs) - 1  # whole runs only: the last run is missing either way
        assert_tables(got, (wr, wp), "the prefix")
        ev = r.drain()
        # the next submit -- one block, so that it fits -- captures normally, its CONTINUES flags included
        r.submit(scene()[:, :api.BLOCK_BYTES])
        want2 = want_tables([r.decimated(s, B) for s in range(N)], states)
        got2 = r.read_captures()
        assert not r.capture_overflow
        r.drain()
    assert_tables(got2, want2, "the submit behind the overflow")
    assert (got2[0]["flags"] & capture.RUN_CONTINUES).any()
    assert parity.sort_events(ev).tobytes() == parity.sort_events(one_submit()[2]).tobytes()  # the events do not notice


def test_with_levels_captured_is_triggered_and_telegrams_lie_inside_runs():
    n, nb = 4, 4
    iq = synth.gen_batch(5, 0, n, nb)
    with api.Receiver(n, CTX_TYPES, 500, 0, max_blocks=nb, all_flushes=True, levels=True) as r:
        r.enable_capture(4096, n * nb * B)
        r.submit(iq)
        runs, pool = r.read_captures()
        lv = r.read_levels()
        ev = r.drain()
    per_block = np.zeros((n, nb), dtype=np.int64)
    for x in runs:
        k = np.arange(int(x["start_sample"]), int(x["start_sample"] + x["n_samples"])) // B
        per_block[int(x["stream"])] += np.bincount(k, minlength=nb)
    assert per_block.tolist() == lv["triggered"].tolist() and per_block.sum() == len(pool) > 0
    tele = ev[ev["status"] == 1]
    assert len(tele) > 0
    for e in tele:
        mine = runs[runs["stream"] == e["stream"]]
        at = int(e["end_sample"]) - 1
        assert ((mine["start_sample"] <= at) & (at < mine["start_sample"] + mine["n_samples"])).any(), e
    for s in range(n):
        parity.assert_stream(ev, s, parity.fresh_oracle(iq[s], CTX_TYPES, 500), "stream %d" % s)


def check_plain(r, parts, types, thresh):
    """Submit by submit on a uniform context: the table against the restatement on its own samples -> pairs captured."""
    states, total = [None] * r.n_streams, 0
    for p in parts:
        nb = r.submit(p)
        per = []
        for s in range(r.n_streams):
            runs, pool, states[s] = capture.captures(r.decimated(s, nb * B), types, thresh, states[s])
            per.append((runs, pool))
        got = r.read_captures()
        assert_tables(got, capture.table(per))
        total += len(got[1])
        r.drain()
    return total


def test_a_rate_context_a_10x_context_and_a_serial_one():
    p, q, nb = 4, 3, 3
    row = synth.gen_scene(41, nb, [dict(proto=1, start=5000 * p, payload_seed=5, f0_hz=0, amp=60)], rate_mult=p).reshape(-1, 2)[::q]
    row = np.ascontiguousarray(row).reshape(1, -1)
    assert row.shape[1] == 2 * resample.input_samples(nb, p, q)
    with api.Receiver(1, CTX_TYPES, 500, 0, max_blocks=nb, input_rate=(p, q)) as r:
        r.enable_capture(256, nb * B)
        assert check_plain(r, [row], CTX_TYPES, 500) > 0
    iq10 = np.stack([synth.gen_stream(9, s, 1, rate_mult=10) for s in range(2)])
    with api.Receiver(2, CTX_TYPES, 100, 0, max_blocks=1, input_10x=True) as r:  # (-t 100: the block's noise floor triggers)
        r.enable_capture(256, 2 * B)
        assert check_plain(r, [iq10], CTX_TYPES, 100) > 0
    ser, want, ev, _, th, _ = one_submit(True)
    assert_tables(ser, want, "serial")
    assert ser[0].tobytes() == one_submit()[0][0].tobytes() and ser[1].tobytes() == one_submit()[0][1].tobytes()
    assert th == one_submit()[4]
    assert parity.sort_events(ev).tobytes() == parity.sort_events(one_submit()[2]).tobytes()


def test_without_the_call_nothing_is_held_and_the_read_is_refused():
    n, mb = 3, 5
    with api.Receiver(n, CTX_TYPES, 500, 0, max_blocks=mb) as r:
        plain = r.memory()
        for _ in range(2):
            with pytest.raises(api.TfrecAmdError) as e:
                r.read_captures()
            assert e.value.code == api.E_INVAL
            r.submit(scene()[:n])
        assert r.memory()["pinned_host_bytes"] == plain["pinned_host_bytes"]
        with pytest.raises(api.TfrecAmdError) as e:  # ... and after the first submit it cannot be turned on any more
            r.enable_capture(16, 1024)
        assert e.value.code == api.E_STATE
        r.drain()
        r.drain()
    # the memory of a context that never enabled it is what it was: the level meter's share is still the whole difference
    with api.Receiver(n, CTX_TYPES, 500, 0, max_blocks=mb, levels=True) as r:
        assert r.memory()["device_bytes"] - plain["device_bytes"] == api.FIFO_DEPTH * n * mb * 32 + n * 16
    with api.Receiver(n, CTX_TYPES, 500, 0, max_blocks=mb) as r:
        assert r.memory() == plain
        for bad in ((0, 1024), (16, 0)):
            with pytest.raises(api.TfrecAmdError) as e:
                r.enable_capture(*bad)
            assert e.value.code == api.E_INVAL
        r.enable_capture(16, 1024)
        with pytest.raises(api.TfrecAmdError) as e:
            r.enable_capture(16, 1024)
        assert e.value.code == api.E_INVAL
        m = r.memory()
        # per set the table, the pool and the totals; once the state, counts, bases and staged runs of every stream
        assert m["device_bytes"] - plain["device_bytes"] == api.FIFO_DEPTH * (16 * 32 + 1024 * 4 + 16) + n * (
            16 + 8 + 16 + (mb * B // 356 + 3) * 20)
        assert m["pinned_host_bytes"] == plain["pinned_host_bytes"]
        with pytest.raises(api.TfrecAmdError) as e:
            r.read_captures()
        assert e.value.code == api.E_STATE  # nothing undrained
        # the caller's room too small: E_INVAL, nothing written, the counts set
        r.submit(scene()[:n, :api.BLOCK_BYTES])
        nr, npairs = api.C.c_uint32(0), api.C.c_uint64(0)
        buf = np.full(32, 0x55, dtype=np.uint8)
        rc = r.L.tfrec_amd_read_captures(r.h, buf.ctypes.data, 0, api.C.byref(nr), None, 0, api.C.byref(npairs))
        runs, pool = r.read_captures()
        assert rc == api.E_INVAL and (buf == 0x55).all() and (nr.value, npairs.value) == (len(runs), len(pool)) and len(runs) == 1
        r.drain()


def test_a_failed_enable_leaves_the_context_as_it_was():
    """tfrec_amd_enable_capture that runs out of memory half way -- a pool of 4 TiB per set, past the SIZE_MAX guard and beyond any
    device's memory: hipMalloc returns its ordinary out-of-memory error -- gives back what it made: the memory totals are those
    from before the call, the recorder is off, and a later enable is a first one, whose recorder works."""
    def fresh():
        return api.Receiver(1, CTX_TYPES, 500, 0, max_blocks=1, levels=True)

    with fresh() as r:
        plain = r.memory()
        r.enable_capture(16, 1024)
        one_enable = r.memory()["device_bytes"] - plain["device_bytes"]
    assert one_enable > 0
    with fresh() as r:
        before = r.memory()
        assert before == plain
        with pytest.raises(api.TfrecAmdError) as e:
            r.enable_capture(16, 1 << 40)
        assert e.value.code == api.E_NOMEM
        assert r.memory() == before
        with pytest.raises(api.TfrecAmdError) as e:
            r.read_captures()
        assert e.value.code == api.E_INVAL
        r.enable_capture(16, 1024)
        m = r.memory()
        assert m["device_bytes"] - before["device_bytes"] == one_enable and m["pinned_host_bytes"] == before["pinned_host_bytes"]
        x = np.random.default_rng(23).integers(126, 131, api.BLOCK_BYTES, dtype=np.uint8)
        carrier(x, 4 * 3000, 4 * 3050)  # one run, the burst and the longest window behind it: it fits the pool
        assert 0 < check_plain(r, [x.reshape(1, -1)], CTX_TYPES, 500) <= 1024


def test_cli_capture_of_the_golden_tfa_2_scene(tmp_path):
    cli = parity.build_cli()
    z = np.load(os.path.join(parity.ROOT, "tests", "golden", "iq_tfa_2.npz"))
    nb = 3
    x = np.ascontiguousarray(z["iq"][:nb * api.BLOCK_BYTES])
    f = tmp_path / "tfa2.iq"
    x.tofile(f)
    pre = str(tmp_path / "cap")
    args = ["-T", "2f", "-t", "500", "-b", "2", "-L", str(f)]
    plain = subprocess.run([cli] + args, capture_output=True, text=True, timeout=300)
    out = subprocess.run([cli, "-S", pre] + args, capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0 and out.returncode == 0, out.stderr
    assert parity.telegram_lines(out.stdout) == parity.telegram_lines(plain.stdout) and len(parity.telegram_lines(out.stdout)) >= 1
    # the restatement: the oracle's front end, then capture.py submit by submit (-b 2: two blocks, then one)
    o = O.Oracle(0x2F, 500, 0, keep_dec=True)
    o.process(x)
    dec = o.dec().reshape(-1, 2)
    lines, pools, st = [], [], None
    for a, b in ((0, 2), (2, 3)):
        runs, pool, st = capture.captures(dec[a * B:b * B], 0x2F, 500, st)
        lines += [capture.idx_line(0, r) for r in runs]
        pools.append(pool)
    assert open(pre + ".idx").read().splitlines() == lines and len(lines) >= 1
    assert np.array_equal(np.fromfile(pre + ".0.cs16", dtype="<i2").reshape(-1, 2), np.concatenate(pools))


def test_cli_capture_is_the_same_across_contexts_and_slots(tmp_path):
    """-S of two files (the golden TFA_2 scene's first 3 blocks, and its first 2) with -b 2: as two streams of one context, as one
    stream each of two contexts (-d 0,0) and through one recycled stream (-n 1).  Per file the .idx lines -- without the stream
    column, which is the file's stream on its device -- and the .cs16 bytes are the same."""
    cli = parity.build_cli()
    z = np.load(os.path.join(parity.ROOT, "tests", "golden", "iq_tfa_2.npz"))
    paths = []
    for i, nb in enumerate((3, 2)):
        paths.append(str(tmp_path / ("f%d.iq" % i)))
        np.ascontiguousarray(z["iq"][:nb * api.BLOCK_BYTES]).tofile(paths[-1])
    got = []
    for name, extra in (("plain", []), ("two", ["-d", "0,0"]), ("slot", ["-n", "1"])):
        pre = str(tmp_path / name)
        out = subprocess.run([cli, "-S", pre, "-T", "2f", "-t", "500", "-b", "2"] + extra + ["-L", paths[0], "-L", paths[1]],
                             capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr
        idx = [ln.split() for ln in open(pre + ".idx").read().splitlines()]
        per_file = {}
        for f in (0, 1):
            cs = pre + ".%d.cs16" % f
            per_file[f] = ([ln[:1] + ln[2:] for ln in idx if ln[0] == str(f)], open(cs, "rb").read() if os.path.exists(cs) else None)
        assert set(ln[0] for ln in idx) <= {"0", "1"}
        got.append(per_file)
    assert got[1] == got[0] and got[2] == got[0]
    assert len(got[0][0][0]) >= 1 and got[0][0][1]
