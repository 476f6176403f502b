"""The burst envelope on the GPU (tfrec_amd_enable_burst_envelope, tfrec_amd_read_burst_envelopes, tfrec_gpu -Q), bit
for bit.

The records are compared, byte for byte, with the restatement tfrec_amd/envelope.py run on the context's OWN decimated samples
(tfrec_amd_read_decimated), its own run table and the thresholds read back from the same submit (the level meter's per block, which
an auto stream steps; the run table's where the threshold is fixed), so the front end and the recorder ahead of the envelope are
whatever the context runs (recorder.read_envelope).  Channel-rate contexts (tfrec_amd_create_decimated) take hand-made decimated
samples: the layouts the kernels can get wrong are placed exactly.  Everything is an exact integer; nothing here has a tolerance."""
import functools
import re

import numpy as np
import pytest

import parity
import recorder as R
from recorder import (B, CONT, OPEN, TABLE_FIELDS, W, cli_lines, hand_receiver, last_pairs, raises, read_envelope, same_chains,
                      same_records, zeros)
from recorder_rows import CTX_TYPES, M, N, NB, gap_ladder, golden_iq, loud, quiet, scene
from tfrec_amd import api, burst, capture, decin, envelope

pytestmark = pytest.mark.gpu
ENVELOPE = ("envelope",)  # hand_receiver's stages; the rows here are made for a threshold of 500


# ---- hand-made rows on a channel-rate context
@functools.lru_cache(maxsize=None)
def hand_rows(nb=2):
    """int16 [2, nb B, 2] and what is where.  Stream 0: a burst at the submit's first sample; one inside a mask word; the gap ladder
    from bit 1 of a word, and again ending at bit 63; a burst across the boundary between blocks 0 and 1 with the gap on it; an over
    sample 100 ahead of the input's end.  Stream 1: a burst of 300 over samples that fills whole mask words; a single over sample
    300 ahead of the block boundary, whose tail crosses it; a burst whose gap ends with bit 0 of a mask word; the input's last sample."""
    rows = np.stack([quiet(nb, 21), quiet(nb, 22)])
    E = nb * B
    where = {
        "first": [0, 1, 2, 5, 9],
        "word": [1290, 1291, 1300, 1340],  # word 20: samples 1280 .. 1343
        "ladder": gap_ladder(3009),
        "ladder63": [p + 4992 + 63 - gap_ladder(0)[-1] % 64 for p in gap_ladder(0)],
        "across": [B - 10, B + 20, B + 21],
        "open": [E - 100],
    }
    for v in where.values():
        loud(rows[0], v)
    where1 = {"dense": list(range(900, 1200)), "tail_across": [B - 300], "bit0": [B + 4096 - 30, B + 4096], "last": [E - 1]}
    for v in where1.values():
        loud(rows[1], v, (-2500, 2600))
    rows[0, 1295] = (32767, -32768)  # full scale, and -32768, which the front end clamps
    rows.setflags(write=False)
    return rows, where, where1


@functools.lru_cache(maxsize=None)
def hand_uncut():
    rows, where, where1 = hand_rows()
    with hand_receiver(2, 2, ENVELOPE, thresh=500) as r:
        r.submit(np.ascontiguousarray(rows))
        got, decs, runs = read_envelope(r, 2, zeros(2), [0, 0])
        assert r.read_burst_envelopes().tobytes() == got.tobytes()  # reading pops nothing
        r.drain()
        raises(api.E_STATE, r.read_burst_envelopes)  # nothing undrained
    assert np.array_equal(np.stack(decs).reshape(2, 2 * B, 2), decin.clamp(rows))
    return got


def test_two_streams_of_two_blocks_of_hand_made_samples():
    got = hand_uncut()
    rows, where, where1 = hand_rows()
    of = lambda s: got[got["stream"] == s]  # noqa: E731
    by_start = {(int(r["stream"]), int(r["start_sample"])): r for r in got}
    # the rows hold what they are meant to hold (the values: the restatement's, on the CPU)
    first = by_start[0, 0]
    assert first["flags"] == 0 and (first["n_over"], first["last_over"], first["n_gaps"], first["max_gap"]) == (5, 9, 2, 3)
    word = by_start[0, 1290]
    assert (word["n_over"], word["last_over"], word["n_gaps"], word["max_gap"]) == (5, 50, 3, 39) and word["energy_head"] > 2 * 32767 ** 2
    for key in ("ladder", "ladder63"):
        r = by_start[0, where[key][0]]
        assert (r["n_over"], r["n_gaps"], r["max_gap"], r["last_over"]) == (5, 4, 65, 197) and r["n_samples"] == 198 + W - 1
    assert where["ladder"][0] % 64 == 1 and where["ladder63"][-1] % 64 == 63
    across = by_start[0, B - 10]
    assert (across["n_over"], across["n_gaps"], across["max_gap"], across["last_over"]) == (3, 1, 29, 31)
    last0 = of(0)[-1]
    assert last0["flags"] == OPEN and (last0["n_samples"], last0["last_over"]) == (100, 0)
    dense = by_start[1, 900]
    assert (dense["n_over"], dense["n_gaps"], dense["last_over"], dense["nprod_head"]) == (300, 0, 299, 299)
    tail = by_start[1, B - 300]
    assert (tail["n_over"], tail["last_over"], tail["n_samples"], tail["nprod_tail"]) == (1, 0, W, W - 1)
    last1 = of(1)[-1]
    assert last1["flags"] == OPEN and (last1["n_samples"], last1["n_over"], last1["energy_tail"], last1["nprod_head"]) == (1, 1, 0, 0)
    assert (got["lead_not_over"] == 0).all() and len(got) == 10


def test_the_same_input_in_two_submits_and_the_merged_chains():
    whole = hand_uncut()
    rows, where, where1 = hand_rows()
    with hand_receiver(2, 1, ENVELOPE, thresh=500) as r:
        for k in range(2):  # both queued before the first read
            r.submit(np.ascontiguousarray(rows[:, k * B:(k + 1) * B]))
        got, prev = [], zeros(2)
        for k in range(2):
            part = decin.clamp(rows[:, k * B:(k + 1) * B])  # (a channel-rate context's samples are its input, clamped: hand_uncut)
            recs, decs, _ = read_envelope(r, 1, prev, [k * B] * 2, decs=[part[s].reshape(-1) for s in range(2)])
            got.append(recs)
            prev = last_pairs(decs)
            r.drain()
    c = got[1][(got[1]["flags"] & CONT) != 0]
    assert c["stream"].tolist() == [0, 1] and (c["start_sample"] == B).all()
    assert (c[0]["lead_not_over"], c[0]["last_over"], c[0]["n_gaps"]) == (20, 21, 0)  # the gap on the cut: the piece's lead
    assert (c[1]["lead_not_over"], c[1]["last_over"], c[1]["n_over"]) == (W - 300, -1, 0)  # the tail alone: no over sample
    assert c[1]["energy_head"] == 0 and c[1]["nprod_tail"] == W - 300  # ... with the product across the cut, from prevdec
    o = got[0][(got[0]["flags"] & OPEN) != 0]
    assert o["stream"].tolist() == [0, 1] and o["last_over"].tolist() == [0, 0] and o["n_samples"].tolist() == [10, 300]
    key = lambda r: (int(r["stream"]), int(r["start_sample"]))  # noqa: E731
    merged, uncut = sorted(envelope.chains(got), key=key), sorted(envelope.chains([whole]), key=key)
    assert len(merged) == len(uncut) == len(whole)
    same_chains("envelope", merged, uncut, "1 + 1")


def test_an_auto_stream_whose_threshold_steps_inside_a_run():
    """Eight blocks of noise around the threshold keep an auto stream triggered: one run, and the threshold steps behind block 4.
    The over bits are the mask the threshold pass rewrote block by block."""
    nb = 8
    rng = np.random.default_rng(31)
    x = np.stack([rng.integers(-400, 401, size=(nb * B, 2)), rng.integers(-330, 331, size=(nb * B, 2))]).astype(np.int16)
    with hand_receiver(2, nb, ENVELOPE, thresh=0) as r:
        r.submit(x)
        lev = r.read_levels()
        got, decs, runs = read_envelope(r, nb, zeros(2), [0, 0])
        r.drain()
    th = lev["thresh"]
    assert th[0, 0] == 500 and th[0, -1] != 500 and len(set(th[0].tolist())) >= 2, th.tolist()
    r0 = got[got["stream"] == 0]
    assert len(r0) == 1 and r0[0]["n_samples"] >= nb * B - 16 and r0[0]["flags"] == OPEN and r0[0]["thresh"] == 500
    blind = envelope.envelopes(decs, [500, 500], got[list(TABLE_FIELDS)], zeros(2))
    assert blind[0]["n_over"] != r0[0]["n_over"]  # with the run's first threshold throughout, the count is another
    assert r0[0]["n_gaps"] > 1000 and r0[0]["max_gap"] < W


@pytest.mark.parametrize("n", [65, 97])
def test_stream_counts_across_a_waves_end(n):
    nb = 4
    rows = hand_rows(4)[0]
    rng = np.random.default_rng(41)
    kinds = [rows[0], rows[1], rng.integers(-400, 401, size=(nb * B, 2)).astype(np.int16), quiet(nb, 43)]  # 2: never leaves its window
    x = np.ascontiguousarray(np.stack(kinds)[np.arange(n) % len(kinds)])
    with hand_receiver(n, nb, ENVELOPE, thresh=500, levels=False) as r:
        r.submit(x)
        got, decs, runs = read_envelope(r, nb, zeros(n), [0] * n, levels=False)
        r.drain()
    assert sorted(set(got["stream"].tolist())) == [s for s in range(n) if s % 4 != 3]  # (row 3 is quiet)
    noise = got[got["stream"] % 4 == 2]
    assert len(noise) == len(range(2, n, 4)) and (noise["n_samples"] >= nb * B - 16).all() and (noise["flags"] == OPEN).all()
    assert (noise["n_gaps"] > 500).all() and len({r.tobytes()[24:] for r in noise}) == 1
    for s in (0, 1):  # every copy of a row has the row's records
        mine = got[got["stream"] == s]
        for t in range(s + 4, n, 4):
            theirs = got[got["stream"] == t]
            assert len(theirs) == len(mine) and all(a.tobytes()[4:] == b.tobytes()[4:] for a, b in zip(mine, theirs)), t


# ---- the other kinds of context
def scene_receiver(**kw):
    r = R.receiver(levels=True, **kw)
    r.enable_burst_envelope()
    return r


@functools.lru_cache(maxsize=None)
def scene_uncut():
    with scene_receiver() as r:
        r.submit(scene())
        got, decs, runs = read_envelope(r, NB, zeros(N), [0] * N)
        ev = r.drain()
    return got, decs, runs, ev


def test_the_aimed_u8_scene_and_its_events():
    got, decs, runs, ev = scene_uncut()
    of = lambda s: got[got["stream"] == s]  # noqa: E731
    assert len(of(0)) == 0 and len(of(1)) == 1 and of(1)[0]["start_sample"] < 2 * B < of(1)[0]["start_sample"] + of(1)[0]["n_samples"]
    assert of(1)[0]["last_over"] + W == of(1)[0]["n_samples"] and envelope.summary(of(1)[0])[2] > 100
    assert of(7)[0]["last_over"] + 400 == of(7)[0]["n_samples"]  # TFA_1 alone: its own window
    for s, length in ((3, 1), (4, 3), (5, 5)):
        assert of(s)[-1]["n_samples"] == length and of(s)[-1]["last_over"] <= length - 1
    assert of(6)[-1]["n_samples"] >= M - 16 and of(6)[-1]["n_gaps"] > 100  # the auto stream over noise
    assert parity.sort_events(ev).tobytes() == parity.sort_events(R.one_submit()[2]).tobytes()  # the events do not notice


def test_a_reset_mid_chain_drops_the_chain():
    parts = parity.cut(scene(), (2, 2))
    with scene_receiver(max_blocks=2) as r:
        r.submit(parts[0])
        got0, d0, _ = read_envelope(r, 2, zeros(N), [0] * N)
        r.drain()
        r.reset_streams([1, 6])
        r.submit(parts[1])
        base = [0 if s in (1, 6) else 2 * B for s in range(N)]  # a reset stream counts from 0 again
        got1, _, _ = read_envelope(r, 2, last_pairs(d0), base)
        r.drain()
    assert got0[got0["stream"] == 6][-1]["flags"] & OPEN
    r6 = got1[got1["stream"] == 6]
    assert not (r6["flags"] & CONT).any() and r6[0]["start_sample"] < 16 and r6[0]["lead_not_over"] == 0
    r7 = got1[got1["stream"] == 7][0]  # 7 was not reset: its piece continues
    assert r7["flags"] & CONT and r7["start_sample"] == 2 * B
    ch = envelope.chains([got0, got1], restarts={1: [1, 6]})
    six = [c for c in ch if c["stream"] == 6]
    assert len(six) == len(got0[got0["stream"] == 6]) + len(r6)  # nothing of stream 6 was merged across the reset
    dropped = six[len(six) - len(r6) - 1]  # the chain the reset cut off: it ends, still OPEN, where the first submit ends
    assert dropped.tobytes() == envelope.merge([got0[got0["stream"] == 6][-1]]).tobytes() and dropped["flags"] & OPEN
    assert dropped["start_sample"] + dropped["n_samples"] == 2 * B and envelope.summary(dropped)[2] is None  # no tail, no ratio
    seven = [c for c in ch if c["stream"] == 7 and c["start_sample"] < 2 * B < c["start_sample"] + c["n_samples"]]
    assert len(seven) == 1 and seven[0].tobytes() == [c for c in envelope.chains([scene_uncut()[0]])
                                                      if c["stream"] == 7 and c["start_sample"] == seven[0]["start_sample"]][0].tobytes()


def test_a_golden_scene_with_the_burst_meter_beside_it_and_neither():
    x = golden_iq()
    with api.Receiver(1, 0x2F, 500, 0, max_blocks=4, all_flushes=True) as r:
        plain_mem = r.memory()
        r.submit(x)
        plain = r.drain()
    with api.Receiver(1, 0x2F, 500, 0, max_blocks=4, all_flushes=True, levels=True) as r:
        r.enable_capture(256, 4 * B)
        r.enable_burst_meter()
        r.enable_burst_envelope()
        r.submit(x)
        got, decs, runs = read_envelope(r, 4, zeros(1), [0])
        bursts = r.read_bursts()
        ev = r.drain()
    with api.Receiver(1, 0x2F, 500, 0, max_blocks=4, all_flushes=True) as r:
        assert r.memory() == plain_mem  # a context without the call holds what it held
    want = burst.bursts(decs, runs, zeros(1))
    assert bursts.tobytes() == want.tobytes() and len(bursts) == len(got) >= 2
    assert parity.sort_events(ev).tobytes() == parity.sort_events(plain).tobytes() and len(ev) >= 1
    whole = [c for c in got if not c["flags"] & OPEN]
    assert all(c["last_over"] + W == c["n_samples"] and envelope.summary(c)[2] > 10000 for c in whole) and len(whole) >= 2
    # the head's products are the meter's without the tail's: the two outputs agree where they overlap
    for c, m in zip(got, bursts):
        assert c["nprod_head"] + c["nprod_tail"] == m["n_products"] and c["dot_head"] + c["dot_tail"] == m["sum_dot"]
        assert c["crs_head"] + c["crs_tail"] == m["sum_crs"] and c["energy_head"] + c["energy_tail"] == m["energy"]


def test_a_submit_runs_replay_gives_the_recordings_records():
    """The golden TFA_2 scene recorded by a u8 context (1 + 3 blocks) and replayed through sparse submits (2 + 2): between the runs
    the replay's samples are (0, 0) and never over, and the merged records are the recording's."""
    x = golden_iq()
    with api.Receiver(1, 0x2F, 500, 0, max_blocks=3, all_flushes=True, levels=True) as r:
        r.enable_capture(256, 4 * B)
        r.enable_capture_pre()
        r.enable_burst_envelope()
        tabs, recs, prev, pos = [], [], zeros(1), 0
        for p, nb in zip(parity.cut(x, (1, 3)), (1, 3)):
            r.submit(p)
            tabs.append(r.read_captures(pre=True))
            got, decs, _ = read_envelope(r, nb, prev, [pos * B])
            recs.append(got)
            prev, pos = last_pairs(decs), pos + nb
            r.drain()
    off = 0
    for t, pool, _ in tabs:
        t["pool_offset"] += off
        off += len(pool)
    runs, pool, pre = (np.concatenate([t[i] for t in tabs]) for i in range(3))
    assert len(runs) >= 2
    with api.Receiver(1, 0x2F, 500, 0, max_blocks=2, all_flushes=True, decimated=True) as r:
        r.enable_runs_input(len(runs) + 2, len(pool) + 1)
        r.enable_capture(256, 1)
        r.enable_burst_envelope()
        rep, prev = [], zeros(1)
        for k in range(2):
            t, p, q = decin.rebase(runs, pool, pre, 2 * k * B, 2 * B)
            assert r.submit_runs(t, p, q, 2) == 2
            got, decs, _ = read_envelope(r, 2, prev, [2 * k * B], levels=False)
            z = decs[0].reshape(-1, 2)
            covered = np.zeros(2 * B, dtype=bool)
            for c in got:  # a run's samples, and the pair ahead of it, which a sparse submit carries too (it is not over)
                a = int(c["start_sample"]) - 2 * k * B
                covered[max(a - 1, 0):a + int(c["n_samples"])] = True
            assert not z[~covered].any() and z[covered].any()  # zeros between the runs
            rep.append(got)
            prev = last_pairs(decs)
            r.drain()
    a, b = envelope.chains(recs), envelope.chains(rep)
    assert len(a) == len(b) >= 2
    same_chains("envelope", b, a, "the replay")


def test_overflow_delivers_the_prefix_and_a_pool_of_one_pair_delivers_everything():
    whole = hand_uncut()
    rows = np.ascontiguousarray(hand_rows()[0])
    with hand_receiver(2, 2, ENVELOPE, thresh=500, cap=(len(whole) - 1, 1)) as r:
        r.submit(rows)
        raises(api.E_OVERFLOW, r.read_burst_envelopes)
        got = r.read_burst_envelopes(allow_overflow=True)
        assert r.envelope_total == len(whole)
        same_records(got, whole[:-1], "the prefix")
        r.drain()
    with hand_receiver(2, 2, ENVELOPE, thresh=500, cap=(len(whole), 1), levels=False) as r:  # the envelope alone, the table just large enough
        r.submit(rows)
        same_records(r.read_burst_envelopes(), whole, "a pool of one pair")
        assert len(r.read_captures(allow_overflow=True)[1]) <= 1  # the pool itself held nothing
        r.drain()


def test_the_refusals_of_the_enable_call_and_what_a_context_without_it_holds():
    n, mb = 3, 2
    x = scene()[:n, :api.BLOCK_BYTES]
    with api.Receiver(n, CTX_TYPES, 500, 0, max_blocks=mb) as r:
        plain = r.memory()
        raises(api.E_INVAL, r.enable_burst_envelope)  # no recorder
        raises(api.E_INVAL, r.read_burst_envelopes)
        assert r.memory() == plain
        r.enable_capture(64, 1024)
        rec = r.memory()
        raises(api.E_INVAL, r.read_burst_envelopes)  # the recorder alone: no envelope
        r.submit(x)
        raises(api.E_INVAL, r.read_burst_envelopes)
        submitted = r.memory()  # (a host submit's staging is counted)
        raises(api.E_STATE, r.enable_burst_envelope)  # after the first submit
        assert r.memory() == submitted
        runs_plain = r.read_captures()
        ev_plain = r.drain()
    with api.Receiver(n, CTX_TYPES, 500, 0, max_blocks=mb) as r:
        r.enable_capture(64, 1024)
        assert r.memory() == rec  # a recorder without the envelope holds what it held
        r.enable_burst_envelope()
        m = r.memory()
        assert m["device_bytes"] - rec["device_bytes"] == api.FIFO_DEPTH * 64 * 128 and m["pinned_host_bytes"] == rec["pinned_host_bytes"]
        raises(api.E_INVAL, r.enable_burst_envelope)  # a second call: refused, and nothing changes
        assert r.memory() == m
        r.enable_burst_meter()  # independent of the meter: either order
        assert r.memory()["device_bytes"] - m["device_bytes"] == api.FIFO_DEPTH * 64 * 320
        raises(api.E_STATE, r.read_burst_envelopes)  # nothing undrained
        r.submit(x)
        nr = api.C.c_uint32(0)
        buf = np.full(128, 0x55, dtype=np.uint8)  # the caller's room too small: E_INVAL, nothing written, the count set
        assert r.L.tfrec_amd_read_burst_envelopes(r.h, buf.ctypes.data, 0, api.C.byref(nr)) == api.E_INVAL and (buf == 0x55).all()
        assert r.L.tfrec_amd_read_burst_envelopes(r.h, buf.ctypes.data, 1, None) == api.E_INVAL
        recs = r.read_burst_envelopes()
        assert nr.value == len(recs) == len(runs_plain[0]) == len(r.read_bursts()) == 1
        runs = r.read_captures()
        ev = r.drain()
    R.assert_tables(runs, runs_plain)
    assert parity.sort_events(ev).tobytes() == parity.sort_events(ev_plain).tobytes()


# ---- tfrec_gpu -Q
WORDS = ("extent", "burst", "scan")


def test_cli_extent_lines_of_the_golden_whb_scene_cut_into_batches(tmp_path):
    parity.build_cli()
    nb, T = 6, 3000  # -t 3000 cuts into the telegram's envelope: gaps; -b 2: the burst lies in all three batches
    x = np.ascontiguousarray(golden_iq("whb", nb)[0])
    f = str(tmp_path / "whb.iq")
    x.tofile(f)
    base = ["-T", "2f", "-t", str(T), "-b", "2"]
    plain = cli_lines(base + ["-L", f], *WORDS)
    got = cli_lines(["-Q"] + base + ["-L", f], *WORDS)
    assert plain["extent"] == [] and got["telegrams"] == plain["telegrams"] and got["burst"] == []  # the telegrams do not notice
    # the restatement: the oracle's front end (the context's, bit for bit), capture.py and envelope.py submit by submit (2 + 2 + 2)
    dec = parity.fresh_oracle(x, 0x2F, T, keep_dec=True).dec().reshape(-1, 2)
    recs, st, prev = [], None, zeros(1)
    for a, b in ((0, 2), (2, 4), (4, 6)):
        part = dec[a * B:b * B]
        runs, _, st = capture.captures(part, 0x2F, T, st)
        recs.append(envelope.envelopes([part], [T], runs, prev, base=[a * B]))
        prev = last_pairs([part])
    assert any(c["flags"] & CONT for c in recs[1]) and any(c["flags"] & CONT for c in recs[2])  # a burst is cut by the batches, twice
    want = [envelope.line(f, c) for c in envelope.chains(recs)]
    assert got["extent"] == want and len(want) >= 1
    assert any(ln.split()[8] != "-" and int(ln.split()[6]) >= 1 and int(ln.split()[3]) > 2 * B for ln in want)  # a ratio, and gaps
    # beside -M: both kinds of line, each what it is alone; through a recycled slot beside a second file
    meter = cli_lines(["-M"] + base + ["-L", f], *WORDS)
    both = cli_lines(["-M", "-Q"] + base + ["-L", f], *WORDS)
    assert both["extent"] == want and both["burst"] == meter["burst"] and len(meter["burst"]) == len(want)
    f2 = str(tmp_path / "short.iq")
    x[:2 * api.BLOCK_BYTES].tofile(f2)
    slot = cli_lines(["-Q", "-n", "1"] + base + ["-L", f, "-L", f2], *WORDS)
    assert [ln for ln in slot["extent"] if ln.split()[1] == f] == want
    # the channel table's column
    scan = cli_lines(["-Q", "-s", "100", "-t", "500", "-L", f], *WORDS)
    assert scan["extent"] == [] and len(scan["scan"]) >= 3 and all(re.search(r" burst_snr=(-|\d+\.\d\d)$", ln) for ln in scan["scan"])
    assert any(not ln.endswith("=-") for ln in scan["scan"])
    assert all("burst_snr" not in ln for ln in cli_lines(["-s", "100", "-t", "500", "-L", f], "scan")["scan"])
