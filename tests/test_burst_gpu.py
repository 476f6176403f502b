"""The burst meter on the GPU (tfrec_amd_enable_burst_meter, tfrec_amd_read_bursts, tfrec_gpu -M), bit for bit.

The records are compared with the restatement tfrec_amd/burst.py run on the context's OWN decimated samples
(tfrec_amd_read_decimated) and its own run table, so the front end and the recorder ahead of the meter are whatever the context
runs (recorder.read_meter).  The aimed scene is recorder_rows.scene: eight streams of four blocks with a run across a block
boundary, runs ending on word edges, runs open at the submit's last 1, 3 and 5 samples, a noise row that stays inside its window and
a quiet row.  Everything is an exact integer; nothing here has a tolerance."""
import functools
import os

import numpy as np
import pytest

import parity
import recorder as R
from recorder import B, cli_lines, last_pairs, raises, read_meter, same_chains, same_records, zeros
from recorder_rows import CTX_TYPES, M, N, NB, scene
from tfrec_amd import api, burst, capture, decin, resample, synth

pytestmark = pytest.mark.gpu


def receiver(**kw):
    r = R.receiver(**kw)
    r.enable_burst_meter()
    return r


@functools.lru_cache(maxsize=None)
def one_submit(serial=False):
    """-> (records, the table, every stream's decimated samples, events); the records are the restatement's."""
    with receiver(serial_chains=serial) as r:
        r.submit(scene())
        r.read_captures()  # (refused had the recorder overflowed: read_meter then holds the records to the whole table and total)
        recs, decs, runs = read_meter(r, NB, zeros(N), [0] * N)
        assert r.read_bursts().tobytes() == recs.tobytes()  # reading pops nothing
        ev = r.drain()
        raises(api.E_STATE, r.read_bursts)  # nothing undrained
    return recs, runs, decs, ev


def test_the_records_equal_the_restatement_on_the_aimed_scene():
    recs, runs, decs, ev = one_submit()
    same_records(recs, burst.bursts(decs, runs, zeros(N)))  # (on the table itself; read_meter: on what the records repeat of it)
    of = lambda s: recs[recs["stream"] == s]  # noqa: E731
    assert len(of(0)) == 0 and len(of(1)) == 1  # the quiet row; the run across the boundary between blocks 1 and 2 ...
    r1 = of(1)[0]
    assert r1["start_sample"] < 2 * B < r1["start_sample"] + r1["n_samples"] and r1["n_products"] > 0  # ... two workgroups, one record
    for s, length in ((3, 1), (4, 3), (5, 5)):  # the open runs of 1, 3 and 5 samples: 0, 2 and 4 products at the most
        assert of(s)[-1]["n_samples"] == length and of(s)[-1]["n_products"] <= length - 1
    r6 = of(6)[-1]  # the noise row never leaves its window: one run over (nearly) all four blocks, spread over their workgroups
    assert r6["n_samples"] >= M - 16 and r6["n_products"] > 3 * B
    assert burst.summary(r1) is not None
    assert parity.sort_events(ev).tobytes() == parity.sort_events(R.one_submit()[2]).tobytes()  # the events do not notice


def test_one_plus_three_queued_before_the_first_read_and_the_merged_chains():
    whole, wruns, decs, _ = one_submit()
    parts = parity.cut(scene(), (1, 3))
    with receiver(max_blocks=3) as r:
        for p in parts:
            r.submit(p)
        got, prev, pos = [], zeros(N), 0
        for k, nb in enumerate((1, 3)):  # (the front end does not depend on the cut: the uncut context's samples)
            d = [x[2 * pos * B:2 * (pos + nb) * B] for x in decs]
            r.read_captures()  # (nothing overflowed)
            recs, _, runs = read_meter(r, nb, prev, [pos * B] * N, decs=d)
            if k == 1:  # the CONTINUES piece used prevdec: with (0, 0) ahead of it the restatement counts one product less
                c = np.flatnonzero(runs["flags"] & capture.RUN_CONTINUES)
                assert len(c) >= 1 and (runs["stream"][c] == 6).all()
                blind = burst.bursts(d, runs, zeros(N), base=[pos * B] * N)
                assert (blind["n_products"][c] == recs["n_products"][c] - 1).all()
            got.append(recs)
            prev, pos = last_pairs(d), pos + nb
            r.drain()
    key = lambda r: (int(r["stream"]), int(r["start_sample"]))  # noqa: E731
    merged, uncut = sorted(burst.chains(got), key=key), sorted(burst.chains([whole]), key=key)
    assert len(merged) == len(uncut) == len(whole)
    same_chains("meter", merged, uncut, "1 + 3")


def test_a_reset_between_submits_gives_no_continues_and_leaves_the_first_product_out():
    parts = parity.cut(scene(), (2, 2))
    with receiver(max_blocks=2) as r:
        r.submit(parts[0])
        r.read_captures()  # (nothing overflowed)
        got0, d0, _ = read_meter(r, 2, zeros(N), [0] * N)
        r.drain()
        r.reset_streams([1, 6])
        r.submit(parts[1])
        base = [0 if s in (1, 6) else 2 * B for s in range(N)]  # a reset stream counts from 0 again
        r.read_captures()
        got1, _, _ = read_meter(r, 2, last_pairs(d0), base)
        r.drain()
    r6 = got1[got1["stream"] == 6]
    assert not (r6["flags"] & capture.RUN_CONTINUES).any() and r6[0]["start_sample"] < 16
    assert r6[0]["n_products"] <= r6[0]["n_samples"] - 1  # its first sample has no product
    r7 = got1[got1["stream"] == 7][0]  # 7 was not reset: its piece continues, with the product across the cut
    assert r7["flags"] & capture.RUN_CONTINUES and r7["start_sample"] == 2 * B
    open_chains = burst.chains([got0, got1], restarts={1: [1, 6]})
    assert sum(int(c["n_samples"]) for c in open_chains) == int(got0["n_samples"].sum() + got1["n_samples"].sum())


def test_overflow_delivers_the_prefix_and_a_pool_of_one_pair_delivers_everything():
    whole, wruns, decs, _ = one_submit()
    with receiver(cap=(len(wruns) - 1, N * M)) as r:
        r.submit(scene())
        raises(api.E_OVERFLOW, r.read_bursts)
        got = r.read_bursts(allow_overflow=True)
        assert r.burst_total == len(wruns)
        same_records(got, whole[:-1], "the prefix")
        r.drain()
        r.submit(scene()[:, :api.BLOCK_BYTES])  # the next submit -- one block, so that it fits -- is exact, CONTINUES included
        r.read_captures()  # (nothing overflowed)
        got2, _, runs2 = read_meter(r, 1, last_pairs(decs), [M] * N)
        r.drain()
    assert (runs2["flags"] & capture.RUN_CONTINUES).any()
    with receiver(cap=(4096, 1)) as r:  # the meter alone: the pool holds nothing, the table and the records are whole
        r.submit(scene())
        same_records(r.read_bursts(), whole, "a pool of one pair")
        r.drain()


# ---- hand-made rows on a channel-rate context
def hand_rows():
    """int16 [rows, B, 2], one block: extreme products, a tone, zeros inside a run, triggers at the first and the last sample, and
    every product that lies on a boundary between two bins or on an axis."""
    rows = np.zeros((6, B, 2), dtype=np.int16)
    k = np.arange(B)
    # 0: full scale, alternating in sign -- and -32768, which the front end clamps: |dot| = 2 * 32767^2, the largest
    rows[0, 100:900] = np.where((k[100:900] % 2 == 0)[:, None], 32767, -32768)
    rows[0, 1500:2300, 0] = np.where(k[1500:2300] % 2 == 0, 32767, -32767)  # I alone flips, then (from 1900) Q alone
    rows[0, 1500:1900, 1] = 32767
    rows[0, 1900:2300, 0] = -32767
    rows[0, 1900:2300, 1] = np.where(k[1900:2300] % 2 == 0, 32767, -32767)
    rows[0, 3000:3400] = np.stack([np.where(k[:400] % 4 < 2, 32767, -32767), np.where((k[:400] + 1) % 4 < 2, 32767, -32767)], 1)  # quarter turns
    # 1: a tone of amplitude 20000 at +31 kHz, 1500 samples
    ph = 2 * np.pi * 31000 / 384000 * np.arange(1500)
    rows[1, 4000:5500] = np.stack([np.round(20000 * np.cos(ph)), np.round(20000 * np.sin(ph))], 1)
    # 2: loud samples 50 apart with zeros between them (zero products inside a run), then loud pairs
    rows[2, 1000:3000:50] = (3000, -2000)
    rows[2, 3000:3600:50] = (-700, 900)
    rows[2, 3001:3600:50] = (900, 700)
    # 3: a trigger at sample 0 and one at the last sample
    rows[3, 0] = (4000, 1)
    rows[3, 1:40] = (300, -300)
    rows[3, B - 1] = (-5, 4000)
    # 4: (1, 0) and the boundary vectors by turns: the products are the vector and its mirror image, both ties; then the axes and diagonals
    c, s = burst.directions()
    ties = [(s[(j + 1) % 64] - s[j], c[j] - c[(j + 1) % 64]) for j in range(64)]
    ties += [(3000, 0), (0, 3000), (-3000, 0), (0, -3000), (2000, 2000), (-2000, 2000), (-2000, -2000), (2000, -2000)]
    rows[4, 500] = (3000, 0)
    for i, v in enumerate(ties):
        rows[4, 501 + 2 * i] = (1, 0)
        rows[4, 502 + 2 * i] = v
    # 5: quiet
    rows[5] = np.random.default_rng(3).integers(-40, 41, (B, 2))
    return rows


@pytest.mark.parametrize("n", [65, 97])
def test_hand_made_rows_on_a_channel_rate_context(n):
    rows = hand_rows()
    x = np.ascontiguousarray(rows[np.arange(n) % len(rows)])
    with api.Receiver(n, 0x2F, 500, 0, max_blocks=1, decimated=True) as r:
        r.enable_capture(16 * n, 1)
        r.enable_burst_meter()
        r.submit(x)
        decs = [r.decimated(s, B) for s in range(n)]
        got = r.read_bursts()
        r.drain()
    assert np.array_equal(np.stack(decs).reshape(n, B, 2), decin.clamp(x))
    per = [capture.captures(d, 0x2F, 500)[:2] for d in decs]
    runs = capture.table(per)[0]
    want = burst.bursts(decs, runs, zeros(n))
    same_records(got, want)
    assert (got["hist"].sum(axis=1) == got["n_products"]).all()
    assert (got["stream"] == runs["stream"]).all() and len(np.unique(got["stream"])) == n - len(range(5, n, 6))  # (row 5 is quiet)
    # the rows hold what they are meant to hold (the values: the restatement's, on the CPU)
    first = {int(s): got[got["stream"] == s] for s in range(len(rows))}
    assert first[0][0]["pwr_max"] == 65534 and set(np.flatnonzero(first[0][0]["hist"]).tolist()) == {0, 16, 32, 48}  # the axes alone
    assert first[0][0]["sum_dot"] < -(1 << 40)
    assert burst.summary(first[1][0]) == (30000, 0) and first[1][0]["hist"][5] == 1499  # 31 kHz: bin 5
    assert first[2][0]["n_products"] == 12 and first[2][0]["n_samples"] > 3000  # the zero rule
    assert first[3][0]["start_sample"] == 0 and first[3][0]["flags"] == 0 and first[3][-1]["start_sample"] == B - 1
    assert first[3][-1]["n_products"] == 0 and first[3][-1]["flags"] == capture.RUN_OPEN and first[3][-1]["energy"] == 25 + 16000000
    h = first[4][0]["hist"]  # a tie goes to the lower bin -- bin 63 loses both of its ties, to 62 and to 0
    assert h.sum() == 144 and h[:63].min() >= 2 and h[63] == 0


# ---- one case each on the other kinds of context
def check_plain(r, parts, types, thresh, submit=None):
    """Submit by submit on a uniform context: the records against the restatement on its own samples and table -> products."""
    n = r.n_streams
    prev, pos, total, all_recs = zeros(n), 0, 0, []
    for p in parts:
        nb = submit(r, p) if submit else r.submit(p)
        got, decs, _ = read_meter(r, nb, prev, [pos * B] * n)
        r.drain()
        prev, pos, total = last_pairs(decs), pos + nb, total + int(got["n_products"].sum())
        all_recs.append(got)
    return total, all_recs


def test_a_rate_context():
    p, q, nb = 25, 16, 2
    row = synth.gen_scene(41, nb, [dict(proto=1, start=5000 * p, payload_seed=5, f0_hz=0, amp=60)], rate_mult=p).reshape(-1, 2)[::q]
    row = np.ascontiguousarray(row).reshape(1, -1)[:, :2 * resample.input_samples(nb, p, q)]
    with api.Receiver(1, 0x2F, 500, 0, max_blocks=nb, input_rate=(p, q)) as r:
        r.enable_capture(256, 1)
        r.enable_burst_meter()
        assert check_plain(r, [row], 0x2F, 500)[0] > 0


def test_a_10x_context_with_the_meter_alone():
    iq10 = np.stack([synth.gen_stream(9, s, 1, rate_mult=10) for s in range(2)])
    with api.Receiver(2, 0x2F, 100, 0, max_blocks=1, input_10x=True, burst_meter=True) as r:  # (-t 100: the block's noise floor triggers)
        assert check_plain(r, [iq10], 0x2F, 100)[0] > 0


def test_a_serial_chains_context():
    ser, runs, _, ev = one_submit(True)
    assert ser.tobytes() == one_submit()[0].tobytes() and runs.tobytes() == one_submit()[1].tobytes()
    assert parity.sort_events(ev).tobytes() == parity.sort_events(one_submit()[3]).tobytes()


def test_a_submit_runs_replay_gives_the_recordings_records():
    """The golden TFA_2 scene recorded by a u8 context (1 + 3 blocks) and replayed through sparse submits (2 + 2): between the runs
    the replay's samples are (0, 0), and the merged records are the recording's."""
    x = np.load(os.path.join(parity.ROOT, "tests", "golden", "iq_tfa_2.npz"))["iq"][None, :NB * api.BLOCK_BYTES]
    with api.Receiver(1, 0x2F, 500, 0, max_blocks=3, all_flushes=True) as r:
        r.enable_capture(256, M)
        r.enable_capture_pre()
        r.enable_burst_meter()
        tabs, recs = [], []
        for p in parity.cut(x, (1, 3)):
            r.submit(p)
            tabs.append(r.read_captures(pre=True))
            recs.append(r.read_bursts())
            r.drain()
    off = 0
    for t, pool, _ in tabs:
        t["pool_offset"] += off
        off += len(pool)
    runs, pool, pre = (np.concatenate([t[i] for t in tabs]) for i in range(3))
    assert len(runs) >= 1 and sum(int(c["n_products"]) for c in recs[0]) + sum(int(c["n_products"]) for c in recs[1]) > 1000

    def submit(r, k):
        t, p, q = decin.rebase(runs, pool, pre, 2 * k * B, 2 * B)
        return r.submit_runs(t, p, q, 2)

    with api.Receiver(1, 0x2F, 500, 0, max_blocks=2, all_flushes=True, decimated=True) as r:
        r.enable_runs_input(len(runs) + 2, len(pool) + 1)
        r.enable_capture(256, 1)
        r.enable_burst_meter()
        total, rep = check_plain(r, [0, 1], 0x2F, 500, submit=submit)
    a, b = burst.chains(recs), burst.chains(rep)
    assert len(a) == len(b) >= 1 and total > 1000
    same_chains("meter", b, a, "the replay")


def test_without_the_call_nothing_changes_and_a_failed_enable_leaves_the_context_as_it_was():
    n, mb = 3, 2
    with api.Receiver(n, CTX_TYPES, 500, 0, max_blocks=mb) as r:
        plain = r.memory()
        raises(api.E_INVAL, r.enable_burst_meter)  # no recorder
        raises(api.E_INVAL, r.read_bursts)
        assert r.memory() == plain
        r.enable_capture(64, 1024)
        rec = r.memory()
        raises(api.E_INVAL, r.read_bursts)  # the recorder alone: no meter
        r.submit(scene()[:n, :api.BLOCK_BYTES])
        raises(api.E_INVAL, r.read_bursts)
        submitted = r.memory()  # (a host submit's staging is counted)
        raises(api.E_STATE, r.enable_burst_meter)  # after the first submit
        assert r.memory() == submitted
        runs_plain = r.read_captures()
        ev_plain = r.drain()
    with api.Receiver(n, CTX_TYPES, 500, 0, max_blocks=mb) as r:
        r.enable_capture(64, 1024)
        assert r.memory() == rec  # a recorder without the meter holds what it held
        r.enable_burst_meter()
        m = r.memory()
        assert m["device_bytes"] - rec["device_bytes"] == api.FIFO_DEPTH * 64 * 320 and m["pinned_host_bytes"] == rec["pinned_host_bytes"]
        raises(api.E_INVAL, r.enable_burst_meter)  # a second call: refused, and nothing changes
        assert r.memory() == m
        raises(api.E_STATE, r.read_bursts)  # nothing undrained
        r.submit(scene()[:n, :api.BLOCK_BYTES])
        nr = api.C.c_uint32(0)
        buf = np.full(320, 0x55, dtype=np.uint8)  # the caller's room too small: E_INVAL, nothing written, the count set
        assert r.L.tfrec_amd_read_bursts(r.h, buf.ctypes.data, 0, api.C.byref(nr)) == api.E_INVAL and (buf == 0x55).all()
        assert r.L.tfrec_amd_read_bursts(r.h, buf.ctypes.data, 1, None) == api.E_INVAL
        recs = r.read_bursts()
        assert nr.value == len(recs) == len(runs_plain[0]) == 1
        runs = r.read_captures()
        ev = r.drain()
    R.assert_tables(runs, runs_plain)
    assert parity.sort_events(ev).tobytes() == parity.sort_events(ev_plain).tobytes()


# ---- tfrec_gpu -M
def test_cli_burst_lines_of_the_golden_tfa_2_scene(tmp_path):
    parity.build_cli()
    z = np.load(os.path.join(parity.ROOT, "tests", "golden", "iq_tfa_2.npz"))
    nb = 3
    x = np.ascontiguousarray(z["iq"][:nb * api.BLOCK_BYTES])
    f = str(tmp_path / "tfa2.iq")
    x.tofile(f)
    base = ["-T", "2f", "-t", "500", "-b", "2"]
    plain = cli_lines(base + ["-L", f], "burst")
    got = cli_lines(["-M"] + base + ["-L", f], "burst")
    assert plain["burst"] == [] and got["telegrams"] == plain["telegrams"] and len(got["telegrams"]) >= 1  # the telegrams do not notice
    # the restatement: the oracle's front end (the context's, bit for bit), capture.py and burst.py submit by submit (-b 2: 2 + 1)
    o = parity.fresh_oracle(x, 0x2F, 500, keep_dec=True)
    dec = o.dec().reshape(-1, 2)
    recs, st, prev = [], None, zeros(1)
    for a, b in ((0, 2), (2, 3)):
        part = dec[a * B:b * B]
        runs, _, st = capture.captures(part, 0x2F, 500, st)
        recs.append(burst.bursts([part], runs, prev, base=[a * B]))
        prev = last_pairs([part])
    want = [burst.line(f, c) for c in burst.chains(recs)]
    assert got["burst"] == want and len(want) >= 1
    assert any(ln.split()[5] != "-" for ln in want)
    # the same through a recycled slot beside a second file, and with the recorder's files beside it
    f2 = str(tmp_path / "short.iq")
    x[:2 * api.BLOCK_BYTES].tofile(f2)
    slot = cli_lines(["-M", "-n", "1"] + base + ["-L", f, "-L", f2], "burst")
    assert [ln for ln in slot["burst"] if ln.split()[1] == f] == want
    both = cli_lines(["-M", "-S", str(tmp_path / "cap")] + base + ["-L", f], "burst")
    assert both["burst"] == want and os.path.getsize(str(tmp_path / "cap") + ".0.cs16") > 0
