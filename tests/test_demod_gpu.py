"""The burst demodulator on the GPU (tfrec_amd_enable_burst_demod, tfrec_amd_read_burst_demods, tfrec_gpu -w), bit for bit:
every record and every entry of the decision pool against demod.demods on the context's OWN decimated samples and run table.  A loud
stretch [a, b) gives the run [a, b + W - 1); a run shorter than W is one that the submit's end cuts.  No tolerance."""
import numpy as np
import pytest

import parity
import recorder as R
from recorder import B, CONT, W, cli_lines, hand_receiver, raises, same_records
from recorder_rows import fsk, golden_iq, quiet
from tfrec_amd import api, capture, decin, demod

pytestmark = pytest.mark.gpu
NB, M = 2, 2 * B
# 384000 / R is no integer; 64 samples a symbol; b(1) = 4; Pn = 384 and Nt = 21; Manchester; the largest rate Manchester allows
CASES = [(17240, "nrz"), (6000, "nrz"), (96000, "nrz"), (1000, "nrz"), (8842, "man"), (48000, "man")]
# the loud stretches [a, b) of every stream: a run of 30 samples at the submit's end (fewer than 8 decisions at every rate: Pn - 1 + g(8)
# >= 35); a run of 5793 samples (a decision straddles the tile's edge at 4096; 1000 bit/s times 14 of its 21 decisions); one across the
# block boundary; one at the submit's first sample; a second run longer than a tile, from another place in the pool
STRETCH = [(M - 30, M), (100, 5200), (B - 300, B + 300), (0, 1300), (9000, 9000 + 4097)]


def rows_of(stretches, nb, rate, seed):
    rng = np.random.default_rng(seed)
    rows = np.stack([quiet(nb, 40 + s) for s in range(len(stretches))])
    for s, (a, b) in enumerate(stretches):
        rows[s, a:b] = fsk(rng.integers(0, 2, 2 + (b - a) * rate // 384000).tolist(), rate)[:b - a]
    rows.setflags(write=False)
    return rows


def demod_receiver(n, nb, rate, code, cap=None):
    r = hand_receiver(n, nb, (), cap=cap or (32 * n, n * nb * B), levels=False)
    r.enable_burst_demod(rate, code, 20000)
    return r


def read_demod(r, nb, st, state, prev, base, decs=None, overflow=False, max_samples=None):
    """The oldest undrained submit's records and pool against the restatement -> (records, pool, the state behind it, the samples)."""
    decs, runs, _ = R.submit_view(r, nb, decs, levels=None)
    got, pool = r.read_burst_demods(allow_overflow=overflow)
    assert len(got) == min(r.demod_total, r._capture[0]) and len(runs) <= len(got)
    want, wpool, nxt = demod.demods(decs, runs, prev, st, state, r.n_streams, max_samples, base)
    same_records(got[:len(runs)], want, "demod")
    assert not got["timing"][len(runs):].any() and not got["n_symbols"][len(runs):].any()  # behind the pool's end: not looked at
    bad = np.flatnonzero(pool != wpool) if len(pool) == len(wpool) else [-1]
    assert pool.dtype == np.int16 and len(bad) == 0, "demod pool: %d entries, want %d, the first difference at %d" % (len(pool), len(wpool), bad[0])
    return got, pool, nxt, decs


@pytest.mark.parametrize("rate, code", CASES)
def test_hand_made_runs_in_one_submit(rate, code):
    st = demod.Settings(rate, code, 20000)
    rows = rows_of(STRETCH, NB, st.Rc, 11)
    with demod_receiver(len(rows), NB, rate, code) as r:
        r.submit(np.ascontiguousarray(rows))
        got, pool = read_demod(r, NB, st, None, R.zeros(len(rows)), [0] * len(rows))[:2]
        again = r.read_burst_demods()  # reading pops nothing
        assert again[0].tobytes() == got.tobytes() and again[1].tobytes() == pool.tobytes()
        r.drain()
        raises(api.E_STATE, r.read_burst_demods)  # nothing undrained
    by = {int(x["stream"]): x for x in got}
    assert by[0]["timing"] == demod.FLAGGED and by[0]["n_timed"] < 8 and by[0]["n_samples"] == 30
    assert by[1]["timing"] == demod.MEASURED and by[1]["n_samples"] == 5100 + W - 1 and by[1]["n_timed"] == min(st.Nt, st.ended(5793 - st.Pn + 1, 0))
    assert (got["n_symbols"] == [st.ended(int(x["n_samples"]), int(x["phase"])) for x in got]).all() and not got["first_symbol"].any()


def test_65_streams_straddle_the_list_kernels_wave():
    st = demod.Settings(17240, "nrz", 20000)
    rows = rows_of(STRETCH, NB, st.Rc, 11)[np.arange(65) % len(STRETCH)]
    with demod_receiver(65, NB, 17240, "nrz") as r:
        r.submit(np.ascontiguousarray(rows))
        got = read_demod(r, NB, st, None, R.zeros(65), [0] * 65)[0]
        r.drain()
    assert len(got) == 65 and got[64]["timing"] == demod.MEASURED and got[64]["n_symbols"] == got[4]["n_symbols"] > 200


# ---- chains, three blocks: stream 0 an OPEN run of 3 samples continued twice (flagged: the chain inherits phase 0; the second piece a
# whole block, CONTINUES and OPEN); 1 and 2: an OPEN piece of 1000 and of 1001 samples continued twice -- too short for the whole timing
# window at every rate but 96000 and 48000, and a decision straddles a cut unless it falls on the grid, which it cannot for both streams;
# 3: the third block alone
CHAIN = [(B - 3, 2 * B + 900), (B - 1000, 2 * B + 2000), (B - 1001, 2 * B + 2000), (2 * B + 100, 2 * B + 400)]


def cut_submits(rate, code, sizes, restart=None):
    """The chain rows in submits of `sizes` blocks, all queued before the first read (restart: (submit, streams) reset ahead of it, which
    drains what is queued) -> every submit's records."""
    st = demod.Settings(rate, code, 20000)
    rows = rows_of(CHAIN, 3, st.Rc, 12)
    got, state, prev, done = [], None, R.zeros(4), 0
    edges = (np.concatenate([[0], np.cumsum(sizes)]) * B).tolist()
    spans = list(zip(edges[:-1], edges[1:]))
    base = [0] * 4

    def read(k):
        nonlocal state, prev
        a, b = spans[k]
        part = decin.clamp(rows[:, a:b])
        recs, _, state, decs = read_demod(r, (b - a) // B, st, state, prev, [a - o for o in base], decs=[part[s].reshape(-1) for s in range(4)])
        prev = R.last_pairs(decs)
        got.append(recs)
        r.drain()

    with demod_receiver(4, max(sizes), rate, code) as r:
        for k, (a, b) in enumerate(spans):
            if restart and restart[0] == k:
                while done < k:
                    read(done)
                    done += 1
                r.reset_streams(restart[1])
                for s in restart[1]:
                    state["soft"][s], state["ahead"][s], state["phase"][s] = np.zeros(demod.SPAN, np.int64), 0, 0
                    base[s] = a
            r.submit(np.ascontiguousarray(rows[:, a:b]))
        for k in range(done, len(spans)):
            read(k)
    return got, st


@pytest.mark.parametrize("rate, code", CASES)
def test_a_chain_over_three_queued_submits(rate, code):
    got, st = cut_submits(rate, code, (1, 1, 1))
    assert [np.count_nonzero(g["flags"] & CONT) for g in got] == [0, 3, 3]
    assert all((g["timing"][(g["flags"] & CONT) != 0] == demod.INHERITED).all() for g in got)
    first = {int(x["stream"]): x for x in got[0]}
    timed = min(st.Nt, st.ended(1000 - st.Pn + 1, 0))  # of the piece of 1000 samples: all Nt at 96000 and 48000 alone, one at 1000
    assert first[0]["timing"] == demod.FLAGGED and first[1]["timing"] == (demod.MEASURED if timed >= 8 else demod.FLAGGED)
    assert first[1]["n_timed"] == timed and (timed < st.Nt) == (rate < 48000)
    straddles = 0  # decisions of streams 1 and 2 that begin ahead of a cut and end behind it
    for s, n0 in ((1, 1000), (2, 1001)):
        for k, ahead in ((1, n0), (2, n0 + B)):
            x = got[k][got[k]["stream"] == s][0]
            assert x["phase"] == first[s]["phase"] and x["first_symbol"] == st.ended(ahead, int(x["phase"]))
            straddles += int(x["phase"]) + st.g(int(x["first_symbol"])) < ahead
    assert straddles >= 2


@pytest.mark.parametrize("rate, code", [(17240, "nrz"), (8842, "man")])
def test_a_restart_between_submits_drops_the_chain(rate, code):
    got, _ = cut_submits(rate, code, (1, 1), restart=(1, [1]))
    one, two = got[1][got[1]["stream"] == 1][0], got[1][got[1]["stream"] == 2][0]
    assert not one["flags"] & CONT and one["timing"] == demod.MEASURED and one["first_symbol"] == 0
    assert two["flags"] & CONT and two["timing"] == demod.INHERITED and two["first_symbol"] > 0


@pytest.mark.parametrize("cap, fits", [((3, 5 * M), 3), ((64, 7000), None)])
def test_overflows_deliver_their_prefixes(cap, fits):
    st = demod.Settings(17240, "nrz", 20000)
    rows = rows_of(STRETCH, NB, st.Rc, 11)
    with demod_receiver(len(rows), NB, 17240, "nrz", cap=cap) as r:
        r.submit(np.ascontiguousarray(rows))
        raises(api.E_OVERFLOW, r.read_burst_demods)
        got, pool = read_demod(r, NB, st, None, R.zeros(len(rows)), [0] * len(rows), overflow=True, max_samples=cap[1])[:2]
        r.drain()
    assert len(got) == (fits or len(STRETCH))
    if fits is None:  # 30 + 5793 pairs fit, the run of 1293 behind them does not: neither it nor a later one is looked at
        assert got["timing"].tolist() == [demod.FLAGGED, demod.MEASURED, 0, 0, 0] and len(pool) == 5823


def test_the_golden_scene_beside_the_other_stages_the_refusals_and_the_cli(tmp_path):
    x = golden_iq()
    st = demod.Settings(17240)
    with api.Receiver(1, 0x2F, 500, 0, max_blocks=4, all_flushes=True, levels=True) as r:
        plain_mem = r.memory()
        raises(api.E_INVAL, r.enable_burst_demod, 17240)  # no recorder
        raises(api.E_INVAL, r.read_burst_demods)
        assert r.memory() == plain_mem
        r.enable_capture(256, 4 * B)
        rec_mem = r.memory()
        r.enable_burst_meter()
        r.enable_burst_clock()
        r.submit(x)
        raises(api.E_STATE, r.enable_burst_demod, 17240)  # after the first submit
        raises(api.E_INVAL, r.read_burst_demods)  # the stage is off
        plain_meter, plain_clock = r.read_bursts(), r.read_burst_clocks()
        plain_runs = r.read_captures()
        plain = r.drain()
    with api.Receiver(1, 0x2F, 500, 0, max_blocks=4, all_flushes=True, levels=True) as r:
        r.enable_capture(256, 4 * B)
        assert r.memory() == rec_mem  # a recorder without the call holds what it held
        for bad in ((999,), (96001,), (48001, "man"), (9600, "nrzi"), (9600, "nrz", 192001), (9600, "nrz", -192001), (2 ** 31,)):
            raises(api.E_INVAL, r.enable_burst_demod, *bad)
        assert r.L.tfrec_amd_enable_burst_demod(r.h, 9600, 2, 0) == api.E_INVAL and r.L.tfrec_amd_enable_burst_demod(None, 9600, 0, 0) == api.E_INVAL
        assert r.memory() == rec_mem  # a call that fails leaves the context as it was
        r.enable_burst_demod(17240)
        m = r.memory()
        assert m["device_bytes"] - rec_mem["device_bytes"] == demod.device_bytes(1, 4, 256, 4 * B)
        assert m["pinned_host_bytes"] == rec_mem["pinned_host_bytes"] + demod.pinned_bytes(1)
        raises(api.E_INVAL, r.enable_burst_demod, 17240)  # a second call: refused, and nothing changes
        assert r.memory() == m
        r.enable_burst_meter()
        r.enable_burst_clock()
        r.submit(x)
        got = read_demod(r, 4, st, None, R.zeros(1), [0])[0]
        assert r.read_bursts().tobytes() == plain_meter.tobytes() and r.read_burst_clocks().tobytes() == plain_clock.tobytes()
        tab = r.read_captures()
        ev = r.drain()
    R.assert_tables(tab, plain_runs)
    R.same_events(ev, plain)
    assert len(ev) >= 1 and len(got) == 2 and (got["timing"] == demod.MEASURED).all()
    # tfrec_gpu -w: the scene moved 5500 samples back inside 6 blocks of silence, so that -b 2 cuts both bursts at a batch's end; the
    # lines against the restatement in the same three batches on the context's own decimated samples
    x6 = np.full(6 * api.BLOCK_BYTES, 128, dtype=np.uint8)
    x6[8 * 5500:8 * 5500 + x.shape[1]] = x[0]
    with api.Receiver(1, 0x2F, 500, 0, max_blocks=6, all_flushes=True, levels=True) as r:
        r.submit(x6[None])
        dec = r.decimated(0, 6 * B)
        r.drain()
    state, cst, prev, parts = None, None, np.zeros(2, np.int16), []
    for a in (0, 2, 4):
        part = dec[2 * a * B:2 * (a + 2) * B]
        runs, _, cst = capture.captures(part, 0x2F, 500, state=cst)
        recs, pool, state = demod.demods([part], runs, [prev], st, state, base=[a * B])
        parts.append((recs, pool))
        prev = part.reshape(-1, 2)[-1]
    parity.build_cli()
    f = str(tmp_path / "tfa_2.iq")
    x6.tofile(f)
    base = ["-T", "2f", "-t", "500", "-b", "2", "-L", f]
    lines, alone = cli_lines(["-w", "17240", "-C"] + base, "demod", "clock"), cli_lines(["-C"] + base, "demod", "clock")
    assert lines["demod"] == [demod.line(f, c, st) for c in demod.chains(parts)] and len(lines["demod"]) == 2 and alone["demod"] == []
    assert sum(len(p[0]) for p in parts) == 4 and all("2dd49" in ln.split()[-1] for ln in lines["demod"])
    assert lines["clock"] == alone["clock"] and lines["telegrams"] == alone["telegrams"]
