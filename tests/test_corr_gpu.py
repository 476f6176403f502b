"""The burst correlator on the GPU (tfrec_amd_enable_burst_corr, tfrec_amd_read_burst_corrs, tfrec_gpu -y), bit for bit.

Every record is compared, byte for byte, with corr.corrs run on the context's OWN decimated samples and run table.  Channel-rate
contexts take hand-made samples, so a template's length beside the instruction's depth of 64, a run's length beside a template's and
beside the tile of 256 positions, the carried history and the pool's byte alignment are placed exactly.  A loud stretch [a, b) gives
the run [a, b + W - 1); a run shorter than W is one that the submit's end cuts.  Everything is an exact integer: no tolerance."""
import functools

import numpy as np
import pytest

import parity
import recorder as R
from recorder import B, CONT, OPEN, TABLE_FIELDS, W, cli_lines, hand_receiver, raises, same_chains, same_records
from recorder_rows import fsk, golden_iq, quiet, word_bits
from stream_count_rows import COUNTS, rows_of
from tfrec_amd import api, band, corr, decin

pytestmark = pytest.mark.gpu
NB, M = 2, 2 * B
# K_t = floor(384000 P / R): 63, 64 and 65 taps (one chunk of the instruction against two); 160 and 1024 (the right alignment); 2048;
# and sixteen templates of 8 .. 64 bits
BANKS = {
    "chunks": ([(0xB2, 8, 48761), (0xB2, 8, 48000), (0xB2, 8, 47261)], 0),
    "mix": ([(0xB2, 8, 19200), (0x2DD4B2A7, 32, 12000)], 20000),
    "long": ([(0x2DD4B2A79C35E10F, 64, 12000)], -35000),
    "sixteen": ([(0x2DD4B2A79C35E10F >> t, 8 + 3 * t, 17240 + 1999 * t) for t in range(16)], -3001),
}
# the loud stretches [a, b) of every stream: runs of K - 1 and K samples at the submit's end for K = 63, 64, 65 and 160; a run at the
# submit's first sample; 255, 256 and 257 defined positions of the 1024-tap template (n = 1278, 1279, 1280: the runs of streams 5, 6 and 7
# also share 16-byte words of the byte pool); 767, 768 and 769 samples (the tile's edge); across the block boundary; 2047 and 2048 samples
STRETCH = [(M - 62, M), (M - 63, M), (M - 64, M), (M - 65, M), (M - 159, M), (M - 160, M), (0, 1278 - W + 1), (100, 100 + 1279 - W + 1),
           (40, 40 + 1280 - W + 1), (7, 7 + 767 - W + 1), (9, 9 + 768 - W + 1), (11, 11 + 769 - W + 1), (B - 300, B + 300),
           (5, 5 + 2047 - W + 1), (5, 5 + 2048 - W + 1)]


@functools.lru_cache(maxsize=None)
def hand_rows():
    """One stream per stretch, FSK at 19200 bit/s inside it; then a stream with a stretch of zero products and a run
    that is constant (u = -c but for the chain's first sample: every position behind the first ties), and one that says the complement of 'mix's first word."""
    rng = np.random.default_rng(11)
    rows = np.stack([quiet(NB, 40 + s) for s in range(len(STRETCH) + 2)])
    for s, (a, b) in enumerate(STRETCH):
        rows[s, a:b] = fsk(rng.integers(0, 2, 200).tolist(), 19200)[:b - a]
    rows[-2, M - 1500:] = (3000, 0)
    rows[-2, 5000:6000:2], rows[-2, 5001:6000:2] = (0, 0), (3000, -2000)
    inv = fsk([1, 0] * 8 + [1 - v for v in word_bits(0xB2, 8)] + [0, 1] * 4, 19200, dev=40000)
    rows[-1, 3000:3000 + len(inv)] = inv
    rows.setflags(write=False)
    return rows


def corr_receiver(n, nb, bank, cap=None, **kw):
    r = hand_receiver(n, nb, (), cap=cap or (32 * n, n * nb * B), levels=False, **kw)
    r.enable_burst_corr(*BANKS[bank])
    return r


def read_corr(r, nb, st, state, prev, base, decs=None, overflow=False, max_samples=None):
    """The oldest undrained submit's records against the restatement -> (records, the state behind the submit, the samples)."""
    decs, runs, _ = R.submit_view(r, nb, decs, levels=None)
    got = r.read_burst_corrs(allow_overflow=overflow)
    assert len(got) == min(r.corr_total, r._capture[0]) and len(runs) <= len(got)
    want, nxt = corr.corrs(decs, runs, prev, st, state, r.n_streams, max_samples, base)
    same_records(got[:len(runs)], want, "corr")
    return got, nxt, decs


@functools.lru_cache(maxsize=None)
def uncut(bank, n=None):
    rows = hand_rows()
    x = rows if n is None else rows[rows_of(n, len(rows))]
    with corr_receiver(len(x), NB, bank) as r:
        r.submit(np.ascontiguousarray(x))
        got = read_corr(r, NB, corr.Settings(*BANKS[bank]), None, R.zeros(len(x)), [0] * len(x))[0]
        assert r.read_burst_corrs().tobytes() == got.tobytes()  # reading pops nothing
        r.drain()
        raises(api.E_STATE, r.read_burst_corrs)  # nothing undrained
    return got


@pytest.mark.parametrize("bank", BANKS)
def test_hand_made_runs_against_every_bank(bank):
    got = uncut(bank)
    n_pos = {(int(r["stream"]), int(r["n_samples"])): r["t"]["n_pos"].tolist() for r in got}
    K = corr.Settings(*BANKS[bank]).K
    for key, pos in n_pos.items():  # the defined positions: n - K + 1, and none below K samples
        assert pos == [max(0, key[1] - k + 1) for k in K] + [0] * (16 - len(K))
    none = got["t"]["n_pos"] == 0
    assert (got["t"]["peak"][none] == corr.NONE_PEAK).all() and (got["t"]["trough"][none] == corr.NONE_TROUGH).all()
    if bank == "chunks":
        assert [n_pos[(s, 62 + s)][:3] for s in range(4)] == [[0, 0, 0], [1, 0, 0], [2, 1, 0], [3, 2, 1]]
    if bank == "mix":
        assert [n_pos[(s, n)][1] for s, n in ((6, 1278), (7, 1279), (8, 1280))] == [255, 256, 257]
        st = corr.Settings(*BANKS[bank])
        assert corr.summary(got[got["stream"] == len(STRETCH) + 1][0], st)[1][0][0] == "-"  # the inverted word: the trough wins
        flat = got[got["stream"] == len(STRETCH)][-1]["t"]  # the constant run: the positions behind the first tie, the first of them wins
        assert flat["n_pos"].tolist()[:2] == [1341, 477] and (flat["peak_at"][:2] <= st.K).all() and (flat["trough_at"][:2] <= st.K).all()


@pytest.mark.parametrize("n", COUNTS)
def test_stream_counts_that_straddle_a_wave(n):
    got, one = uncut("mix", n), uncut("mix")
    rows = rows_of(n, len(hand_rows()))
    for s in (0, 63, 64, n - 1):
        a, b = got[got["stream"] == s], one[one["stream"] == rows[s]]
        assert a["t"].tobytes() == b["t"].tobytes() and len(a) >= 1


# ---- the history, three blocks: stream 0 an OPEN run of 3 samples continued twice (the second piece a whole block, CONTINUES and
# OPEN: the carry kernel's H' + n and the bytes it writes are read by the third submit); 1: an OPEN piece of 1000 samples continued
# twice (the carried bytes and the new ones meet in a tile); 2: a piece longer than 2047 samples (H saturates); 3: the third block alone
@functools.lru_cache(maxsize=None)
def chain_rows():
    rng = np.random.default_rng(12)
    rows = np.stack([quiet(3, 60 + s) for s in range(4)])
    for s, (a, b) in enumerate(((B - 3, 2 * B + 900), (B - 1000, 2 * B + 2000), (B - 3000, B + 500), (2 * B + 100, 2 * B + 400))):
        rows[s, a:b] = fsk(rng.integers(0, 2, 600).tolist(), 19200)[:b - a]
    rows.setflags(write=False)
    return rows


def cut_submits(bank, sizes):
    """chain_rows in submits of `sizes` blocks, all queued before the first read -> every submit's records."""
    rows, st = chain_rows(), corr.Settings(*BANKS[bank])
    got, state, prev = [], None, R.zeros(4)
    edges = np.concatenate([[0], np.cumsum(sizes)]) * B
    with corr_receiver(4, max(sizes), bank) as r:
        for a, b in zip(edges[:-1], edges[1:]):
            r.submit(np.ascontiguousarray(rows[:, a:b]))
        for a, b in zip(edges[:-1], edges[1:]):
            part = decin.clamp(rows[:, a:b])
            recs, state, decs = read_corr(r, (b - a) // B, st, state, prev, [a] * 4, decs=[part[s].reshape(-1) for s in range(4)])
            prev = R.last_pairs(decs)
            got.append(recs)
            r.drain()
    return got


@pytest.mark.parametrize("bank", ["mix", "long"])
def test_the_same_rows_in_three_queued_submits_merge_to_the_uncut_runs(bank):
    got, whole = cut_submits(bank, (1, 1, 1)), cut_submits(bank, (3,))
    both = [np.count_nonzero((g["flags"] & (CONT | OPEN)) == (CONT | OPEN)) for g in got]
    assert both == [0, 2, 0] and [np.count_nonzero(g["flags"] & CONT) for g in got] == [0, 3, 2]
    key = lambda c: (int(c["stream"]), int(c["start_sample"]))  # noqa: E731
    same_chains("corr", sorted(corr.chains(got), key=key), sorted(corr.chains(whole), key=key), "1 + 1 + 1")


def test_a_reset_mid_chain_drops_the_history():
    rows, st = chain_rows(), corr.Settings(*BANKS["mix"])
    with corr_receiver(4, 1, "mix") as r:
        r.submit(np.ascontiguousarray(rows[:, :B]))
        first, state, decs = read_corr(r, 1, st, None, R.zeros(4), [0] * 4)
        r.drain()
        r.reset_streams([1])
        state["soft"][1] = state["soft"][1][:0]
        r.submit(np.ascontiguousarray(rows[:, B:2 * B]))
        second = read_corr(r, 1, st, state, R.last_pairs(decs), [B, 0, B, B])[0]
        r.drain()
    one = second[second["stream"] == 1][0]
    assert not one["flags"] & CONT and one["t"]["n_pos"][1] == one["n_samples"] - 1023  # no history: the first 1023 positions are undefined
    assert second[second["stream"] == 2][0]["t"]["n_pos"][1] == second[second["stream"] == 2][0]["n_samples"]  # ... and with it none is


# ---- overflows, beside the other stages, a context without the call, the refusals, and tfrec_gpu -y
@pytest.mark.parametrize("cap, fits", [((5, 17 * M), 5), ((64, 700), None)])
def test_overflows_deliver_their_prefixes(cap, fits):
    rows, st = hand_rows(), corr.Settings(*BANKS["mix"])
    with corr_receiver(len(rows), NB, "mix", cap=cap) as r:
        r.submit(np.ascontiguousarray(rows))
        raises(api.E_OVERFLOW, r.read_burst_corrs)
        got = read_corr(r, NB, st, None, R.zeros(len(rows)), [0] * len(rows), overflow=True, max_samples=cap[1])[0]
        r.drain()
    assert len(got) == (fits or len(uncut("mix")))
    if fits is None:  # a run that does not fit the pool is not looked at
        assert got["t"]["n_pos"][:6].any() and not got["t"]["n_pos"][6:].any()  # (62 + 63 + 64 + 65 + 159 + 160 = 573 pairs fit)


def test_the_golden_scene_beside_the_other_stages_the_refusals_and_the_cli(tmp_path):
    x = golden_iq()
    bank = [(0x2DD4, 16, 17240), (0x2DD4, 16, 9600), (0x2DD4, 16, 8842)]
    st = corr.Settings(bank)
    with api.Receiver(1, 0x2F, 500, 0, max_blocks=4, all_flushes=True, levels=True) as r:
        plain_mem = r.memory()
        raises(api.E_INVAL, r.enable_burst_corr, bank)  # no recorder
        raises(api.E_INVAL, r.read_burst_corrs)
        assert r.memory() == plain_mem
        r.enable_capture(256, 4 * B)
        rec_mem = r.memory()
        r.submit(x)
        raises(api.E_STATE, r.enable_burst_corr, bank)  # after the first submit
        raises(api.E_INVAL, r.read_burst_corrs)  # the recorder alone
        plain_runs = r.read_captures()
        plain = r.drain()
    with api.Receiver(1, 0x2F, 500, 0, max_blocks=4, all_flushes=True, levels=True) as r:
        r.enable_capture(256, 4 * B)
        assert r.memory() == rec_mem  # a recorder without the call holds what it held
        for bad in ([], bank * 6, [(1, 7, 9600)], [(1, 65, 96000)], [(1, 8, 999)], [(1, 8, 96001)], [(1, 64, 11990)]):
            raises(api.E_INVAL, r.enable_burst_corr, bad)
        raises(api.E_INVAL, r.enable_burst_corr, bank, 192001)
        assert r.memory() == rec_mem  # a call that fails leaves the context as it was
        r.enable_burst_corr(bank)
        m = r.memory()
        assert m["device_bytes"] - rec_mem["device_bytes"] == corr.device_bytes(1, 4, 256, 4 * B, st)
        assert m["pinned_host_bytes"] == rec_mem["pinned_host_bytes"] + corr.pinned_bytes(1)
        raises(api.E_INVAL, r.enable_burst_corr, bank)  # a second call: refused, and nothing changes
        assert r.memory() == m
        r.enable_burst_band()
        r.enable_burst_clock()
        r.enable_burst_meter()
        r.submit(x)
        got, _, decs = read_corr(r, 4, st, None, R.zeros(1), [0])
        R.read_clock(r, 4, [0])
        R.read_meter(r, 4, R.zeros(1), [0])
        bands = r.read_burst_bands()
        same_records(bands, band.bands(decs, bands[list(TABLE_FIELDS)], base=[0]), "band")
        assert len(bands) == len(got) >= 2
        tab = r.read_captures()
        ev = r.drain()
    R.assert_tables(tab, plain_runs)
    R.same_events(ev, plain)
    assert len(ev) >= 1
    # tfrec_gpu -y: the scene moved 5500 samples back inside 6 blocks of silence, so that -b 2 cuts both bursts at a batch's end
    x6 = np.full(6 * api.BLOCK_BYTES, 128, dtype=np.uint8)
    x6[8 * 5500:8 * 5500 + x.shape[1]] = x[0]
    with api.Receiver(1, 0x2F, 500, 0, max_blocks=6, all_flushes=True, levels=True) as r:
        r.enable_capture(256, 6 * B)
        r.enable_burst_corr(bank)
        r.submit(x6[None])
        whole = read_corr(r, 6, st, None, R.zeros(1), [0])[0]
        r.drain()
    parity.build_cli()
    f = str(tmp_path / "tfa_2.iq")
    x6.tofile(f)
    base = ["-T", "2f", "-t", "500", "-b", "2", "-L", f]
    lines, alone = cli_lines(["-y", "2dd4@17240,2dd4@9600,2dd4@8842", "-C"] + base, "corr", "clock"), cli_lines(["-C"] + base, "corr", "clock")
    assert lines["corr"] == [corr.line(f, c, st) for c in corr.chains([whole])] and len(whole) == 2 and alone["corr"] == []
    assert lines["clock"] == alone["clock"] and lines["telegrams"] == alone["telegrams"]
