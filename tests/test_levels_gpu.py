"""The level meter on the GPU (TFREC_AMD_F_LEVELS, tfrec_amd_read_levels, tfrec_gpu -s), bit for bit.

Every record is compared with the restatement tfrec_amd/levels.py run on the context's OWN decimated samples
(tfrec_amd_read_decimated), so the front end ahead of the meter is whatever the context runs; the events still equal the
oracle's.  Three streams of four blocks: near-silence, crafted bursts (a trigger at the last sample of block 0, a window across
the boundary between blocks 1 and 2), and noise loud enough to move an auto threshold."""
import functools
import os
import subprocess

import numpy as np
import pytest

import parity
from input_rows import input_oracle, tuned_stage0
from meter_rows import scan_file
from oracle import oracle as O
from recorder import same_records
from tfrec_amd import api, levels, resample, synth, tune

pytestmark = pytest.mark.gpu

B = api.BLOCK_DEC
TYPES = 0x2F
NB = 4


def oracle_dec(x, n_blocks):
    o = O.Oracle(TYPES, 500, 0, keep_dec=True)
    o.process(x[:n_blocks * api.BLOCK_BYTES])
    d = o.dec().reshape(-1, 2).astype(np.int64)
    return np.abs(d[:, 0]) + np.abs(d[:, 1])


@functools.lru_cache(maxsize=None)
def scene():
    """[3, 4 blocks] u8 at 1.536 MS/s.  Stream 1: a carrier burst whose end is moved, raw sample by raw sample, until the oracle's
    front end puts its last sample above 500 at decimated sample 8191; a second one 100 decimated samples ahead of block 2."""
    rng = np.random.default_rng(5)
    n = NB * api.BLOCK_BYTES
    quiet = rng.integers(126, 131, n, dtype=np.uint8)
    loud = rng.integers(0, 256, n, dtype=np.uint8)
    base = rng.integers(126, 131, n, dtype=np.uint8)

    def burst(x, end, length):
        x[2 * (end - length):2 * end:2] = 228
        x[2 * (end - length) + 1:2 * end:2] = 128

    found = None
    for end in range(4 * B - 80, 4 * B + 80):
        x = base.copy()
        burst(x, end, 600)
        over = np.flatnonzero(oracle_dec(x, 2) > 500)
        if len(over) and over[-1] == B - 1:
            found = x
            break
    assert found is not None
    burst(found, 4 * (2 * B - 100), 200)
    burst(found, 4 * (3 * B + 3000), 3000)
    return np.stack([quiet, found, loud])


def want_levels(decs, types, thresh, states):
    """The restatement on one submit's decimated samples, per stream; states: each stream's carried state (None: fresh), updated."""
    out = []
    for s, d in enumerate(decs):
        rec, states[s] = levels.levels(d, types[s], thresh[s], states[s])
        out.append(rec)
    return np.stack(out)


def run_levels(r, parts, types, thresh, before=None, states=None):
    """Submit the parts one by one -> (records read per submit, the restatement's, events drained per submit, the final states)."""
    n = r.n_streams
    states = [None] * n if states is None else states
    got, want, evs = [], [], []
    for k, p in enumerate(parts):
        if before:
            before(k, states)
        nb = r.submit(p)
        decs = [r.decimated(s, nb * B) for s in range(n)]
        lv = r.read_levels()
        assert lv.shape == (n, nb) and lv.dtype == levels.LEVEL_DTYPE
        got.append(lv)
        want.append(want_levels(decs, types, thresh, states))
        evs.append(r.drain())
    return got, want, evs, states


@functools.lru_cache(maxsize=None)
def base_run(thresh, sizes, serial=False):
    iq = scene()
    with api.Receiver(3, TYPES, thresh, 0, max_blocks=NB, all_flushes=True, levels=True, serial_chains=serial) as r:
        got, want, evs, _ = run_levels(r, parity.cut(iq, sizes), [TYPES] * 3, [thresh] * 3)
        th = [r.thresh(s) for s in range(3)]
    return np.concatenate(got, axis=1), np.concatenate(want, axis=1), np.concatenate(evs), th


@pytest.mark.parametrize("thresh", [500, 0])
def test_records_equal_the_restatement_however_the_stream_is_cut(thresh):
    one, want, ev, _ = base_run(thresh, (4,))
    cut, want_cut, ev_cut, _ = base_run(thresh, (1, 3))
    same_records(one, want, "one submit")
    same_records(cut, want_cut, "1 + 3")
    assert one.tobytes() == cut.tobytes()
    # the scene is what it is meant to be
    assert one["triggered"][0].sum() == 0 and one["n_over"][0].sum() == 0 and one["pwr_max"][0].max() < 500
    # (the noise triggers from the front end's first full-length outputs on: all but a few samples of block 0)
    assert (one["triggered"][2][1:] == B).all() and one["triggered"][2][0] >= B - 16 and one["triggered_avg"][2][-1] >= 512
    W = max(levels.windows(TYPES))
    # stream 1: the window of the trigger at block 0's last sample lies in block 1, the next one spans blocks 1 and 2
    assert one["triggered"][1][1] >= (W - 1) + 50 and 0 < one["triggered"][1][2] < W + 3200
    assert (one["thresh"] == 500).all()  # (an auto threshold moves after every 4th block: test_auto_...)
    for s in range(3):
        parity.assert_stream(ev, s, parity.fresh_oracle(scene()[s], TYPES, thresh), "stream %d" % s)
    assert parity.sort_events(ev).tobytes() == parity.sort_events(ev_cut).tobytes()


def test_stream_1_triggers_at_the_last_sample_of_block_0():
    """... on the context's own decimated samples, not only in the oracle's."""
    with api.Receiver(3, TYPES, 500, 0, max_blocks=NB, levels=True) as r:
        r.submit(scene())
        d = r.decimated(1, NB * B).reshape(-1, 2).astype(np.int64)
        lv = r.read_levels()
        r.drain()
    pwr = np.abs(d[:, 0]) + np.abs(d[:, 1])
    over = np.flatnonzero(pwr > 500)
    W = max(levels.windows(TYPES))
    assert pwr[B - 1] > 500 and not (pwr[B:B + W] > 500).any()
    first = over[over < B][0]
    assert lv["triggered"][1][0] == B - first and lv["triggered"][1][1] == (W - 1) + (2 * B - over[(over >= B) & (over < 2 * B)][0])
    assert lv["n_over"][1].tolist() == [int(((over >= b * B) & (over < (b + 1) * B)).sum()) for b in range(NB)]
    assert int(lv["energy"][1].sum()) == int((d * d).sum()) and lv["pwr_max"][1].max() == pwr.max()


def test_auto_thresholds_are_the_ones_threshold_kernel_used():
    """The last record's thresh, stepped once more by the recurrence, is tfrec_amd_read_thresh: FskState's, which the meter never
    reads."""
    for sizes in ((4,), (1, 3)):
        got, _, _, th = base_run(0, sizes)
        assert [levels.next_thresh(got[s][-1], True, NB) for s in range(3)] == th
        assert th[0] == 498 and th[2] == 502  # silence lowers it, noise raises it
    got, _, _, th = base_run(500, (4,))
    assert th == [500, 500, 500] and [levels.next_thresh(got[s][-1], False, NB) for s in range(3)] == th


def test_read_levels_follows_the_fifo():
    want, _, _, _ = base_run(0, (1, 3))
    iq = scene()
    with api.Receiver(3, TYPES, 0, 0, max_blocks=NB, all_flushes=True, levels=True) as r:
        for p in parity.cut(iq, (1, 3)):
            r.submit(p)
        first = r.read_levels()
        assert first.shape == (3, 1) and first.tobytes() == np.ascontiguousarray(want[:, :1]).tobytes()
        assert r.read_levels().tobytes() == first.tobytes()  # reading pops nothing
        # too little room, or no pointer: E_INVAL, and nothing is written
        buf = np.full(3 * 1, 0x55, dtype=np.uint8).repeat(32).view(levels.LEVEL_DTYPE)
        nb = api.C.c_int(-7)
        assert r.L.tfrec_amd_read_levels(r.h, buf.ctypes.data, 2, api.C.byref(nb)) == api.E_INVAL
        assert r.L.tfrec_amd_read_levels(r.h, None, 3, api.C.byref(nb)) == api.E_INVAL
        assert r.L.tfrec_amd_read_levels(r.h, buf.ctypes.data, 3, None) == api.E_INVAL
        assert nb.value == -7 and (buf.view(np.uint8) == 0x55).all()
        assert r.L.tfrec_amd_read_levels(r.h, buf.ctypes.data, 3, api.C.byref(nb)) == api.E_OK and nb.value == 1
        assert buf.tobytes() == first.tobytes()
        r.drain()
        second = r.read_levels()
        assert second.shape == (3, 3) and second.tobytes() == np.ascontiguousarray(want[:, 1:]).tobytes()
        r.drain()
        with pytest.raises(api.TfrecAmdError) as e:
            r.read_levels()
        assert e.value.code == api.E_STATE
        assert r.L.tfrec_amd_read_levels(None, buf.ctypes.data, 3, api.C.byref(nb)) == api.E_INVAL


def test_a_reset_restarts_the_level_state_of_that_stream_alone():
    iq = scene()
    two = np.concatenate([iq, iq[:, ::-1][:, :2 * api.BLOCK_BYTES]], axis=1)  # 6 blocks: 4 + 2 (auto: runs 4 is reached in the first)

    def before(k, states):
        if k == 1:
            r.reset_streams([1])
            states[1] = None  # a fresh stream on the input that follows

    with api.Receiver(3, TYPES, 0, 0, max_blocks=NB, all_flushes=True, levels=True) as r:
        got, want, evs, _ = run_levels(r, parity.cut(two, (4, 2)), [TYPES] * 3, [0] * 3, before=before)
        assert [r.thresh(s) for s in range(3)] == [int(got[1][s][-1]["thresh"]) for s in range(3)]  # (runs 6 and 2: no step)
    for k in range(2):
        same_records(got[k], want[k], "submit %d" % k)
    assert got[1]["thresh"].tolist() == [[498, 498], [500, 500], [502, 502]]
    assert got[1]["triggered_avg"][1][0] == got[1]["triggered"][1][0] // 32  # from zero again
    assert got[1]["triggered_avg"][2][0] == (31 * int(got[0]["triggered_avg"][2][-1]) + B) // 32  # carried on
    cutb = 4 * api.BLOCK_BYTES
    for s in (0, 2):
        parity.assert_stream(np.concatenate(evs), s, parity.fresh_oracle(two[s], TYPES, 0), "stream %d" % s)
    parity.assert_segment(evs[0], 1, parity.fresh_oracle(two[1][:cutb], TYPES, 0), "stream 1 before the reset")
    parity.assert_segment(evs[1], 1, parity.fresh_oracle(two[1][cutb:], TYPES, 0), "stream 1 after the reset")


def test_triggered_follows_each_streams_own_window():
    """A 0x2f context whose streams all read the crafted input: stream 0 configured to TFA_1 alone (W = 400), stream 2 to TX22
    alone (W = 694, and auto), stream 1 left with every demodulator (694)."""
    iq = np.stack([scene()[1]] * 3)
    types, thresh = [0x01, TYPES, 0x08], [500, 500, 0]
    with api.Receiver(3, TYPES, 500, 0, max_blocks=NB, all_flushes=True, levels=True) as r:
        r.configure_streams([0, 2], types_mask=[0x01, 0x08], thresh=[500, 0])
        got, want, evs, _ = run_levels(r, parity.cut(iq, (2, 2)), types, thresh)
        th2 = r.thresh(2)
    got, want, ev = np.concatenate(got, axis=1), np.concatenate(want, axis=1), np.concatenate(evs)
    same_records(got, want)
    assert np.array_equal(got["n_over"][0], got["n_over"][1]) and np.array_equal(got["energy"][0], got["energy"][2])
    assert got["triggered"][1][1] - got["triggered"][0][1] >= 694 - 400  # the window behind block 0's last sample, at least
    assert (got["triggered"][0] <= got["triggered"][1]).all() and got["triggered"][2].tolist() == got["triggered"][1].tolist()
    assert th2 == levels.next_thresh(got[2][-1], True, NB)
    for s in range(3):
        parity.assert_stream(ev, s, parity.fresh_oracle(iq[s], types[s], thresh[s]), "stream %d" % s)


def test_the_scans_configuration_on_a_rate_context():
    """create_rate(4, 3), three streams on row 0: an input tune beyond 768 kHz, a tune behind the stage, and none."""
    p, q, nb = 4, 3, 3
    rng = np.random.default_rng(8)
    n = resample.input_samples(nb, p, q)
    row = synth.gen_scene(41, nb, [dict(proto=1, start=5000 * p, payload_seed=5, f0_hz=300000, amp=60),
                                   dict(proto=2, start=35000 * p, payload_seed=6, f0_hz=0, amp=60),
                                   dict(proto=0, start=65000 * p, payload_seed=7, f0_hz=-900000, amp=60)],
                          rate_mult=p).reshape(-1, 2)[::q]
    row = np.ascontiguousarray(row).reshape(1, -1)
    assert row.shape[1] == 2 * n
    hz_in, hz_behind = [-900000, 0, 0], [0, 300000, 0]
    with api.Receiver(3, TYPES, 500, 0, max_blocks=nb, all_flushes=True, levels=True, input_rate=(p, q)) as r:
        r.map_streams([0, 1, 2], [0, 0, 0])
        r.tune_streams_input([0], [hz_in[0]])
        r.tune_streams([1], [hz_behind[1]])
        got, want, evs, _ = run_levels(r, [row], [TYPES] * 3, [500] * 3)
    same_records(got[0], want[0])
    assert (got[0]["triggered"].sum(axis=1) > 0).all()
    tele = []
    for s in range(3):
        orc = input_oracle(row[0], p, q, hz_in[s], hz_behind[s])
        parity.assert_stream(evs[0], s, orc, "stream %d" % s)
        tele.append(sum(1 for e in orc.events_full() if e[7] == 1))
    assert all(t >= 1 for t in tele), tele


def test_a_10x_context_and_a_serial_one():
    iq10 = np.stack([synth.gen_stream(9, s, 1, rate_mult=10) for s in range(2)])
    with api.Receiver(2, TYPES, 0, 0, max_blocks=1, all_flushes=True, levels=True, input_10x=True) as r:
        got, want, evs, _ = run_levels(r, [iq10], [TYPES] * 2, [0] * 2)
    same_records(got[0], want[0], "10x")
    assert got[0].shape == (2, 1) and got[0]["energy"].min() > 0
    for s in range(2):
        parity.assert_stream(evs[0], s, parity.fresh_oracle(iq10[s], TYPES, 0, in10x=True), "10x stream %d" % s)
    ser, want, ev, th = base_run(0, (1, 3), True)
    same_records(ser, want, "serial")
    assert ser.tobytes() == base_run(0, (1, 3))[0].tobytes() and th == base_run(0, (1, 3))[3]
    for s in range(3):
        parity.assert_stream(ev, s, parity.fresh_oracle(scene()[s], TYPES, 0), "serial stream %d" % s)


def test_without_the_flag_nothing_is_held_and_the_call_is_refused():
    n, mb = 3, 5
    with api.Receiver(n, TYPES, 500, 0, max_blocks=mb) as r:
        plain = r.memory()
        with pytest.raises(api.TfrecAmdError) as e:
            r.read_levels()
        assert e.value.code == api.E_INVAL
        r.submit(scene())
        with pytest.raises(api.TfrecAmdError) as e:
            r.read_levels()
        assert e.value.code == api.E_INVAL
        r.drain()
    with api.Receiver(n, TYPES, 500, 0, max_blocks=mb, levels=True) as r:
        flagged = r.memory()
    # one record buffer per FIFO slot and the carried LevelState (16 bytes per stream); no host copy
    assert flagged["device_bytes"] - plain["device_bytes"] == api.FIFO_DEPTH * n * mb * 32 + n * 16
    assert flagged["pinned_host_bytes"] == plain["pinned_host_bytes"]


def test_cli_scan_finds_the_channel(tmp_path):
    cli = parity.build_cli()
    x = scan_file()
    f = tmp_path / "scan.iq"
    x.tofile(f)
    c = 868250
    out = subprocess.run([cli, "-s", "100", "-r", "2048000", "-c", str(c), "-T", "2f", "-t", "500", "-b", "3", "-D", "-L", str(f)],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("scan ")]
    chans = levels.scan_channels(c, 100, 2048000)
    assert [int(ln.split()[1]) for ln in lines] == chans and len(chans) == 17 and c + 600 in chans
    assert len(out.stdout.splitlines()) == len(chans) * (1 + 3)  # no telegram text: the table and, with -D, a line per block
    field = lambda ln, k: int(dict(p.split("=") for p in ln.split()[2:])[k])  # noqa: E731
    # the restatement of the channel at c + 600: the tune behind the resampler, the oracle's front end, levels.py
    o = O.Oracle(TYPES, 500, 0, keep_dec=True)
    o.process_s16(tune.mix_s16(tuned_stage0(x, 4, 3, 0), 600000, 0))
    rec, _ = levels.levels(o.dec(), TYPES, 500)
    telegrams = sum(1 for e in o.events_full() if e[7] == 1 and e[1] < 3 * B)
    assert telegrams >= 1
    mine = lines[chans.index(c + 600)]
    assert mine == levels.scan_line(c + 600, rec, telegrams)
    per_block = [ln for ln in out.stdout.splitlines() if ln.startswith("%d Trigger ratio " % (c + 600))]
    assert per_block == ["%d Trigger ratio %d/8192, avg %d" % (c + 600, r["triggered"], r["triggered_avg"]) for r in rec]
    for k, ln in zip(chans, lines):
        assert field(ln, "blocks") == 3
        if abs(k - (c + 600)) > 100:
            assert field(ln, "telegrams") == 0, ln


def test_cli_scan_with_capture(tmp_path):
    """-S beside -s: the table is the one of the scan alone, the channel that carries the scene has its trigger windows in
    <prefix>.<channel index>.cs16 -- as many samples as its .idx lines count -- and a channel that never triggered has no file."""
    cli = parity.build_cli()
    f = tmp_path / "scan.iq"
    scan_file().tofile(f)
    c = 868250
    args = ["-s", "100", "-r", "2048000", "-c", str(c), "-T", "2f", "-t", "500", "-b", "3", "-L", str(f)]
    pre = str(tmp_path / "cap")
    plain = subprocess.run([cli] + args, capture_output=True, text=True, timeout=300)
    out = subprocess.run([cli, "-S", pre] + args, capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0 and out.returncode == 0, out.stderr
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("scan ")]
    chans = levels.scan_channels(c, 100, 2048000)
    assert lines == [ln for ln in plain.stdout.splitlines() if ln.startswith("scan ")] and len(lines) == len(chans)
    idx = [ln.split() for ln in open(pre + ".idx").read().splitlines()]
    mine = chans.index(c + 600)
    n_samples = sum(int(ln[3]) for ln in idx if int(ln[0]) == mine)
    assert n_samples >= 1 and os.path.getsize(pre + ".%d.cs16" % mine) == 4 * n_samples
    field = lambda ln, k: int(dict(p.split("=") for p in ln.split()[2:])[k])  # noqa: E731
    quiet = [i for i, ln in enumerate(lines) if field(ln, "triggered") == 0]
    assert quiet  # (the channels far from the scene never trigger at -t 500)
    for i in quiet:
        assert not os.path.exists(pre + ".%d.cs16" % i), lines[i]
    # ... and a file exists exactly for the channels that have a run
    assert [i for i in range(len(chans)) if os.path.exists(pre + ".%d.cs16" % i)] == sorted(set(int(ln[0]) for ln in idx))
