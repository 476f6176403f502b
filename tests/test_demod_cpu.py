"""The burst demodulator's restatement (tfrec_amd/demod.py), the record's size, the two exports, tfrec_gpu -w's usage
errors and its output code -- no GPU needed.  Exact integers; nothing here has a tolerance."""
import os
import subprocess

import numpy as np
import pytest

import parity
from recorder_rows import RATE, TELEGRAMS, golden_dec, quiet
from tfrec_amd import api, capture, demod

B = api.BLOCK_DEC
CONT, OPEN = capture.RUN_CONTINUES, capture.RUN_OPEN


@pytest.mark.parametrize("rate, code", [(17240, "nrz"), (96000, "nrz"), (8842, "man")])
def test_demods_against_the_per_sample_form_on_full_range_rows(rate, code):
    """Loud pairs of random direction (every soft value), zero products, a run that CONTINUES with a carried state whose first
    decision straddles the cut, a run too short for a timing, the tail behind a run's last whole decision, and the state behind."""
    rng = np.random.default_rng(5)
    z = quiet(1, 3).copy()
    z[:3000] = rng.integers(-9000, 9000, (3000, 2))
    z[1000:1100:2] = 0
    z[B - 700:] = rng.integers(-9000, 9000, (700, 2))
    runs = np.zeros(4, dtype=capture.RUN_DTYPE)
    runs["start_sample"], runs["n_samples"] = (0, 500, 2000, B - 700), (431, 1200, 7 * 384000 // rate + 3, 700)
    runs["flags"] = (CONT, 0, 0, OPEN)
    runs["pool_offset"] = np.concatenate([[0], np.cumsum(runs["n_samples"])[:-1]])
    st = demod.Settings(rate, code, 192000)  # c = 32: u = -64 .. -1
    state = {"soft": [rng.integers(-64, 64, demod.SPAN)], "ahead": [12345], "phase": [st.Pn - 1]}
    prev = [np.array([700, -900], dtype=np.int16)]
    got, pool, nxt = demod.demods([z.reshape(-1)], runs, prev, st, state)
    want, wpool, wnxt = demod.demods_bruteforce([z.reshape(-1)], runs, prev, st, state)
    assert got.tobytes() == want.tobytes() and pool.tobytes() == wpool.tobytes() and pool.any()
    assert (nxt["ahead"], nxt["phase"]) == (wnxt["ahead"], wnxt["phase"]) == ([700], [int(got[3]["phase"])]) and np.array_equal(nxt["soft"][0], wnxt["soft"][0])
    assert got["timing"].tolist() == [demod.INHERITED, demod.MEASURED, demod.FLAGGED, demod.MEASURED] and got[2]["n_timed"] < 8
    assert got[0]["first_symbol"] == st.ended(12345, st.Pn - 1) and (12345 - st.Pn + 1) * rate % 384000 >= rate  # (the first decision began ahead of the cut)
    assert got["n_symbols"].sum() == sum(len(demod.decisions_of(r, pool)) for r in got) and (got["n_symbols"] >= 7).all()
    # a pool that the third run does not fit: neither it nor the OPEN run behind it is looked at
    cut, cpool, cnxt = demod.demods([z.reshape(-1)], runs, prev, st, state, max_samples=1640)
    assert cut[:2].tobytes() == got[:2].tobytes() and len(cpool) == 1631 and not cut["timing"][2:].any() and cnxt["ahead"] == [0]


@pytest.mark.parametrize("cut, rate, code", [(2, 6000, "nrz"), (3, 6000, "nrz"), (3, 3000, "man")])
def test_a_cut_run_whose_first_piece_holds_the_timing_window_merges_to_the_uncut_run(cut, rate, code):
    dec = golden_dec("whb")  # one burst of 28344 samples from 10004: the first piece holds 6380 or 14572 of them
    st = demod.Settings(rate, code)
    assert (cut * B - 10004) >= st.g(st.Nt) + st.Pn - 1
    table = capture.captures(dec, 0x2F, 500)[0]
    recs, pool, _ = demod.demods([dec], table, [np.zeros(2, np.int16)], st)
    state, cst, prev, got = None, None, np.zeros(2, np.int16), []
    for a, b in ((0, cut), (cut, 5)):
        part = dec[2 * a * B:2 * b * B]
        runs, _, cst = capture.captures(part, 0x2F, 500, state=cst)
        r, p, state = demod.demods([part], runs, [prev], st, state, base=[a * B])
        got.append((r, p))
        prev = part.reshape(-1, 2)[-1]
    merged, whole = demod.chains(got), demod.chains([(recs, pool)])
    assert len(merged) == len(whole) == 1 and len(got[1][0]) == 1 and got[1][0][0]["timing"] == demod.INHERITED
    assert merged[0].rec.tobytes() == whole[0].rec.tobytes() and np.array_equal(merged[0].dec, whole[0].dec) and len(whole[0].dec) > 200


@pytest.mark.parametrize("name", sorted(TELEGRAMS))
def test_the_golden_fsk_scenes_read_their_telegrams(name):
    """TFA_2, TFA_3 and TX22 at their own rate, NRZ about 0 Hz: the hard bits hold 2dd4 and the telegram's bytes behind it, which the
    burst sync's test reads (and the burst track's slicer needs a smoothed track and a run-length walk for)."""
    dec = golden_dec(name)
    st = demod.Settings(RATE[name])
    recs, pool, _ = demod.demods([dec], capture.captures(dec, 0x2F, 500)[0], [np.zeros(2, np.int16)], st)
    assert len(recs) == 2 and (recs["timing"] == demod.MEASURED).all() and (recs["n_timed"] == 64).all()
    for r, telegram in zip(recs, TELEGRAMS[name]):
        text = demod.line("f", demod.Piece(r, demod.decisions_of(r, pool)), st).split()
        assert telegram in text[-1] and text[-1].startswith("aa") and 110 <= int(text[6]) <= 130, text


@pytest.mark.parametrize("offset", [0, 17, 29, 43])
def test_a_manchester_word_at_an_arbitrary_offset(offset):
    """A synthetic soft sequence: 96 random bits at 8842 bit/s, each high then low for a 1, `offset` silent samples ahead.  The
    timing finds the offset within a sample (the bit-long range of phases settles the half-bit ambiguity) and the word comes back."""
    st = demod.Settings(8842, "man")
    word = np.random.default_rng(8).integers(0, 2, 96).tolist()
    u = np.zeros(offset + st.b(2 * len(word)), dtype=np.int64)
    for i in range(2 * len(word)):
        u[offset + st.b(i):offset + st.b(i + 1)] = 40 if (i % 2 == 0) == bool(word[i // 2]) else -40
    p, timing, ns, e_best, e_sum = demod.time_phase(u, st)
    assert timing == demod.MEASURED and ns == 64 and abs(p - offset) <= 1 and e_best * st.Pn > e_sum
    n = st.ended(len(u), p)
    assert n >= len(word) - 1 and demod.bits(demod.decide(u, st, p, 0, n)) == word[:n]


def test_the_settings_the_records_size_and_the_two_exports():
    st = demod.Settings(1000, "nrz", -3001)
    assert (st.Pn, st.Nt, st.c) == (384, 21, -1) and demod.Settings(96000).g(1) == 4 and demod.Settings(17240).Pn == 23
    assert (demod.Settings(48000, "man").Rc, demod.Settings(48000, "man").Pn) == (96000, 8)
    for bad in ((999,), (96001,), (48001, "man"), (9600, "nrzi"), (9600, "nrz", 192001)):
        with pytest.raises(ValueError):
            demod.Settings(*bad)
    assert demod.DEMOD_DTYPE.itemsize == 72 and demod.DEMOD_DTYPE.fields["e_best"][1] == 40 and demod.DEMOD_DTYPE.fields["pool_offset"][1] == 64
    assert {"tfrec_amd_enable_burst_demod", "tfrec_amd_read_burst_demods"} <= set(api.EXPORTS)
    assert callable(api.Receiver.enable_burst_demod) and callable(api.Receiver.read_burst_demods)


@pytest.mark.parametrize("args, says", [(["-w", "8842,man,c=-3000"] + a, "-w") for a in (["-X", "x.hex"], ["-s", "100"], ["-A"], ["-k", "p"], ["-K", "p"])]
                         + [(["-w", b], "bad -w") for b in ("999", "96001", "48001,man", "9600,nrzi", "9600,c=192001", "9600,c=", "man", "9600,")])
def test_cli_usage_errors_are_decided_before_a_device_is_opened(args, says, tmp_path):
    """-w with what it does not work with (the argument itself, the longest accepted form, passes the parser), and arguments that the
    parser refuses."""
    parity.build_cli()
    f = tmp_path / "empty.iq"
    f.write_bytes(b"")
    out = subprocess.run([parity.CLI] + args + ["-L", str(f)], capture_output=True, text=True, timeout=60)
    assert out.returncode in (1, 2) and says in out.stderr and "hip" not in out.stderr.lower()
    assert ("bad -w" in out.stderr) == (says == "bad -w")


def test_the_hosts_merge_and_line_under_the_sanitizers(tmp_path):
    """job.h's demod_parse, demod_take, demod_add and demod_line and the merger, in a stand-alone program under ASan and UBSan: a
    chain of three pieces that crosses the 2048 decisions a line keeps, a flagged burst, one without a decision, one whose pieces
    start with an inherited timing, and a measured timing whose e_sum is 0."""
    exe = str(tmp_path / "demod_driver")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(parity.ROOT, "tests", "demod_driver.cpp")])
    st = demod.Settings(17240, "nrz", -3001)
    rng = np.random.default_rng(3)
    pieces = [(OPEN, 0, B, 5, demod.MEASURED, 90000, 1500000, rng.integers(-300, 300, 367)),
              (CONT | OPEN, B, B, 5, demod.INHERITED, 0, 0, rng.integers(-300, 300, 1678)),
              (CONT, 2 * B, 900, 5, demod.INHERITED, 0, 0, rng.integers(-300, 300, 40)),
              (0, 30000, 100, 0, demod.FLAGGED, 0, 0, np.array([7, -7, 0, 1])), (0, 40000, 3, 0, demod.FLAGGED, 0, 0, np.zeros(0)),
              (CONT, 50000, 700, 21, demod.INHERITED, 0, 0, np.array([-1, 2, 3, -4, 5])), (0, 60000, 4000, 0, demod.MEASURED, 0, 0, np.zeros(9))]
    recs = []
    for flags, start, n, phase, timing, e_best, e_sum, dec in pieces:
        r = np.zeros((), dtype=demod.DEMOD_DTYPE)
        r["flags"], r["start_sample"], r["n_samples"], r["phase"], r["timing"] = flags, start, n, phase, timing
        r["e_best"], r["e_sum"], r["n_symbols"] = e_best, e_sum, len(dec)
        recs.append(demod.Piece(r, dec))
    want = [demod.line("f", c, st) for c in [demod.merge(recs[:3])] + recs[3:]]
    text = "".join("%d %d %d %d %d %d %d %d %s\n" % (p[:7] + (len(p[7]), " ".join("%d" % d for d in p[7]))) for p in pieces)
    out = subprocess.run([exe, "17240,nrz,c=-3001"], input=text, capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stderr == "" and out.stdout.splitlines() == want
    assert want[0].split()[2:8] == ["0", str(2 * B + 900), "5", "m", "138", "2085+"] and len(want[0].split()[8]) == 512
    assert want[1].endswith(" 0 f - 4 9") and want[2].endswith(" 0 f - 0 -") and want[3].endswith(" 21 i - 5 68") and want[4].endswith(" 0 m - 9 000")
