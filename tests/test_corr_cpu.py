"""The burst correlator's restatement (tfrec_amd/corr.py), the record's size, the two exports,
tfrec_gpu -y's usage errors and its output code -- no GPU needed.  Exact integers; nothing here has a tolerance."""
import os
import subprocess

import numpy as np
import pytest

import parity
from recorder_rows import GOLDEN, PLATEAUS, RATE, fsk, golden_dec, quiet, word_bits
from tfrec_amd import api, capture, corr

B = api.BLOCK_DEC
CONT, OPEN = capture.RUN_CONTINUES, capture.RUN_OPEN
BANK = [(0x2DD4, 16, 17240), (0x2DD4, 16, 9600), (0x2DD4, 16, 8842), (0xAA2DD4, 24, 17240), (0x2DD4, 16, 38400), (0x2DD4, 16, 6000)]


def test_a_template_whose_symbols_have_unequal_lengths():
    t = corr.template(0b10110010, 8, 17240)  # b = 0, 22, 44, 66, 89, 111, 133, 155, 178
    assert len(t) == 178 and t.tolist() == [1] * 22 + [-1] * 22 + [1] * 45 + [-1] * 44 + [1] * 22 + [-1] * 23
    st = corr.Settings([(0x2DD4, 16, 17240), (0xAA, 8, 48761)], -3001)
    assert st.K == [356, 63] and st.Kp == 384 and st.c == -1
    for bad in ([], [(1, 7, 9600)], [(1, 8, 999)], [(1, 64, 11990)], [(1, 8, 9600)] * 17):
        with pytest.raises(ValueError):
            corr.Settings(bad)
    with pytest.raises(ValueError):
        corr.Settings(BANK, 192001)


def test_corrs_against_the_per_position_form_on_crafted_rows():
    """An FSK word and its complement, a constant stretch, zero products, a run shorter than a template, one that CONTINUES at the
    submit's first sample with a history, and the state behind the submit."""
    z = quiet(1, 3).copy()
    z[100:279] = fsk(word_bits(0xB2, 8), 17240)
    z[600:900] = (3000, 0)
    z[1000:1100:2] = 0
    z[2000:2179] = fsk([1 - b for b in word_bits(0xB2, 8)], 17240, dev=35000)
    runs = np.zeros(5, dtype=capture.RUN_DTYPE)
    runs["start_sample"], runs["n_samples"] = (0, 500, 950, 1990, B - 300), (400, 450, 200, 100, 300)
    runs["flags"] = (CONT, 0, 0, 0, OPEN)
    runs["pool_offset"] = np.concatenate([[0], np.cumsum(runs["n_samples"])[:-1]])
    st = corr.Settings([(0xB2, 8, 17240), (0xB2B2, 16, 38400), (0x4D, 8, 17240)], 20000)
    state = {"soft": [np.arange(-60, 40, dtype=np.int64)]}
    prev = [np.array([7, -9], dtype=np.int16)]
    got, nxt = corr.corrs([z.reshape(-1)], runs, prev, st, state)
    want, wnxt = corr.corrs_bruteforce([z.reshape(-1)], runs, prev, st, state)
    assert got.tobytes() == want.tobytes() and np.array_equal(nxt["soft"][0], wnxt["soft"][0]) and len(nxt["soft"][0]) == 300
    assert got[0]["t"]["n_pos"][:3].tolist() == [400 - 77, 400 - 59, 400 - 77] and got[3]["t"]["n_pos"][0] == 0
    assert got[3]["t"]["peak"][0] == corr.NONE_PEAK and got[3]["t"]["trough"][0] == corr.NONE_TROUGH and not got["t"]["n_pos"][:, 3:].any()
    some = [0, 1, 2, 4]
    assert (got["t"]["peak"][some, 0] == -got["t"]["trough"][some, 2]).all()  # the complemented word: the mirror image
    # a pool that the fourth run does not fit: not looked at, and the OPEN run behind it leaves no history
    cut, cnxt = corr.corrs([z.reshape(-1)], runs, prev, st, state, max_samples=1100)
    assert cut[:3].tobytes() == got[:3].tobytes() and not cut["t"]["n_pos"][3:].any() and len(cnxt["soft"][0]) == 0


@pytest.mark.parametrize("cut", range(1, 4))
def test_merged_chains_are_the_uncut_streams(cut):
    dec = golden_dec("tfa_2")
    st = corr.Settings(BANK)
    table = capture.captures(dec, 0x2F, 500)[0]
    whole = corr.corrs([dec], table, [np.zeros(2, np.int16)], st)[0]
    state, cst, prev, got = None, None, np.zeros(2, np.int16), []
    for a, b in ((0, cut), (cut, 4)):
        part = dec[2 * a * B:2 * b * B]
        runs, _, cst = capture.captures(part, 0x2F, 500, state=cst)
        recs, state = corr.corrs([part], runs, [prev], st, state, base=[a * B])
        got.append(recs)
        prev = part.reshape(-1, 2)[-1]
    merged = corr.chains(got)
    assert len(merged) == len(whole) and all(m.tobytes() == w.tobytes() for m, w in zip(merged, whole))


def test_the_records_size_and_the_two_exports():
    assert corr.CORR_DTYPE.itemsize == 536 and corr.CORR_DTYPE.fields["t"][1] == 24 and corr.SCORE_DTYPE.fields["sum_abs"][1] == 24
    assert {"tfrec_amd_enable_burst_corr", "tfrec_amd_read_burst_corrs"} <= set(api.EXPORTS)
    assert callable(api.Receiver.enable_burst_corr) and callable(api.Receiver.read_burst_corrs)


# -y with what it does not work with, and banks that the parser refuses
BAD_BANKS = ["2dd4", "2dd4@999", "2@9600", "2dd4@9600,c=200000", "c=0", "2dd4@9600,c=0,2dd4@9600", "ffffffffffffffff@11990", ",".join(["aa@9600"] * 17)]


@pytest.mark.parametrize("args, says", [(["-y", "2dd4@9600"] + a, "-y") for a in (["-X", "x.hex"], ["-s", "100"], ["-A"], ["-k", "p"], ["-K", "p"])]
                         + [(["-y", b], "bad -y") for b in BAD_BANKS])
def test_cli_usage_errors_are_decided_before_a_device_is_opened(args, says, tmp_path):
    parity.build_cli()
    f = tmp_path / "empty.iq"
    f.write_bytes(b"")
    out = subprocess.run([parity.CLI] + args + ["-L", str(f)], capture_output=True, text=True, timeout=60)
    assert out.returncode in (1, 2) and says in out.stderr and "hip" not in out.stderr.lower()


# what the restatement gives for every trigger window of the five golden scenes with BANK about 0 Hz (DESIGN.md 6ze holds the same
# table): <start_sample> <n_samples> <best> <end_sample> <+|-> <dev_hz> <quality_c> <dev_hz of every template>
GOLDEN_LINES = {
    "tfa_1": ["10004 4056 4 13497 - 12075 1115 11308,5362,5100,7426,12075,4927", "28315 4056 4 31831 - 14137 1199 9252,6759,6510,7528,14137,4980"],
    "tfa_2": ["10003 2167 0 10539 + 23747 655 23747,12506,10711,22707,12825,10710", "25583 2168 0 26119 + 37786 686 37786,18084,19374,35943,19762,15046"],
    "tfa_3": ["10004 3976 1 11604 + 37434 616 19297,37434,26403,14471,18525,26548", "24647 3977 1 26248 + 34546 669 16500,34546,24043,13426,17625,17203"],
    "tx22": ["10004 4605 2 11394 + 36925 647 19971,27028,36925,15033,19012,26496", "24737 5300 2 26127 + 38982 663 19820,28603,38982,15359,20137,22259"],
    "whb": ["10004 28344 4 37938 + 11700 1124 8544,6018,3700,7213,11700,2736"],
}


@pytest.mark.parametrize("name", GOLDEN)
def test_the_golden_scenes_lines_and_the_stages_point(name):
    """The pinned table; and in each FSK run the best template is the scene's own rate with the word 2dd4 or aa2dd4, its end within
    one symbol of the end of the burst sync's plateau, where a window that ends with the word's last symbol should be."""
    dec = golden_dec(name)
    st = corr.Settings(BANK)
    recs = corr.corrs([dec], capture.captures(dec, 0x2F, 500)[0], [np.zeros(2, np.int16)], st)[0]
    assert [corr.line("f", r, st) for r in recs] == ["corr f " + ln for ln in GOLDEN_LINES[name]]
    for r, plateau in zip(recs, PLATEAUS.get(name, ())):
        best, fig = corr.summary(r, st)
        assert BANK[best][2] == RATE[name] and BANK[best][0] in (0x2DD4, 0xAA2DD4)
        assert abs(fig[best][3] - plateau[1]) <= -(-384000 // RATE[name])


def test_the_hosts_merge_summary_and_line_under_the_sanitizers(tmp_path):
    """job.h's corr_parse, corr_add, corr_summary and corr_line and the merger, in a stand-alone program under ASan and UBSan: a
    chain of two pieces with a tie (the earlier piece's wins) and a later, lower trough; a trough that wins (polarity -); a tie of
    two templates' dev_hz (the lower index); sum_abs of 0; scores that are all negative; and a record with no position."""
    exe = str(tmp_path / "corr_driver")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(parity.ROOT, "tests", "corr_driver.cpp")])
    st = corr.Settings([(0x2DD4, 16, 17240), (0x2DD4, 16, 9600), (0xAA, 8, 48000)], -3001)
    pieces = [(OPEN, 0, B, {0: (900, 40, -300, 7, 7000, 350000), 2: (64, 63, -64, 70, 8129, 90000)}),
              (CONT, B, 900, {0: (900, 3, -301, 5, 900, 40000), 1: (10, 639, 10, 639, 1, 10)}),
              (0, 20000, 5000, {0: (500, 9, -2000, 444, 4000, 123456), 1: (1280, 700, -100, 9, 4000, 99999)}),
              (0, 30000, 5000, {0: (712, 1, -5, 2, 10, 0), 1: (1280, 5, -1280, 4, 10, 7)}),
              (0, 40000, 700, {1: (-50, 650, -50, 650, 1, 50)}), (0, 50000, 10, {})]
    recs = []
    for flags, start, n, scores in pieces:
        r = np.zeros((), dtype=corr.CORR_DTYPE)
        r["flags"], r["start_sample"], r["n_samples"] = flags, start, n
        r["t"]["peak"], r["t"]["trough"] = corr.NONE_PEAK, corr.NONE_TROUGH
        for t, v in scores.items():
            x = r["t"][t]
            x["peak"], x["peak_at"], x["trough"], x["trough_at"], x["n_pos"], x["sum_abs"] = v
        recs.append(r)
    chain = corr.merge(recs[:2])
    assert tuple(chain["t"][0].tolist())[:5] == (900, 40, -301, B + 5, 7900) and int(chain["t"][1]["peak_at"]) == B + 639
    want = [corr.line("f", c, st) for c in [chain] + recs[2:]]
    text = "".join("%d %d %d %s\n" % (p[:3] + (" ".join("%d:" % t + ":".join("%d" % x for x in v) for t, v in p[3].items()),)) for p in pieces)
    out = subprocess.run([exe, "2dd4@17240,2dd4@9600,aa@48000,c=-3001"], input=text, capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stderr == "" and out.stdout.splitlines() == want
    assert want[1].split()[4:7] == ["0", "20444", "-"] and want[2].split()[4:9] == ["0", "30001", "+", "12000", "-"]
    assert want[3].endswith(" 1 40650 - 468 100 -,468,-") and want[4].endswith(" - - - - - -,-,-")
