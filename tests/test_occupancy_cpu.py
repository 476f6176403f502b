"""The occupancy detector without a GPU (tfrec_amd_enable_occupancy, tfrec_gpu -A): the restatement against a direct
evaluation of the definition in Python ints, the thresholds' edges, what it finds on noise and on the scan file, the grouping of
hits into channels, and what tfrec_gpu decides before it opens a device.
"""
import functools
import re

import numpy as np
import pytest

import parity
from meter_rows import scan_file
from tfrec_amd import api, occupancy, spectrum


def direct(s, p, nf, ratio, rel):
    """The definition, one record and one bin at a time."""
    recs, words = [], []
    for sr, pr, f in zip(s.tolist(), p.tolist(), nf.tolist()):
        n = len(sr)
        m = sorted(v // f for v in sr)
        floor = m[n // 2 - 1]
        top = max(pr)
        hit = [v > max(floor, 1) * ratio and v * rel >= top for v in pr]
        recs.append((floor, sum(hit), f))
        words.append([sum(int(hit[32 * w + b]) << b for b in range(32)) for w in range(n // 32)])
    return recs, words


def assert_equals_direct(s, p, nf, ratio, rel):
    recs, bits = occupancy.occupancy(s, p, nf, ratio, rel)
    want_recs, want_words = direct(s, p, nf, ratio, rel)
    assert recs.dtype == occupancy.OCC_DTYPE and bits.dtype == np.uint32 and bits.shape == (len(nf), s.shape[1] // 32)
    assert recs.tolist() == want_recs and bits.tolist() == want_words
    hit = occupancy.unpack(bits, s.shape[1])
    assert hit.sum(axis=1).tolist() == [r[1] for r in want_recs]
    assert np.array_equal(occupancy.pack(hit), bits)
    return recs, hit


def test_restatement_equals_the_direct_definition():
    rng = np.random.default_rng(21)
    n = 64
    nf = np.array([7, 3, 1, 16384, 5, 9, 11], dtype=np.uint32)
    p = rng.integers(0, 1 << 20, (len(nf), n)).astype(np.uint64)
    s = (p * nf[:, None].astype(np.uint64)) // np.uint64(2) + rng.integers(0, 7, p.shape).astype(np.uint64)  # n_frames does not divide them
    assert (s % nf[:, None] != 0).any()
    p[0, 5] = (1 << 49) - 1                    # the largest peak there is
    s[1] = (s[1] // np.uint64(1 << 16)) * np.uint64(3)  # many equal m values (a few distinct ones), ...
    s[2, :] = 1000                             # ... and all m equal
    p[2, 17] = 1 << 30
    s[4], p[4] = 0, 0                          # an all-zero record: floor 0, nothing hits
    s[5], p[5] = 0, 0                          # a single non-zero bin: the median is 0, the clamp to 1 decides
    s[5, 40], p[5, 40] = 9 * 40, 40
    for ratio, rel in ((32, 16), (2, 1), (4096, 4096), (2, 4096), (4096, 1)):
        recs, hit = assert_equals_direct(s, p, nf, ratio, rel)
        assert recs["floor"][4] == 0 and recs["n_hit"][4] == 0
        assert recs["floor"][5] == 0 and hit[5].tolist() == [k == 40 and 40 > ratio for k in range(n)]
    assert len(np.unique(s[1] // np.uint64(3))) < n // 2


@pytest.mark.parametrize("ratio,rel", [(2, 1), (4096, 4096), (2, 4096), (4096, 1), (32, 16)])
def test_values_on_and_one_above_each_threshold(ratio, rel):
    """> against the floor, >= against the top."""
    n, floor = 64, 1000
    s = np.full((1, n), floor * 10 + 3, dtype=np.uint64)  # 10 frames: m = 1000 everywhere
    nf = np.array([10], dtype=np.uint32)
    top = floor * ratio * rel * 4 + 1  # far above the floor test for every bin placed below; not a multiple of rel
    assert top < 1 << 49
    p = np.zeros((1, n), dtype=np.uint64)
    p[0, 0] = top
    p[0, 1] = floor * ratio            # on the floor threshold: no hit
    p[0, 2] = floor * ratio + 1        # one above: a hit, if the top test lets it
    p[0, 3] = -(-top // rel)           # the smallest value with p * rel >= top: a hit
    p[0, 4] = -(-top // rel) - 1       # one below: no hit
    recs, hit = assert_equals_direct(s, p, nf, ratio, rel)
    assert recs["floor"][0] == floor
    assert hit[0, 0] and not hit[0, 1] and not hit[0, 4]
    assert hit[0, 2] == ((floor * ratio + 1) * rel >= top)
    assert hit[0, 3] == (-(-top // rel) > floor * ratio) and (rel == 1 or hit[0, 3])
    # the floor test alone decides where the top is low: bins 0 and 2 are the strongest, and equal (>= holds at rel = 1)
    p[0, 0] = floor * ratio + 1
    p[0, 3] = p[0, 4] = 0
    recs, hit = assert_equals_direct(s, p, nf, ratio, rel)
    assert hit[0, 0] and hit[0, 2] and not hit[0, 1] and recs["n_hit"][0] == 2
    for bad in ((1, 16), (4097, 16), (32, 0), (32, 4097)):
        with pytest.raises(ValueError):
            occupancy.occupancy(s, p, nf, *bad)


def test_noise_alone_hits_nothing_at_the_defaults():
    rng = np.random.default_rng(3)
    row = np.clip(np.rint(128 + rng.normal(0, 20, 2 * 256 * 200)), 0, 255).astype(np.uint8)
    s, p, nf = spectrum.spectrum(row, 256, 50, fmt="u8")
    recs, bits = occupancy.occupancy(s, p, nf)
    assert len(recs) == 4 and (recs["floor"] > 1000).all() and recs["n_hit"].sum() == 0 and not bits.any()


@functools.lru_cache(maxsize=None)
def scan_hits(n_bins, g):
    s, p, nf = spectrum.spectrum(scan_file(), n_bins, g, fmt="u8")
    recs, bits = occupancy.occupancy(s, p, nf)
    return occupancy.unpack(bits, n_bins).sum(axis=0), len(nf)


@pytest.mark.parametrize("n_bins,g,lo,hi", [(256, 170, 70, 80), (1024, 42, 282, 318)])
def test_the_scan_file_holds_one_channel(n_bins, g, lo, hi):
    hits, records = scan_hits(n_bins, g)
    assert records == 4
    ch = occupancy.channels(hits, records, n_bins, 2048000, 868250)
    assert ch == [{"kind": "found", "khz": 868850, "lo": lo, "hi": hi, "hits": 1, "in_range": True}]


def found(ch):
    return [(c["lo"], c["hi"]) for c in ch if c["kind"] == "found"]


def test_channels_join_rule_at_the_limit():
    n, fs = 256, 2048000  # a bin is 8000 Hz: a gap of 6 empty bins is 48000 Hz, of 7 is 56000 Hz
    hits = [0] * n
    hits[10] = hits[17] = 1  # 6 empty bins between them
    assert found(occupancy.channels(hits, 10, n, fs, 868250, join_hz=48000)) == [(10, 17)]   # gap = limit
    assert found(occupancy.channels(hits, 10, n, fs, 868250, join_hz=47999)) == [(10, 10), (17, 17)]  # limit + 1 Hz short
    hits[17], hits[18] = 0, 1  # 7 empty bins
    assert found(occupancy.channels(hits, 10, n, fs, 868250, join_hz=48000)) == [(10, 10), (18, 18)]
    assert found(occupancy.channels(hits, 10, n, fs, 868250, join_hz=56000)) == [(10, 18)]
    assert found(occupancy.channels(hits, 10, n, fs, 868250, join_hz=0)) == [(10, 10), (18, 18)]
    hits[11] = 3
    ch = occupancy.channels(hits, 10, n, fs, 868250, join_hz=0)  # adjacent bins join at any limit; the group's hits are its largest
    assert found(ch) == [(10, 11), (18, 18)] and ch[0]["hits"] == 3
    # the offset: floor(((lo + hi) fs + 1000 N) / (2000 N)) -- the middle of bins 10 and 11 is 84000 Hz
    assert ch[0]["khz"] == 868250 + 84 and ch[1]["khz"] == 868250 + 144


def test_channels_carrier_rule_and_the_edges_of_the_band():
    n, fs = 256, 2048000
    hits = [0] * n
    hits[0] = 5    # 2 * 5 = 10 = records: not a carrier
    hits[3] = 6    # 2 * 6 = records + 2 > records: a carrier (with 11 records below: 2 * 6 = records + 1)
    hits[127] = 1  # the highest bin, +1016 kHz
    hits[128] = 1  # bin -N/2, -1024 kHz: no wrap-around -- 127 and -128 are neighbours on the circle only
    hits[255] = 2  # bin -1
    ch = occupancy.channels(hits, 10, n, fs, 868250)
    assert [c["kind"] for c in ch] == ["found", "found", "carrier", "found"]
    assert found(ch) == [(-128, -128), (-1, 0), (127, 127)]
    assert ch[0]["khz"] == 868250 - 1024 and not ch[0]["in_range"] and not ch[3]["in_range"] and ch[1]["in_range"]
    assert ch[1]["hits"] == 5 and ch[1]["khz"] == 868250 - 4  # floor((-1 * 2048000 + 256000) / 512000) = floor(-3.5): floor, not truncation
    assert ch[2] == {"kind": "carrier", "khz": 868250 + 24, "bin": 3, "hits": 6}
    assert occupancy.channels(hits, 11, n, fs, 868250)[2]["kind"] == "carrier"   # 2 * 6 = records + 1
    ch12 = occupancy.channels(hits, 12, n, fs, 868250)                            # 2 * 6 = records: active, and it joins 0
    assert [c["kind"] for c in ch12] == ["found"] * 3 and found(ch12) == [(-128, -128), (-1, 3), (127, 127)]
    # a carrier between two active bins is no part of the group but does not cut it either: the gap counts bins, not what they hold
    hits = [0] * n
    hits[20], hits[21], hits[22] = 1, 9, 1
    ch = occupancy.channels(hits, 10, n, fs, 868250)
    assert [(c["kind"], c["khz"]) for c in ch] == [("found", 868250 + 168), ("carrier", 868250 + 168)] and found(ch) == [(20, 22)]
    # the scan's own range: |off| * 1000 <= fs / 2 - 192000 = 832000
    for b, ok in ((104, True), (105, False), (-104, True), (-105, False)):  # 104 bins = 832000 Hz
        hits = [0] * n
        hits[b % n] = 1
        (c,) = occupancy.channels(hits, 10, n, fs, 868250)
        assert c["khz"] == 868250 + 8 * b and c["in_range"] == ok, b


def test_the_library_exports_the_two_symbols():
    assert "tfrec_amd_enable_occupancy" in api.EXPORTS and "tfrec_amd_read_occupancy" in api.EXPORTS
    L = api.load_library()
    assert L.tfrec_amd_enable_occupancy is not None and L.tfrec_amd_read_occupancy is not None
    assert L.tfrec_amd_enable_occupancy(None, 32, 16) == api.E_INVAL
    assert L.tfrec_amd_read_occupancy(None, 0, None, None, 0, None) == api.E_INVAL


# ---- tfrec_gpu -A: what is decided before a device is opened
@pytest.fixture(scope="module")
def cli():
    return parity.build_cli()


def test_cli_usage_errors(cli, tmp_path):
    f = str(tmp_path / "missing.iq")
    for extra in (["-s", "50"], ["-n", "2"], ["-p", "t=100"], ["-f", "868300"], ["-e", "true"], ["-E", "true"], ["-X", f], ["-S", "x"],
                  ["-L", f], ["-d", "0,1"]):
        out = parity.run_cli(["-A", "-L", f] + extra)
        assert out.returncode == 1 and "-A finds and scans the channels of one -L file" in out.stderr, extra
    for bad in ("1", "4097", "32,0", "32,4097", "32,16,100001", "32,16,5,1", "32,", "32,x", "32;16", "0"):
        for args in (["-A", bad], ["-A" + bad]):
            out = parity.run_cli(args + ["-L", f])
            assert out.returncode == 1 and "bad -A" in out.stderr, args
    for args in (["-A"], ["-A", "2"], ["-A4096,4096,0"], ["-A", "32,16,100000", "-x"], ["-A", "-P", "1024", "-r", "2400000", "-F", "s16"],
                 ["-c", "433920", "-A", "64,1"]):
        out = parity.run_cli(args + ["-L", f])  # accepted: the file is looked for
        assert out.returncode == 2 and "missing.iq" in out.stderr, args
    out = parity.run_cli(["-A"])
    assert out.returncode == 1 and "need -L" in out.stderr


def test_cli_a_bad_argument_is_echoed(cli, tmp_path):
    """The diagnostic names the argument as it was given, attached to -A or as the next word."""
    f = str(tmp_path / "missing.iq")
    for bad in ("1", "32,16,5,1", "32,", "4097,2"):
        for args in (["-A", bad], ["-A" + bad]):
            out = parity.run_cli(args + ["-L", f])
            assert out.returncode == 1 and out.stderr.startswith("tfrec_gpu: bad -A '%s': want [ratio[,rel[,join_kHz]]]" % bad), (args, out.stderr)


@pytest.mark.parametrize("args,fs_in,n_bins,g,occ", [
    (["-r", "2048000", "-c", "868250", "-A"], 2048000, 256, 170, (32, 16, 50000)),
    (["-c", "868250", "-A", "64,8,25"], 1536000, 256, 128, (64, 8, 25000)),
    (["-x", "-c", "868250", "-P", "1024", "-A40"], 15360000, 1024, 320, (40, 16, 50000)),
    (["-r", "2048000", "-c", "433920", "-A", "-P", "1024,42"], 2048000, 1024, 42, (32, 16, 50000)),
])
def test_cli_bin_list(cli, tmp_path, args, fs_in, n_bins, g, occ):
    """The bins of pass 1 in ascending frequency and its parameters, listed before a device is opened (an empty file: no record, no
    channel, no scan -- where a device can be opened at all)."""
    f = tmp_path / "empty.iq"
    f.write_bytes(b"")
    out = parity.run_cli(args + ["-L", str(f)])
    assert out.returncode in (0, 2)
    c = int(args[args.index("-c") + 1])
    assert "spec: %d bins, %d frames per record, input rate %d S/s" % (n_bins, g, fs_in) in out.stderr
    assert "occ: ratio %d, rel %d, join %d Hz" % occ in out.stderr
    got = re.findall(r"^spec bin (\S+) kHz$", out.stderr, re.M)
    khz = spectrum.bin_khz(c, fs_in, n_bins)
    assert got == ["%.3f" % khz[(i + n_bins // 2) % n_bins] for i in range(n_bins)]
    assert not re.search(r"^(found|carrier|scan) ", out.stdout, re.M)
