"""The packet check without a GPU (tfrec_amd/packet.py, tests/packet_rows.py): the whitening sequence, the settings'
refusals, and what the restatement alone reports on the planted rows the GPU tests run -- exactly the planted packets."""
import ctypes
import re

import pytest

import packet_rows as PR
import parity
from tfrec_amd import api, packet, sync

GOOD = dict(rate=38400, len_max=60, width=16, poly=0x8005)
ROWS = [(n, k, None) for n in PR.SETS for k in ("whole", "across", "end", "cut")] + [("cc1101", "length", v) for v in (0, 1, 62, 63, 64, 65, 127, 128)] + \
       [("plain", "length", v) for v in (1, 20, 21)] + [("cc1101", "flip", v) for v in (3, 20, 8 * 10 + 5)]


def test_pn9_is_the_cc1101_sequence():
    assert packet.pn9(20).hex() == "ffe11d9aed853324ea7ad2397097570a547d2dd8"


@pytest.mark.parametrize("bad", [dict(sync=None), dict(sync=sync.Settings(17240, PR.WORD, 16)), dict(sync=sync.Settings(38400, PR.WORD, 16, 0, True)),
                                 dict(len_min=61), dict(skip=1), dict(len_max=203), dict(len_add=17), dict(width=12), dict(poly=0),
                                 dict(whiten=bytes(275))])
def test_settings_refusals(bad):
    packet.Settings(**GOOD, sync=sync.Settings(38400, PR.WORD, 16))
    with pytest.raises(ValueError):
        packet.Settings(**{**GOOD, **bad})


def test_the_largest_reach_is_admitted_and_one_more_sample_is_not():
    assert PR.settings("reach").reach == 16381 and packet.Settings(38400, 201, 16, 0x8005).reach == 16320
    with pytest.raises(ValueError):
        packet.Settings(**{**PR.SETS["reach"], "rate": 6000})


@pytest.mark.parametrize("name,kind,arg", ROWS)
def test_the_restatement_alone_reports_exactly_the_planted_packet(name, kind, arg):
    st, rows, want = PR.case(name, kind, arg)
    nb = rows.shape[1] // PR.B
    whole, cut = PR.restated(st, rows, (nb,))[0], PR.restated(st, rows, (1,) * nb)[0]
    v, w = packet.chains(whole[2]), packet.chains(cut[2])
    assert len(v) == len(w) == 1 and v[0].rec.tobytes() == w[0].rec.tobytes() and (v[0].bits == w[0].bits).all()  # the cut does not matter
    v, s = v[0], sync.chains(whole[1])[0]
    (a, b), = sync.plateaus(s.bits)  # the planted word's matches, and no other
    if want[0] is None:
        assert int(v["n_ok"]) == 0 and int(v["first_at"]) == packet.NONE and not v.bits.any()
        if kind in ("cut", "length") or arg == 3:  # cut off, too long, or a length byte that names an end behind the burst
            assert int(v["n_seen"]) == 0
        else:
            assert 1 <= int(v["n_seen"]) <= b - a + 1
        return
    (ka, kb), = sync.plateaus(v.bits)  # one ok plateau ...
    k = (a + b) // 2 + packet.delta(st.rate, 8 * len(want[0]))
    assert ka <= k <= kb and int(v["n_ok"]) == kb - ka + 1 and int(v["first_at"]) == ka and int(v["n_seen"]) == b - a + 1  # ... that holds c + delta(8 T)
    item = [x for x in packet.read(sync.track.chains(whole[0])[0], s, v, st)]
    assert item == [((a + b) // 2, want[0][0], "ok", want[0])]
    if kind == "end":
        start = int(v["start_sample"])
        assert ka + start <= PR.B - 1 and kb + start >= PR.B  # an end on the block's last sample and one on the next block's first
    if kind == "across":
        pieces = [int(r["n_ok"]) for recs, _ in cut[2] for r in recs]
        assert len(pieces) == nb and pieces[0] == 0 and sum(pieces[1:]) == int(v["n_ok"])  # the word in the first piece, the end in a later one
        assert a + int(v["start_sample"]) < PR.B <= (a + b) // 2 + int(v["start_sample"]) + packet.delta(st.rate, 8)


def test_the_c_abi_exports_the_packet_check_and_its_record_has_48_bytes():
    lib = ctypes.CDLL(api.load_library()._name)
    assert lib.tfrec_amd_enable_burst_packets and lib.tfrec_amd_read_burst_packets
    text = open(parity.ROOT + "/include/tfrec_amd.h").read()
    body = re.search(r"typedef struct \{[^}]*\} tfrec_amd_burst_packet;", text).group(0)
    size = {"uint32_t": 4, "int32_t": 4, "int64_t": 8, "uint64_t": 8}
    assert sum(size[t] for t in re.findall(r"^\s*(u?int\d+_t)\s", body, re.M)) == 48 == packet.PACKET_DTYPE.itemsize


def test_cli_packet_usage_errors_and_accepted_forms(tmp_path):
    parity.build_cli()
    f = str(tmp_path / "missing.iq")
    base = ["-G", "38400", "-Y", "2dd4,0,8", "-V", "16,8005,ffff"]
    for args, text in ((base[:4] + ["-N", "60"], "-N checks the packets"), (["-N", "60", "-V", "16,8005"], "-V checks the frames"),
                       (base + ["-N", "x"], "bad -N"), (base + ["-N", "60,0,0,abc"], "bad -N"), (base + ["-N", "203"], "-N: "),
                       (base + ["-N", "60,61"], "-N: "), (base[:2] + ["-Y", "2dd4,0,8,1"] + base[4:] + ["-N", "60"], "both"),
                       (base + ["-N", "60", "-s", "50"], "-G reads the bursts")):
        out = parity.run_cli(args + ["-L", f])
        assert out.returncode == 1 and text in out.stderr, (args, out.stderr)
    for form in ("60", "201,1", "60,0,2", "160,0,0,pn9", "60,0,0,ff00aa"):
        out = parity.run_cli(base + ["-N", form, "-L", f])  # accepted: the file is looked for
        assert out.returncode == 2 and "missing.iq" in out.stderr, (form, out.stderr)
