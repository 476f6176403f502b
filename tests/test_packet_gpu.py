"""The packet check on the GPU (tfrec_amd_enable_burst_packets, tfrec_amd_read_burst_packets), bit for bit: the records
and the ok bitmap's words against the restatement tfrec_amd/packet.py run on the context's OWN track and sync records and words of
the same submit.  tests/packet_rows.py says what each planted row is there for, and tests/test_packet_cpu.py that the restatement
alone reports exactly the planted packets.  Everything is an exact integer; nothing here has a tolerance."""
import numpy as np
import pytest

import packet_rows as PR
import parity
import recorder as R
from recorder import cli_lines, hand_receiver, raises, same_records, same_words
from tfrec_amd import api, linecode, packet

pytestmark = pytest.mark.gpu
B = PR.B
LAYOUTS = {"one": lambda nb: (nb,), "blocks": lambda nb: (1,) * nb}


def run(st, rows, sizes, code=None, resets=None):
    """The rows in submits of `sizes` blocks, all queued before the first read (unless a reset comes between them); every submit's
    packet records and words compared -> the merged chains, by stream.  code: the line code ahead of the sync; resets: {submit:
    the streams reset ahead of it}."""
    n, sst = len(rows), PR.sync_settings(st)
    subs, pos = [], 0
    with hand_receiver(n, max(sizes), (), cap=(32 * n, n * max(sizes) * B)) as r:
        r.enable_burst_track(PR.L)
        r.enable_burst_sync(sst.rate, sst.pattern, sst.P, sst.E, sst.both)
        r.enable_burst_packets(**st.args())
        if code is not None:  # (behind the packet check's enable: the input is chosen per submit)
            r.enable_burst_code(code.rate, code.taps, code.invert)
        r.set_burst_track_centre(range(n), [0] * n)
        parts = []
        for nb in sizes:
            parts.append(np.ascontiguousarray(rows[:, pos * B:(pos + nb) * B]))
            pos += nb
        if not resets:
            for x in parts:
                r.submit(x)
        state = sstate = None
        for i, x in enumerate(parts):
            if resets:
                if i in resets:
                    r.reset_streams(resets[i])
                r.submit(x)
            r.read_captures()
            trecs, twords = r.read_burst_codes() if code is not None else r.read_burst_tracks()
            srecs, swords, sstate = R.read_sync(r, sst, sstate, trecs, twords)
            got, words = r.read_burst_packets()
            assert got.dtype == packet.PACKET_DTYPE and r.packet_total == (r.code_total if code is not None else r.track_total)
            want, wwords, state = packet.packets(trecs, twords, srecs, swords, st, state, n, max_samples=r._capture[1])
            same_records(got, want, "packet")
            same_words(words, wwords, "packet")
            subs.append((got, words))
            r.drain()
    return {int(c["stream"]): c for c in packet.chains(subs)}


def found(st, rows, want, sizes, **kw):
    """... and the planted packets are what the GPU reports: an ok plateau where one is planted, nothing where none is."""
    ch = run(st, rows, sizes, **kw)
    for s, data in enumerate(want):
        assert (int(ch[s]["n_ok"]) > 0) == (data is not None) and int(ch[s]["n_ok"]) == int(ch[s].bits.sum()), (s, ch[s].rec)
    return ch


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("kind", ["across", "end"])
@pytest.mark.parametrize("name", list(PR.SETS))
def test_every_settings_row_in_one_submit_and_in_one_block_submits(name, kind, layout):
    st, rows, want = PR.case(name, kind)
    found(st, rows, want, LAYOUTS[layout](rows.shape[1] // B))


@pytest.mark.parametrize("name,arg", [("cc1101", v) for v in (0, 1, 62, 63, 64, 65, 127, 128)] + [("plain", v) for v in (1, 20, 21)])
def test_lengths_on_both_sides_of_a_wave_and_of_the_admitted_range(name, arg):
    st, rows, want = PR.case(name, "length", arg)
    ch = found(st, rows, want, (3,))
    assert want[0] is not None or int(ch[0]["n_seen"]) == 0  # len_max + 1 is dropped and not counted


@pytest.mark.parametrize("kind,arg", [("cut", None), ("flip", 3), ("flip", 20), ("flip", 85)])
def test_a_packet_cut_off_by_the_bursts_end_and_flipped_bits_in_the_length_the_payload_and_the_field(kind, arg):
    st, rows, want = PR.case("cc1101", kind, arg)
    ch = found(st, rows, want, (2,))
    assert (int(ch[0]["n_seen"]) == 0) == (kind == "cut" or arg == 3)


@pytest.mark.parametrize("n", [3, 65])
def test_streams_with_different_plants_in_one_context(n):
    st, rows, want = PR.case("cc1101", "three")
    ch = found(st, np.ascontiguousarray(rows[np.arange(n) % 3]), [want[s % 3] for s in range(n)], (1, 1))
    assert all(ch[s].bits.tobytes() == ch[s % 3].bits.tobytes() for s in range(n))


def test_the_line_code_ahead_of_the_sync_is_the_input():
    """The "whole" packet sent NRZI-precoded: only the coded track carries the word and the packet."""
    st = PR.settings("cc1101")
    sym, data = PR.symbols(st, 9, 1)
    rows = PR.row(2, 77, st, [(300, np.bitwise_xor.accumulate(sym).tolist())])[None]
    found(st, rows, [data], (2,), code=linecode.nrzi(st.rate))


def test_a_reset_between_the_sync_word_and_the_length_byte_drops_the_packet():
    st, rows, want = PR.case("cc1101", "across")
    ch = run(st, rows, (1, 1), resets={1: [0]})
    assert ch and all(int(c["n_ok"]) == 0 for c in ch.values())  # the run behind the reset does not CONTINUE


def test_cli_packet_and_pkts_lines_of_three_recordings_read_a_block_a_batch(tmp_path):
    parity.build_cli()
    xs, wants = PR.cli_scene()
    files = [str(tmp_path / ("p%d.iq" % i)) for i in range(3)]
    for f, x in zip(files, xs):
        x.tofile(f)
    kinds = ("bits", "frame", "packet", "pkts")
    got = cli_lines(PR.CLI_ARGS + ["-T", "2f", "-t", "500", "-b", "1"] + sum((["-L", f] for f in files), []), kinds)[kinds]
    for f, want in zip(files, wants):
        assert [ln for ln in got if ln.split()[1] == f] == [ln % f for ln in want]
    verdicts = [ln.split()[5] for ln in got if ln.startswith("packet ")]
    assert sorted(verdicts) == ["bad", "ok", "ok"] and len([ln for ln in got if ln.startswith("pkts ")]) == 3


def test_the_refusals_and_the_memory():
    st, sst = PR.settings("cc1101"), PR.sync_settings(PR.settings("cc1101"))
    with hand_receiver(2, 1, (), cap=(64, 2 * B)) as r:
        r.enable_burst_track(PR.L)
        raises(api.E_INVAL, r.enable_burst_packets, **st.args())  # no sync
        raises(api.E_INVAL, r.read_burst_packets)
        r.enable_burst_sync(sst.rate, sst.pattern, sst.P, sst.E, False)
        m = r.memory()
        for bad in (dict(rate=17240), dict(len_min=161), dict(skip=1), dict(len_max=203), dict(len_add=17), dict(width=12), dict(poly=0),
                    dict(whiten=bytes(275))):
            raises(api.E_INVAL, r.enable_burst_packets, **{**st.args(), **bad})
        assert r.memory() == m  # nothing was allocated
        r.enable_burst_packets(**st.args())
        assert r.memory()["device_bytes"] - m["device_bytes"] == packet.device_bytes(2, 64, 2 * B)
        assert r.memory()["pinned_host_bytes"] == m["pinned_host_bytes"]
        raises(api.E_INVAL, r.enable_burst_packets, **st.args())  # a second call
    with hand_receiver(1, 1, (), cap=(64, B)) as r:
        r.enable_burst_track(PR.L)
        r.enable_burst_sync(sst.rate, sst.pattern, sst.P, sst.E, True)
        raises(api.E_INVAL, r.enable_burst_packets, **st.args())  # the sync's BOTH
