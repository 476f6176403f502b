"""CPU tests of the `frames` and `splices` families (oracle/scenes.py): every class of carried decoder state the rows claim is
measured back from the oracle -- FRAMES_CLASSES and SPLICES_CLASSES name them, frames_classes() / splices_classes() return what
a batch reaches --, and where a class says that a telegram DEPENDS on carried state, the counterfactual is shown too: the
bit log replayed through a Python store_bit with the shift register cleared by every flush, the stale bytes zeroed, a fresh
oracle on the part behind a submit cut."""
import functools

import numpy as np
import pytest

from oracle import oracle as O
from oracle import scenes as S
from tfrec_amd import synth

TYPES = 0x2F
TYPE_BIT = (0, 1, 2, 3, 5)   # slot -> its bit in the types mask
NAMES = tuple(n.lower() for n in synth.PROTO_NAMES)
B2 = 2 * 32768               # bytes per block


def run(iq, types=TYPES):
    o = O.Oracle(types, S.THRESH, 0, log_bits=True)
    o.process(iq)
    return o


@functools.lru_cache(maxsize=None)
def results(fam):
    """[(row, its bytes, its oracle)] of a family."""
    out = []
    for row in S.family(fam):
        iq = S.render(row)
        iq.setflags(write=False)
        out.append((row, iq, run(iq)))
    return out


def row_of(fam, name):
    return next(r for r in results(fam) if r[0]["name"] == name)


def flushes(o, slot):
    """The slot's flushes that held bytes, as events_full tuples."""
    return [e for e in o.events_full() if e[0] == slot and e[2] > 0]


def records(o, slot):
    """The slot's records of the bit log, one string of bits per flush."""
    return [(ln.split() + [""])[3] for ln in o.bits_text().splitlines() if int(ln.split()[1]) == slot]


# ---- the decoders' store_bit, restated
def tfa1_replay(recs, zero_sr=False):
    """tfa1_decoder::store_bit (tfa1.cpp:120-134) and what flush re-arms, over the bit log's records -> per flush (byte_cnt, the
    bit of the record at which a sync word completed last, or None).  zero_sr: the shift register cleared by every flush --
    which the decoder does not do."""
    sr, out = 0, []
    for bits in recs:
        sr_cnt, byte_cnt, sync_at = -1, 0, None
        for i, ch in enumerate(bits):
            sr = (sr >> 1) | (int(ch) << 31)
            if sr & 0xffff == 0xd42d:
                sr_cnt, byte_cnt, sync_at = 0, 0, i
            if sr_cnt == 0:
                byte_cnt += 1
            if sr_cnt >= 0:
                sr_cnt = (sr_cnt + 1) & 7
        out.append((byte_cnt, sync_at))
        if zero_sr:
            sr = 0
    return out


def whb_replay(recs, zero_lfsr_at=()):
    """whb_decoder::store_bit (whb.cpp:566-603) over the bit log's records -> per flush (byte_cnt, the bit at which the sync word
    completed last, or None).  zero_lfsr_at: (record, bit) positions ahead of which the descrambler is cleared."""
    last_bit = psk = last_psk = nrzs = lfsr = sr = 0
    out = []
    for k, bits in enumerate(recs):
        sr_cnt, byte_cnt, sync_at = -1, 0, None
        for i, ch in enumerate(bits):
            if (k, i) in zero_lfsr_at:
                lfsr = 0
            bit = int(ch)
            if bit == last_bit:
                psk = 1 - psk
            if psk == last_psk:
                nrzs = 1 - nrzs
            last_bit, last_psk = bit, psk
            o = nrzs ^ ((lfsr >> 16) & 1) ^ ((lfsr >> 11) & 1)
            lfsr = ((lfsr << 1) | nrzs) & 0xffffffff
            sr = (sr >> 1) | (o << 31)
            if sr == 0x2bd42d4b:
                sr_cnt, byte_cnt, sync_at = 0, 3, i
            if sr_cnt == 0:
                byte_cnt += 1
            if sr_cnt >= 0:
                sr_cnt = (sr_cnt + 1) & 7
        out.append((byte_cnt, sync_at))
        sr = 0  # whb_decoder::flush
    return out


def test_the_restated_store_bits_count_the_oracles_bytes():
    """The two replays against every TFA_1 and WHB flush of both families: the byte counts the oracle reported."""
    n = 0
    for fam in ("frames", "splices"):
        for row, _, o in results(fam):
            for slot, replay in ((0, tfa1_replay), (4, whb_replay)):
                want = [e[2] for e in o.events_full() if e[0] == slot]
                assert [b for b, _ in replay(records(o, slot))] == want, (row["name"], slot)
                n += len(want)
    assert n > 40


# ---- frames
def _labels_frames():
    out = []
    for p in (1, 2, 3):
        out += ["%s:%s" % (k, NAMES[p]) for k in ("inverted", "plain_inverted_plain_one_window", "plain_inverted_plain_split", "iq_swap")]
    out += ["tx22_byte_cnt_%d" % n for n in (6, 7, 63, 64)] + ["tx22_num_0", "tx22_num_7", "tx22_nibble"]
    out += ["tx22_stale_accept", "tx22_stale_reject", "tx22_stale_over"]
    out += ["whb_byte_cnt_%d" % n for n in (10, 11, 60, 61)] + ["whb_plen_%d" % n for n in (0, 3, 4, 60, 61)]
    out += ["whb_unknown_type", "whb_stale_accept", "whb_stale_reject"]
    out += ["tfa1_byte_cnt_%d" % n for n in (9, 10, 11)] + ["tfa1_rdata10_cleared"]
    out += ["byte_cnt_over_%d:%s" % (n, NAMES[p]) for p in (0, 1) for n in (64, 256)]
    return tuple(out)


FRAMES_CLASSES = _labels_frames()


def _telegrams_with_polarity(o, slot):
    """Per accepted telegram of the slot, in order: whether `Inverted SYNC` was printed since the slot's telegram before it.
    (Every chain of the TFA_2 family prints the line: only its presence is read.)"""
    from parity import PREFIX
    out, inv = [], False
    for ln in o.text().splitlines():
        if ln == "Inverted SYNC":
            inv = True
        elif ln.startswith(PREFIX[slot]):
            out.append(inv)
            inv = False
        elif ln.startswith(tuple(PREFIX.values())):
            inv = False
    return out


def frames_classes(batch):
    """batch: [(row, bytes, oracle)] -> the labels of FRAMES_CLASSES it reaches, measured on the oracle's events and text alone
    (the rows' names are not read)."""
    hit = set()
    for row, _, o in batch:
        swapped = bool(row.get("iq_swap"))
        for p in (1, 2, 3):
            fl, pol = flushes(o, p), _telegrams_with_polarity(o, p)
            ok = [e for e in fl if e[7] == 1]
            if swapped and len(pol) >= 2 and all(pol):
                hit.add("iq_swap:" + NAMES[p])
            if not swapped and pol == [True] and len(ok) == 1 and len(row["bursts"]) == 1:
                hit.add("inverted:" + NAMES[p])
            if not swapped and pol == [False, True, False]:
                hit.add("plain_inverted_plain_split:" + NAMES[p])
            if not swapped and len(row["bursts"]) == 3 and len(fl) == 1 and len(ok) == 1 and "Inverted SYNC" in o.text():
                # one flush over three frames, the middle one's sync found complemented, the last one's plain again
                if bytes(ok[0][5])[:len(row["bursts"][2]["frame"]) // 2].hex() == row["bursts"][2]["frame"]:
                    hit.add("plain_inverted_plain_one_window:" + NAMES[p])
        tx = flushes(o, 3)
        for k, e in enumerate(tx):
            n, st, r = e[2], e[7], bytes(e[5])
            num = r[3] & 7
            if (n, st) in ((6, 0), (64, 0)) or (n == 7 and st != 0) or (n == 63 and st == 1):
                hit.add("tx22_byte_cnt_%d" % n)
            if st == 1 and num in (0, 7) and n >= 2 * num + 5:
                hit.add("tx22_num_%d" % num)
            if st == 2 and r[2] >> 4 != 0xa and r[2 * num + 4] == S.crc8(r[2:4 + 2 * num]) and n >= 2 * num + 5:
                hit.add("tx22_nibble")
            if 7 <= n < 2 * num + 5 and r[2] >> 4 == 0xa and k > 0:  # the checksum and bytes under it are not this flush's own
                if k == 1 and tx[0][2] >= 2 * num + 5:
                    hit.add("tx22_stale_accept" if st == 1 else "tx22_stale_reject")
                if k == 2 and st == 1 and n < tx[1][2] < 2 * num + 5 <= tx[0][2]:  # two earlier flushes share the stale stretch
                    hit.add("tx22_stale_over")
        for e in flushes(o, 4):
            n, st, r = e[2], e[7], bytes(e[5])
            if (n, st) in ((10, 0), (61, 0)) or (n == 11 and st != 0) or (n == 60 and st == 1):
                hit.add("whb_byte_cnt_%d" % n)
            if 11 <= n <= 60:
                if r[4] in (0, 3, 4, 60, 61) and r[5] in S.WHB_INIT and st == 2:
                    hit.add("whb_plen_%d" % r[4])
                if r[5] == 0x05 and st == 2 and "unsupported sensor type 05" in o.text():
                    hit.add("whb_unknown_type")
                if 11 < r[4] <= 60 and r[4] + 4 > n and r[5] in S.WHB_INIT and len(flushes(o, 4)) == 2:  # the CRC lies behind its own bytes
                    hit.add("whb_stale_accept" if st == 1 else "whb_stale_reject")
        fl = flushes(o, 0)
        for k, e in enumerate(fl):
            n, st, r = e[2], e[7], bytes(e[5])
            if (n == 9 and st == 0) or (n in (10, 11) and st != 0):
                hit.add("tfa1_byte_cnt_%d" % n)
            if n == 10 and k > 0:
                before = bytes(fl[k - 1][5])
                if before[10] != 0 and before[11] != 0 and r[10] == 0 and r[11] == before[11] and fl[k - 1][2] > 11:
                    hit.add("tfa1_rdata10_cleared")
        for p in (0, 1):
            for e in flushes(o, p):
                for n in (64, 256):
                    if e[2] > n:
                        hit.add("byte_cnt_over_%d:%s" % (n, NAMES[p]))
    return hit


def test_frames_rows_are_8_blocks_of_integers():
    for fam in ("frames", "splices"):
        for row, iq, _ in results(fam):
            assert 4 <= row["n_blocks"] <= 8 and iq.size == row["n_blocks"] * B2 and iq.dtype == np.uint8, row["name"]


@pytest.mark.parametrize("label", FRAMES_CLASSES)
def test_frames_reach_every_class(label):
    assert label in frames_classes(results("frames"))


def test_frames_classes_are_not_reached_by_an_ordinary_family():
    """The labels are measurements, not names: the repeats family reaches none of the stale, length or polarity classes."""
    batch = [(row, None, run(S.render(row))) for row in S.family("repeats")[:10]]
    assert not frames_classes(batch)


def _verdict_of_bytes(slot, stale, own):
    """The slot's decoder's verdict on the bytes `own` with `stale` (or nothing) left behind by a flush before: -X's
    store_bytes + flush on a decoder of its own."""
    o = O.Oracle(1 << TYPE_BIT[slot], S.THRESH, 0)
    if stale is not None:
        o.hex(stale)
    o.hex(own)
    return o.events_full()[-1][7]


@pytest.mark.parametrize("name,slot", [("tx22_stale_accept", 3), ("tx22_stale_over", 3), ("whb_stale_accept", 4)])
def test_a_stale_acceptance_flips_when_the_earlier_bytes_are_zeroed(name, slot):
    row, iq, o = row_of("frames", name)
    fl = flushes(o, slot)
    b, before = fl[-1], fl[-2]
    assert b[7] == 1
    own = bytes(b[5])[:b[2]]
    # the flush before left all 64 bytes of its event behind (and TFA_1 alone clears one of them)
    assert _verdict_of_bytes(slot, bytes(before[5]), own) == 1, "the restated verdict is not the row's"
    assert _verdict_of_bytes(slot, None, own) == 2, "B is accepted on its own bytes"
    # the same on the signal: without the frames ahead of it B is rejected
    alone = dict(row, bursts=row["bursts"][-1:])
    last = flushes(run(S.render(alone)), slot)
    assert len(last) == 1 and last[0][2] == b[2] and last[0][7] == 2


def test_the_rejecting_twins_differ_in_one_stale_bit():
    for acc, rej, slot in (("tx22_stale_accept", "tx22_stale_reject", 3), ("whb_stale_accept", "whb_stale_reject", 4)):
        a, r = flushes(row_of("frames", acc)[2], slot)[-1], flushes(row_of("frames", rej)[2], slot)[-1]
        diff = [i for i in range(64) if a[5][i] != r[5][i]]
        read = 19 if slot == 3 else a[5][4] + 4   # the bytes the verdict reads: up to the checksum's last
        seen = [i for i in diff if i < read]
        assert all(i >= a[2] for i in diff) and len(seen) == 1 and bin(a[5][seen[0]] ^ r[5][seen[0]]).count("1") == 1
        assert (a[7], r[7]) == (1, 2) and a[1:5] == r[1:5]


# ---- where the GPU tests cut the submits (S.carried_cut_claims, asserted again there before the GPU is used)
def test_submit_cuts_fall_where_the_state_is_carried():
    claims = S.carried_cut_claims("frames") + S.carried_cut_claims("splices")
    for name, cut, lo, hi in claims:
        assert lo < cut < hi and cut in S.carried_boundaries(), name
    names = {c[0] for c in claims}
    assert {r["name"] for r in S.family("frames") if r["name"].startswith("pol_") or "_stale_" in r["name"]} <= names
    assert len([n for n in names if n.startswith("tfa1_split")]) == 6 and "whb_cut_preamble_submit_cut" in names
    # the TFA_1 splice rows without a claim lie in one submit altogether (the WHB burst is longer than two blocks: its second
    # window lies across the second cut, and in one submit only when the whole row is one)
    for row in S.family("splices"):
        if row["name"] not in names:
            assert S.splice_parts(row)[1] + 16000 < S.CUT_A or row["name"].startswith("whb"), row["name"]


@pytest.mark.parametrize("fam", ["frames", "splices"])
def test_a_fresh_receiver_behind_the_submit_cut_loses_the_telegram(fam):
    """open_at_the_cut's argument for every row with a claim: the whole row decodes a telegram behind the cut that a fresh oracle
    on the part behind the cut does not produce."""
    n = 0
    for name, cut, lo, hi in S.carried_cut_claims(fam):
        row, iq, o = row_of(fam, name)
        if name.endswith("_reject"):
            continue
        slot = row["base"]["bursts"][0]["proto"] if row["kind"] == "splice" else row["bursts"][-1]["proto"]
        tel = [e for e in o.events_full() if e[0] == slot and e[7] == 1 and e[1] > cut // 4]
        assert tel, name
        tail = run(iq[2 * cut:])
        assert not [e for e in tail.events_full() if e[0] == slot and e[7] == 1 and e[5] == tel[0][5]], name
        n += 1
    assert n >= (6 if fam == "splices" else 14)


# ---- splices
SPLICES_CLASSES = ("tfa1_split_one_submit", "tfa1_split_window0_of_next_submit", "tfa1_split_open_at_submit_cut",
                   "tfa1_split_one_empty_window", "tfa1_split_two_empty_windows", "tfa1_split_empty_window_behind_submit_cut",
                   "tfa1_split_three_ways_one_submit", "tfa1_split_three_ways_window0_of_next_submit",
                   "tfa1_split_at_5_points", "whb_cut_in_preamble_one_submit", "whb_cut_in_preamble_at_submit_cut")


def _tfa1_split(o):
    """-> (flushes of slot 0 ahead of the telegram's, the telegram's flush, the bits of its sync word that earlier windows hold) if
    there are such bits, else None.  (store_bit finds the word 16 bits behind its last bit, in the register's lower half: a
    word that lies in one window is found at bit 31 of the record or later.)"""
    ev = [e for e in o.events_full() if e[0] == 0]
    rep = tfa1_replay(records(o, 0))
    for k, e in enumerate(ev):
        if e[7] == 1 and rep[k][1] is not None and rep[k][1] < 31:
            return ev[:k], e, 31 - rep[k][1]
    return None


def splices_classes(batch):
    hit = set()
    m = np.cumsum(S.CARRIED_CUTS) * S.BLOCK_DEC
    bits_seen = set()
    for row, iq, o in batch:
        sp = _tfa1_split(o)
        if sp:
            before, tel, ahead = sp
            bits_seen.add(ahead)
            recs = records(o, 0)
            empty = sum(1 for r in recs[1:len(before)] if not r)  # windows without a bit between the first part's and the telegram's
            assert before and before[0][2] == 0 and all(e[2] == 0 for e in before)
            first_end, tel_open = before[0][1], tel[1] - S.WINDOW[0]
            cuts_between = [c for c in m if first_end - S.WINDOW[0] < c < tel_open + 100]
            if len(before) == 1 and not cuts_between:
                hit.add("tfa1_split_one_submit")
            if len(before) == 1 and any(first_end < c for c in cuts_between):
                hit.add("tfa1_split_window0_of_next_submit")
            if len(before) == 1 and any(c <= first_end for c in cuts_between):
                hit.add("tfa1_split_open_at_submit_cut")
            short = [r for r in recs[1:len(before)] if 0 < len(r) < 32]  # windows between that hold a few bits of the word
            if len(before) == 2 and len(short) == 1 and ahead > len(short[0]):  # ... and the window before them the rest
                hit.add("tfa1_split_three_ways_window0_of_next_submit" if any(first_end < c < before[1][1] - S.WINDOW[0] for c in cuts_between)
                        else "tfa1_split_three_ways_one_submit")
            if len(before) == 2 and empty == 1 and not cuts_between:
                hit.add("tfa1_split_one_empty_window")
            if len(before) == 3 and empty == 2 and not cuts_between:
                hit.add("tfa1_split_two_empty_windows")
            if len(before) == 2 and empty == 1 and any(first_end < c < before[1][1] - S.WINDOW[0] for c in cuts_between):
                hit.add("tfa1_split_empty_window_behind_submit_cut")
        w = [e for e in o.events_full() if e[0] == 4 and e[7] == 1]
        if row["kind"] == "splice" and w:
            lo, hi = S.splice_parts(row)
            if (hi - lo) // 4 > S.WINDOW[4]:
                between = [c for c in m if lo // 4 < c < hi // 4]
                hit.add("whb_cut_in_preamble_at_submit_cut" if between else "whb_cut_in_preamble_one_submit")
    if len(bits_seen) >= 5 and min(bits_seen) <= 5 and max(bits_seen) >= 12 and all(1 <= b <= 15 for b in bits_seen):
        hit.add("tfa1_split_at_5_points")
    return hit


@pytest.mark.parametrize("label", SPLICES_CLASSES)
def test_splices_reach_every_class(label):
    assert label in splices_classes(results("splices"))


def test_the_split_telegram_exists_only_through_the_carried_shift_register():
    """Every TFA_1 splice row: the oracle decodes README.md:123's telegram in a window that holds fewer than 16 bits of its sync
    word; the same bits through store_bit with the shift register cleared by every flush find no sync word at all."""
    n = 0
    for row, iq, o in results("splices"):
        if not row["name"].startswith("tfa1"):
            continue
        sp = _tfa1_split(o)
        assert sp, row["name"]
        assert bytes(sp[1][5])[:11].hex() == S.TFA1_TELEGRAM and sp[1][2] >= 11, row["name"]
        assert "TFA1 ID 65b0 +22.0 35% seq e lowbat 0" in o.text(), row["name"]
        cleared = tfa1_replay(records(o, 0), zero_sr=True)
        assert all(s is None for _, s in cleared) and all(b == 0 for b, _ in cleared), row["name"]
        # and the uncut burst decodes the same telegram in one window
        whole = run(S.render(row["base"]))
        assert [bytes(e[5])[:11] for e in whole.events_full() if e[0] == 0 and e[7] == 1] == [bytes(sp[1][5])[:11]]
        n += 1
    assert n == 14


def test_whb_cut_in_the_preamble_decodes_and_the_descrambler_handed_over_decides_nothing():
    """The WHB rows: the second window begins 18 bits ahead of the sync word -- the nearest cut that decodes at all, see the header
    of the splices in oracle/scenes.py -- and the telegram is found with the descrambler cleared at that bit too: whb_demod hands
    over bits of its own at the cut, so the 17 bits the descrambler remembers are never the preamble's."""
    for row, iq, o in results("splices"):
        if not row["name"].startswith("whb"):
            continue
        at, behind = S.splice_parts(row)
        head = iq.copy()
        head[2 * at:] = 128
        first = run(head).pending_bits(4)   # the first window's bits: it ends unsynced, without a flush
        recs = records(o, 4)
        assert len(recs) == 1 and recs[0].startswith(first) and len(first) > 150, row["name"]
        n1 = len(first)
        byte_cnt, sync_at = whb_replay(recs)[0]
        lead = sync_at - 31 - n1          # bits of the second window ahead of the sync word's first
        assert 17 <= lead <= 20, (row["name"], lead)
        assert whb_replay(recs, {(0, n1)})[0] == (byte_cnt, sync_at), row["name"]
        # the uncut burst's bits: the cut added two
        whole = records(run(S.render(row["base"])), 4)[0]
        assert len(recs[0]) == len(whole) + 2 and recs[0][:n1 - 4] == whole[:n1 - 4], row["name"]
        assert (behind - at) // 4 > S.WINDOW[4]
