"""The level meter (TFREC_AMD_F_LEVELS, include/tfrec_amd.h: tfrec_amd_level) restated in numpy -- no GPU needed.

Per block of 8192 decimated samples of ONE stream: the power the receiver saw (energy, pwr_sum, pwr_max, n_over) and the trigger
bookkeeping of the reference's fsk_demod::process (fm_demod.cpp:36-73: triggered, thresh, triggered_avg).  Two forms:

  levels             vectorised, from the definition in the header: sample n is triggered iff a sample n' with pwr > thresh lies
                     in (n - W, n], W the largest window of the registered demodulators;
  levels_bruteforce  a per-sample simulation straight from the reference's text: one timeout_cnt per registered demodulator, set
                     to its window at pwr > thresh, counted while non-zero, then decremented (tfa1.cpp:147-164, tfa2.cpp:351-375,
                     whb.cpp:636-657); the sample counts when any demodulator returned non-zero (fm_demod.cpp:48-52).

Both take the decimated samples as tfrec_amd_read_decimated returns them (int16, I and Q interleaved, or shaped [n, 2]), the
stream's -T mask and its -t (0: auto, starting at 500), and a `state` to continue a stream over several calls; both return
(records, state), records a LEVEL_DTYPE array with one entry per block.
"""
from __future__ import annotations

import numpy as np

BLOCK_DEC = 8192
LEN = 2 * BLOCK_DEC  # 'len' of fsk_demod::process (int16 values per block): the thresholds of fm_demod.cpp:64-68 are len/32, len/64

LEVEL_DTYPE = np.dtype([("energy", "<u8"), ("pwr_sum", "<u4"), ("pwr_max", "<i4"), ("n_over", "<i4"), ("triggered", "<i4"),
                        ("thresh", "<i4"), ("triggered_avg", "<i4")])
assert LEVEL_DTYPE.itemsize == 32

# sensor_e bit (main.cpp -T) -> the demodulator's trigger window in decimated samples: 40 * BITPERIOD (tfa1.cpp:148),
# (int)(16 * spb) with spb = 384000 / baud (tfa2.cpp:355; main.cpp:186-205), (int)(8 * spb) with spb = 64 (whb.cpp:641)
_NO_WINDOW = -(1 << 40)


def windows(types_mask: int) -> list:
    """The trigger windows of the demodulators -T types_mask registers, in registration order (main.cpp:173-218)."""
    w = []
    if types_mask & 0x01:
        w.append(400)
    for bit, baud in ((0x02, 17240), (0x04, 9600), (0x08, 8842)):
        if types_mask & bit:
            w.append(int(16 * (384000.0 / baud)))
    if types_mask & 0x20:
        w.append(int(8 * (384000.0 / 6000)))
    if not w or types_mask & ~0x2F:
        raise ValueError("types_mask 0x%x registers no demodulator or an unknown one" % types_mask)
    return w


def _iq(dec):
    a = np.asarray(dec)
    assert a.dtype == np.int16, a.dtype
    a = a.reshape(-1, 2).astype(np.int64)
    assert len(a) % BLOCK_DEC == 0, "whole blocks of %d decimated samples" % BLOCK_DEC
    return a[:, 0], a[:, 1]


def _start(thresh: int) -> dict:
    """fsk_demod::fsk_demod, fm_demod.cpp:18-32; last_trig: the last trigger, relative to the next call's first sample."""
    assert thresh >= 0
    return {"thresh": thresh if thresh else 500, "auto": thresh == 0, "triggered_avg": 0, "runs": 0, "last_trig": _NO_WINDOW}


def _step(st: dict, triggered: int) -> None:
    """The end of fsk_demod::process, fm_demod.cpp:58-73 (runs was incremented at its head, :37)."""
    st["triggered_avg"] = (31 * st["triggered_avg"] + triggered) // 32
    if st["auto"] and (st["runs"] & 3) == 0:
        if st["triggered_avg"] >= LEN // 32:
            st["thresh"] += 2
        elif st["triggered_avg"] <= LEN // 64 and st["thresh"] > 50:
            st["thresh"] -= 2


def levels(dec, types_mask: int, thresh: int, state: dict | None = None):
    """-> (records[n_blocks], state).  state: None for a fresh stream (or one that restarts here), else what an earlier call
    returned for the samples just before these."""
    I, Q = _iq(dec)
    W = max(windows(types_mask))
    st = dict(state) if state is not None else _start(thresh)
    nb = len(I) // BLOCK_DEC
    rec = np.zeros(nb, dtype=LEVEL_DTYPE)
    idx = np.arange(BLOCK_DEC, dtype=np.int64)
    last = st["last_trig"]  # relative to the current block's first sample
    for b in range(nb):
        i, q = I[b * BLOCK_DEC:(b + 1) * BLOCK_DEC], Q[b * BLOCK_DEC:(b + 1) * BLOCK_DEC]
        pwr = np.abs(i) + np.abs(q)
        over = pwr > st["thresh"]
        st["runs"] += 1
        # the last trigger at or before every sample, the one carried in included
        lt = np.maximum(np.maximum.accumulate(np.where(over, idx, _NO_WINDOW)), last)
        triggered = int(np.count_nonzero(idx - lt < W))
        r = rec[b]
        r["energy"] = int(np.sum(i * i + q * q))
        r["pwr_sum"] = int(pwr.sum())
        r["pwr_max"] = int(pwr.max())
        r["n_over"] = int(np.count_nonzero(over))
        r["triggered"] = triggered
        r["thresh"] = st["thresh"]
        _step(st, triggered)
        r["triggered_avg"] = st["triggered_avg"]
        last = max(int(lt[-1]) - BLOCK_DEC, _NO_WINDOW)
    st["last_trig"] = last
    return rec, st


def levels_bruteforce(dec, types_mask: int, thresh: int, state: dict | None = None):
    """The same records from a sample-by-sample run of the reference's loops.  Its state carries the demodulators' timeout
    counters instead of a last trigger; the two kinds of state are not interchangeable."""
    I, Q = _iq(dec)
    win = windows(types_mask)
    if state is not None:
        st = dict(state)
        cnt = list(st["timeout_cnt"])
    else:
        st = _start(thresh)
        del st["last_trig"]
        cnt = [0] * len(win)  # tfa1.cpp:140, tfa2.cpp:319, whb.cpp:608
    nb = len(I) // BLOCK_DEC
    rec = np.zeros(nb, dtype=LEVEL_DTYPE)
    Il, Ql = I.tolist(), Q.tolist()
    for b in range(nb):
        triggered = n_over = pwr_sum = pwr_max = energy = 0
        st["runs"] += 1  # fm_demod.cpp:37
        th = st["thresh"]
        for n in range(b * BLOCK_DEC, (b + 1) * BLOCK_DEC):
            i, q = Il[n], Ql[n]
            pwr = abs(i) + abs(q)  # fm_demod.cpp:45
            t = 0
            for k, w in enumerate(win):  # demodulator::demod, fm_demod.cpp:48-49
                if pwr > th:
                    cnt[k] = w
                if cnt[k]:
                    t += 1
                    cnt[k] -= 1
            if t:
                triggered += 1  # fm_demod.cpp:51-52
            n_over += pwr > th
            pwr_sum += pwr
            pwr_max = max(pwr_max, pwr)
            energy += i * i + q * q
        rec[b] = (energy, pwr_sum, pwr_max, n_over, triggered, th, 0)
        _step(st, triggered)
        rec[b]["triggered_avg"] = st["triggered_avg"]
    st["timeout_cnt"] = cnt
    return rec, st


def next_thresh(rec, auto: bool, runs: int) -> int:
    """The threshold in force AFTER the block of record `rec`, the runs-th (1-based) of its stream since the start or last
    restart: the step of fm_demod.cpp:63-73 applied to the record's thresh and triggered_avg."""
    st = {"thresh": int(rec["thresh"]), "auto": auto, "triggered_avg": int(rec["triggered_avg"]), "runs": runs}
    if st["auto"] and (runs & 3) == 0:
        if st["triggered_avg"] >= LEN // 32:
            st["thresh"] += 2
        elif st["triggered_avg"] <= LEN // 64 and st["thresh"] > 50:
            st["thresh"] -= 2
    return st["thresh"]


def scan_channels(center_khz: int, step_khz: int, fs_in: int) -> list:
    """tfrec_gpu -s: the channels c + k * step (kHz) with |k * step * 1000| <= fs_in / 2 - 192000, ascending."""
    assert step_khz >= 1
    kmax = (fs_in - 384000) // (2000 * step_khz)
    return [center_khz + k * step_khz for k in range(-kmax, kmax + 1)]


def scan_line(khz: int, rec, telegrams: int) -> str:
    """tfrec_gpu -s: one channel's line from its records (every block of the file)."""
    n = len(rec)
    return "scan %d blocks=%d mean_pwr=%d peak=%d over=%d triggered=%d thresh=%d telegrams=%d" % (
        khz, n, int(rec["pwr_sum"].astype(np.int64).sum()) // (BLOCK_DEC * n), int(rec["pwr_max"].max()),
        int(rec["n_over"].astype(np.int64).sum()), int(rec["triggered"].astype(np.int64).sum()), int(rec["thresh"][-1]), telegrams)
