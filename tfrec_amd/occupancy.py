"""CPU restatement of the occupancy detector and of the grouping of its hits into channels (include/tfrec_amd.h:
tfrec_amd_enable_occupancy), in exact integers.  Written from the definition alone: nothing here calls the C library.

    m[k]    sum[k] // n_frames                                   per record of the spectrum (spectrum.py)
    floor   the lower median of m: sorted ascending, the value at index N/2 - 1
    top     max_k peak[k]
    hit[k]  peak[k] > max(floor, 1) * ratio  and  peak[k] * rel >= top
    bitmap  bit (k & 31) of word (k >> 5) is hit[k]

peak < 2^49 and ratio, rel <= 2^12: both products stay below 2^61, so uint64 holds them.
"""
from __future__ import annotations

import numpy as np

RATIO = 32          # the default: e^-32 per frame and bin for exponentially distributed noise power
REL = 16            # the default: bins within 12 dB of the record's strongest
RATIO_RANGE = (2, 4096)
REL_RANGE = (1, 4096)
JOIN_HZ = 50000     # the default gap that still joins two active bins into one channel
MAX_CHANNELS = 4096
SCAN_EDGE_HZ = 192000  # a scanned channel lies this far inside the recording (the scan's own rule)

OCC_DTYPE = np.dtype([("floor", "<u8"), ("n_hit", "<u4"), ("n_frames", "<u4")])
assert OCC_DTYPE.itemsize == 16


def _check(ratio: int, rel: int) -> None:
    if not RATIO_RANGE[0] <= ratio <= RATIO_RANGE[1]:
        raise ValueError("ratio %r outside [%d, %d]" % ((ratio,) + RATIO_RANGE))
    if not REL_RANGE[0] <= rel <= REL_RANGE[1]:
        raise ValueError("rel %r outside [%d, %d]" % ((rel,) + REL_RANGE))


def occupancy(sum_, peak, n_frames, ratio: int = RATIO, rel: int = REL):
    """The detector on the records of one row (spectrum.spectrum's output: sum[n_records, N], peak[n_records, N],
    n_frames[n_records]) -> (records: OCC_DTYPE [n_records], bitmap: uint32 [n_records, N / 32])."""
    _check(ratio, rel)
    s = np.asarray(sum_, dtype=np.uint64)
    p = np.asarray(peak, dtype=np.uint64)
    nf = np.asarray(n_frames, dtype=np.uint64)
    assert s.ndim == 2 and s.shape == p.shape and nf.shape == (s.shape[0],) and s.shape[1] % 32 == 0
    nr, n = s.shape
    recs = np.zeros(nr, dtype=OCC_DTYPE)
    bits = np.zeros((nr, n // 32), dtype=np.uint32)
    if nr == 0:
        return recs, bits
    assert int(p.max()) < 1 << 49 and (nf >= 1).all()
    m = s // nf[:, None]
    floor = np.sort(m, axis=1)[:, n // 2 - 1]
    top = p.max(axis=1)
    hit = (p > (np.maximum(floor, np.uint64(1)) * np.uint64(ratio))[:, None]) & (p * np.uint64(rel) >= top[:, None])
    recs["floor"] = floor
    recs["n_hit"] = hit.sum(axis=1)
    recs["n_frames"] = nf
    bits[:] = pack(hit)
    return recs, bits


def pack(hit) -> np.ndarray:
    """hit[..., N] (bool) -> uint32 [..., N / 32]: bit (k & 31) of word (k >> 5) is hit[k]."""
    h = np.asarray(hit, dtype=bool)
    w = h.reshape(h.shape[:-1] + (h.shape[-1] // 32, 32)).astype(np.uint64) << np.arange(32, dtype=np.uint64)
    return w.sum(axis=-1).astype(np.uint32)


def unpack(bitmap, n_bins: int | None = None) -> np.ndarray:
    """The bitmap words uint32 [..., N / 32] -> hit[..., N] (bool)."""
    b = np.asarray(bitmap, dtype=np.uint32)
    h = ((b[..., None] >> np.arange(32, dtype=np.uint32)) & np.uint32(1)).astype(bool)
    h = h.reshape(b.shape[:-1] + (b.shape[-1] * 32,))
    assert n_bins is None or h.shape[-1] == n_bins
    return h


def channels(hits, records: int, n_bins: int, fs_in: int, center_khz: int, join_hz: int = JOIN_HZ):
    """Group the hit counts of a recording into channels.  hits[k]: in how many of its `records` records bin k was hit.
    -> a list, in ascending frequency, of dicts
        {"kind": "carrier", "khz", "bin" (signed), "hits"}                   a bin hit in more than half of the records
        {"kind": "found", "khz", "lo", "hi" (signed bins), "hits" (the largest of the group), "in_range"}
    Python ints throughout: exact."""
    hits = [int(v) for v in hits]
    n, fs_in, records, join_hz, center_khz = int(n_bins), int(fs_in), int(records), int(join_hz), int(center_khz)
    assert len(hits) == n and join_hz >= 0
    signed = sorted((k if k < n // 2 else k - n, hits[k]) for k in range(n))  # b = -N/2 .. N/2 - 1
    out = []
    group = None  # [lo, hi, max hits]
    for b, h in signed:
        if h < 1:
            continue
        if 2 * h > records:
            # (the carrier's frequency: the group formula on the one bin)
            out.append({"kind": "carrier", "khz": center_khz + (2 * b * fs_in + 1000 * n) // (2000 * n), "bin": b, "hits": h})
            continue
        if group is not None and (b - group[1] - 1) * fs_in <= join_hz * n:
            group[1] = b
            group[2] = max(group[2], h)
            continue
        group = [b, b, h]
        out.append(group)
    res = []
    for g in out:
        if isinstance(g, dict):
            res.append((2 * g["bin"], g))
            continue
        lo, hi, h = g
        off = ((lo + hi) * fs_in + 1000 * n) // (2000 * n)
        res.append((lo + hi, {"kind": "found", "khz": center_khz + off, "lo": lo, "hi": hi, "hits": h,
                              "in_range": 2000 * abs(off) <= fs_in - 2 * SCAN_EDGE_HZ}))
    if sum(1 for _, g in res if g["kind"] == "found") > MAX_CHANNELS:
        raise ValueError("more than %d channels" % MAX_CHANNELS)
    # ascending frequency: by twice the middle bin (a carrier may lie inside a group's span; the sort is stable)
    return [g for _, g in sorted(res, key=lambda t: t[0])]
