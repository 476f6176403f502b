"""The harness of the save / load tests (tfrec_amd_save_streams / tfrec_amd_load_streams): context A runs the first part of its rows
and saves its streams, context B -- 65 streams -- loads the blobs into other streams, one of them stream 64, and runs the rest; both
against one context U that ran both parts.  And the input condition such a test rests on: a telegram whose window is open at the
cut.  Imported as a plain module (`import state_harness`) like parity."""
import numpy as np

import parity
from tfrec_amd import api

NB_ = 65                      # B's streams
DST = (64, 0, 33, 63, 17)     # where A's streams 0 .. 4 continue in B


def open_at_the_cut(run, rows_x, first, across, label, only=None):
    """The input condition.  run(x) -> a fresh oracle over one row's samples x (whatever the receiver's input is restated as).
    Row k: its planted burst begins before the cut and ends behind it, the uninterrupted run decodes a slot-k telegram (status 1)
    whose flush lies behind the cut and within a window's timeout of the burst's end -- its trigger window was open at the cut --,
    and a fresh receiver on the second part alone does not produce that telegram.  -> the oracles."""
    m = first * api.BLOCK_DEC
    out = []
    for k, (x, cut) in enumerate(rows_x):
        if only is not None and k != only:
            continue
        start, n = across[k]
        assert start < m < start + n, label
        whole = run(x)
        tail = run(x[cut:])
        hit = [e for e in whole.events_full() if e[0] == k and e[7] == 1 and m < e[1] < start + n + 1000]
        assert hit, "%s row %d: no telegram across the cut" % (label, k)
        assert not [v for v in tail.events_full() if v[0] == k and v[7] == 1 and v[5] == hit[0][5]], \
            "%s row %d: the second part alone decodes the telegram" % (label, k)
        out.append(whole)
    return out


def relabel(ev, mapping):
    """B's events of the streams mapping's keys, named as their source streams; the rest dropped."""
    keep = np.isin(ev["stream"], list(mapping))
    out = ev[keep].copy()
    out["stream"] = np.array([mapping[int(s)] for s in out["stream"]], dtype=out["stream"].dtype) if len(out) else out["stream"]
    return parity.sort_events(out)


def same(a, b, label=""):
    a, b = parity.sort_events(a), parity.sort_events(b)
    assert len(a) == len(b) and a.tobytes() == b.tobytes(), label


def b_rows(part, others=None):
    """B's input for one submit: the sources' rows at DST, `others` (or silence) elsewhere."""
    fill = np.full((NB_, part.shape[1]), 128 if part.dtype == np.uint8 else 0, dtype=part.dtype) if others is None else others.copy()
    for i, j in enumerate(DST[:len(part)]):
        fill[j] = part[i]
    return fill


def continue_in_b(parts, make, submit=None, setup=None, others=None, side=None):
    """U runs parts[0] and parts[1]; A runs parts[0] and saves; B (65 streams) loads into DST and runs parts[1].
    make(n_streams) -> a Receiver; setup(r, streams): tunes and settings of the source streams, on U and A; side(r) -> what is
    read from a receiver before each drain (compared too).  -> (A's events, B's relabelled, U's per submit, blobs, B's all)."""
    n = len(parts[0])
    submit = submit or (lambda r, x: r.submit(x))
    src = list(range(n))
    with make(n) as u:
        if setup:
            setup(u, src)
        want, want_side = [], []
        for x in parts:
            submit(u, x)
            want_side.append(side(u) if side else None)
            want.append(u.drain())
    with make(n) as a:
        if setup:
            setup(a, src)
        submit(a, parts[0])
        side_a = side(a) if side else None
        ev_a = a.drain()
        blobs = a.save_streams(src)
        assert blobs.shape == (n, a.state_bytes)
        again = a.save_streams(src)
        assert again.tobytes() == blobs.tobytes(), "two saves differ"
    same(ev_a, want[0], "A is the uninterrupted run's first part")
    with make(NB_) as b:
        b.load_streams(DST[:n], blobs)
        back = b.save_streams(DST[:n])
        assert back.tobytes() == blobs.tobytes(), "a blob saved from B straight after the load is not A's"
        x = parts[1]
        fill = b_rows(x, others) if isinstance(x, np.ndarray) else x
        submit(b, fill)
        side_b = side(b) if side else None
        ev_b = b.drain()
    got = relabel(ev_b, {j: i for i, j in enumerate(DST[:n])})
    same(got, want[1], "B continues as the uninterrupted run")
    return ev_a, got, want, blobs, ev_b, (side_a, side_b, want_side)
