"""The segment harness of the per-stream operations (reset, configure, tune, wide tune, map): a stream is cut at its restarts,
and each segment -- from the stream's start or a restart on -- is compared with a fresh oracle of the segment's settings fed the
input of the row the stream reads, through tune.py's restatement of the mixers and the 10:1 stage.  Imported as a plain module
(`import segments`) like parity."""
import numpy as np

import parity
from oracle import oracle as O
from tfrec_amd import api, tune

CONFIG_KEYS = ("types_mask", "thresh", "filter_type")


class Segment:
    """One segment of a stream: the submit it starts at, its settings (types, thresh, filter), tunes and input row, its oracle,
    and what it has been fed so far."""

    def __init__(self, k, cfg, tune_hz=0, wide_hz=0, row=0, bits=False, in10x=False):
        self.k, self.cfg, self.tune, self.wide, self.row, self.in10x = k, cfg, tune_hz, wide_hz, row, in10x
        self.orc = O.Oracle(cfg[0], cfg[1], cfg[2], log_bits=bits, keep_dec=True)
        self.n = 0        # 1.536 MS/s samples fed
        self.hist = None  # in10x: the last 50 mixed input samples
        self.y0 = None    # in10x: the 10:1 stage's output of the last part

    def feed(self, part_u8):
        x16 = tune.s16_of_u8(np.asarray(part_u8))
        if self.in10x:
            xm = tune.mix10_s16(x16, self.wide, 10 * self.n)
            x16 = self.y0 = tune.decim10_s16(xm, hist=self.hist)
            self.hist = xm[-100:]
        self.orc.process_s16(tune.mix_s16(x16, self.tune, self.n))
        self.n += len(x16) // 2


def run_segments(r, parts, ops, dflt, *, hosts=None, rows0=None, in10x=False, bits=False, default_mode=False, read_between=True):
    """Submit parts[k] ([rows, bytes]; numpy, or device tensors with hosts[k] the numpy copies) through parity.run_fifo.  ops[k]:
    ("map", streams, rows) | ("tune", streams, hz) | ("wide", streams, hz) | ("conf", streams, [(types, thresh, filter), ..]) |
    ("reset", streams), applied before submit k while older submits are still queued; every stream an op names restarts at
    submit k.  Before every submit the context's getters are compared with the bookkeeping here; after the run every stream's
    decimated samples and threshold with its last segment's oracle, and every segment's events with its oracle (dflt: the
    context's settings).

    read_between: feed the oracles and compare the threshold (in10x: stage 0 too) after every submit.  False: nothing is read
    from the receiver between the submits, so that they queue up to the FIFO's depth; the oracles are fed after the last drain.
    -> (events compared, the segments per stream)."""
    hosts = parts if hosts is None else hosts
    n = r.n_streams
    cfg, tn, wd = [dflt] * n, [0] * n, [0] * n
    row = list(range(n)) if rows0 is None else list(rows0)
    book = {"map": row, "tune": tn, "wide": wd, "conf": cfg}
    segs = [[] for _ in range(n)]
    mapped = []

    def call(op):
        if op[0] == "map":
            r.map_streams(op[1], op[2])
            mapped.append(True)
        elif op[0] == "tune":
            r.tune_streams(op[1], op[2])
        elif op[0] == "wide":
            r.tune_streams_wide(op[1], op[2])
        elif op[0] == "conf":
            r.configure_streams(op[1], types_mask=[c[0] for c in op[2]], thresh=[c[1] for c in op[2]],
                                filter_type=[c[2] for c in op[2]])
        else:
            assert op[0] == "reset", op
            r.reset_streams(op[1])

    def before(k):
        restart = set()
        for op in ops.get(k, ()):
            call(op)
            if op[0] != "reset":
                for s, v in zip(op[1], op[2]):  # (a duplicate index: the last value wins)
                    book[op[0]][s] = v
            restart |= set(op[1])
        for s in range(n):
            assert r.stream_config(s) == dict(zip(CONFIG_KEYS, cfg[s])), "stream %d" % s
            assert (r.stream_input(s), r.stream_tune(s), r.stream_tune_wide(s)) == (row[s], tn[s], wd[s]), "stream %d" % s
            if k == 0 or s in restart:
                segs[s].append(Segment(k, cfg[s], tn[s], wd[s], row[s], bits, in10x))
        if mapped:
            assert r.rows_in_use == 1 + max(row)

    def feed(k):
        for s in range(n):
            g = [g for g in segs[s] if g.k <= k][-1]
            g.feed(hosts[k][g.row])

    def after(k):
        feed(k)
        for s in range(n):
            g = segs[s][-1]
            assert r.thresh(s) == g.orc.thresh(), "stream %d submit %d threshold" % (s, k)
            if in10x:
                assert np.array_equal(r.stage0(s, len(g.y0) // 2), g.y0), "stream %d submit %d stage 0" % (s, k)

    evs = parity.run_fifo(r, parts, before=before, after=after if read_between else None)
    if not read_between:
        for k in range(len(hosts)):
            feed(k)
    m = hosts[-1].shape[1] // r.block_bytes * api.BLOCK_DEC
    total = 0
    for s in range(n):
        last = segs[s][-1].orc
        assert np.array_equal(r.decimated(s, m), last.dec()[-2 * m:]), "stream %d decimated" % s
        assert r.thresh(s) == last.thresh(), "stream %d threshold" % s
        bounds = [g.k for g in segs[s]] + [len(hosts)]
        for i, g in enumerate(segs[s]):
            ev = np.concatenate([e[e["stream"] == s] for e in evs[bounds[i]:bounds[i + 1]]])
            label = "stream %d segment %d row %d settings %s tune %d wide %d" % (s, i, g.row, g.cfg, g.tune, g.wide)
            if default_mode:
                total += parity.assert_stream(ev, s, g.orc, label, default_mode=True)
            else:
                total += parity.assert_segment(ev, s, g.orc, label, bits)
            own = {j for j in range(5) if g.cfg[0] & (1 << (j if j < 4 else 5))}
            assert set(np.unique(ev["slot"]).tolist()) <= own, "%s: a slot outside its types" % label
    return total, segs
