"""CPU tests of the shared GPU parity harness (tests/parity.py): the parts the GPU suite can check only indirectly -- the
order in which run_fifo submits and drains, the cuts, the default-mode rule and the parse of the oracle's bit log."""
from types import SimpleNamespace

import numpy as np
import pytest

import parity
from oracle import oracle as O
from tfrec_amd import api, synth


class FakeReceiver:
    """Records submit / drain calls; refuses a submit beyond the FIFO depth like the real context."""

    def __init__(self, log):
        self.log, self.pending, self.n = log, [], 0

    def submit(self, p):
        assert len(self.pending) < api.FIFO_DEPTH, "submit with the FIFO full"
        self.log.append("s%d" % self.n)
        self.pending.append(self.n)
        self.n += 1

    def drain(self):
        k = self.pending.pop(0)
        self.log.append("d%d" % k)
        return k


def fifo_log(n_parts, depth, hooks=False):
    log = []
    r = FakeReceiver(log)
    kw = dict(before=lambda k: log.append("b%d" % k), after=lambda k: log.append("a%d" % k)) if hooks else {}
    out = parity.run_fifo(r, list(range(n_parts)), depth=depth, **kw)
    assert out == list(range(n_parts))  # one drain per submit, in order
    return " ".join(log)


def test_run_fifo_call_order():
    assert fifo_log(7, 4) == "s0 s1 s2 s3 d0 s4 d1 s5 d2 s6 d3 d4 d5 d6"
    assert fifo_log(5, 2) == "s0 s1 d0 s2 d1 s3 d2 s4 d3 d4"
    assert fifo_log(4, 1) == "s0 d0 s1 d1 s2 d2 s3 d3"
    assert fifo_log(3, 4) == fifo_log(3, 3) == "s0 s1 s2 d0 d1 d2"  # depth >= parts: queue everything, then drain
    assert fifo_log(0, 4) == ""


def test_run_fifo_hooks_run_around_each_submit():
    # before(k) while the FIFO is still full, ahead of the drain that frees a slot for submit k; after(k) right after it
    assert fifo_log(6, 4, hooks=True) == "b0 s0 a0 b1 s1 a1 b2 s2 a2 b3 s3 a3 b4 d0 s4 a4 b5 d1 s5 a5 d2 d3 d4 d5"
    assert fifo_log(3, 1, hooks=True) == "b0 s0 a0 b1 d0 s1 a1 b2 d1 s2 a2 d2"


def test_run_fifo_matches_the_counting_loop_it_replaced():
    """The loop the tests wrote out by hand: submit k+depth is queued before submit k is drained."""
    for n_parts in range(9):
        for depth in (1, 2, 3, 4):
            log = []
            r = FakeReceiver(log)
            q = 0
            for k in range(n_parts):
                while q < n_parts and q - k < depth:
                    r.submit(q)
                    q += 1
                r.drain()
            assert fifo_log(n_parts, depth) == " ".join(log), (n_parts, depth)


@pytest.mark.parametrize("block", [api.BLOCK_BYTES, 10 * api.BLOCK_BYTES])
def test_cut_reproduces_the_block_slices(block):
    sizes = (1, 7, 3, 2)
    iq = np.random.default_rng(3).integers(0, 256, (2, sum(sizes) * block), dtype=np.uint8)
    parts = parity.cut(iq, sizes, block)
    bounds = np.cumsum((0,) + sizes)
    assert len(parts) == len(sizes)
    for p, a, b in zip(parts, bounds, bounds[1:]):
        assert np.array_equal(p, iq[:, a * block:b * block])
    assert np.array_equal(np.concatenate(parts, axis=1), iq)
    assert parity.cut(iq, ()) == []


def test_default_mode_rule():
    minb = {0: 10, 1: 7, 2: 7, 3: 7, 4: 11}
    slot, n = np.meshgrid(np.arange(5), np.arange(301), indexing="ij")
    for dtype in (api.EVENT_DTYPE, O.ORC_EVENT_DTYPE):
        ev = np.zeros(slot.size, dtype=dtype)
        ev["slot"], ev["byte_cnt"] = slot.ravel(), n.ravel()
        mask = parity.reported_mask(ev)
        for k, (s, b) in enumerate(zip(slot.ravel().tolist(), n.ravel().tolist())):
            want = b >= minb[s] and not (s == 3 and b >= 64) and not (s == 4 and b > 60)
            assert parity.reported(s, b) == want == bool(mask[k]), (s, b)


def test_oracle_bits_parses_records_in_flush_order():
    log = SimpleNamespace(bits_text=lambda: "W 1 3 010\nW 0 2 11\nW 1 0\nW 1 1 1\n")
    assert parity.oracle_bits(log) == {1: ["010", "", "1"], 0: ["11"]}
    assert parity.oracle_bits(SimpleNamespace(bits_text=lambda: "")) == {}


def test_oracle_bits_of_a_real_run():
    """Oracle(log_bits=True): one record per flush of each slot, in flush order, each as long as its bit count."""
    o = parity.fresh_oracle(synth.gen_batch(43, 3, 1, 24)[0], 0x2F, 500, log_bits=True)
    got = parity.oracle_bits(o)
    flushes = parity.by_slot(o.events_full())
    assert sorted(got) == sorted(flushes) == [0, 1, 2, 3, 4]
    lines = [ln.split() for ln in o.bits_text().splitlines()]
    assert all(p[0] == "W" for p in lines)
    for slot, recs in got.items():
        mine = [p for p in lines if int(p[1]) == slot]
        assert len(recs) == len(flushes[slot])
        assert [len(b) for b in recs] == [int(p[2]) for p in mine]
        assert "".join(recs) == "".join(p[3] for p in mine if len(p) > 3) and set("".join(recs)) <= {"0", "1"}
    assert sum(len(b) for recs in got.values() for b in recs) > 5000
