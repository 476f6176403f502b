"""CPU tests of the shared GPU parity harness (tests/parity.py, tests/segments.py): the parts the GPU suite can check only
indirectly -- the order in which run_fifo submits and drains, the cuts, the default-mode rule, the parse of the oracle's bit
log, a segment's oracle fed part by part, the stage-0 comparison, the table of modes, and the rule that no file under tests/
imports a test module."""
import glob
import os
from types import SimpleNamespace

import numpy as np
import pytest

import parity
import segments
from oracle import oracle as O
from tfrec_amd import api, formats, resample, synth, tune


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


# ---- segments.Segment
SEGMENT_CASES = {"default": (False, 0, 0), "input_10x": (True, 0, 0), "tuned": (False, -200000, 0),
                 "input_10x-wide-tuned": (True, 25000, 2500000)}  # (10x input, tune, wide tune)


@pytest.mark.parametrize("case", sorted(SEGMENT_CASES))
def test_segment_fed_in_ragged_parts_equals_the_oracle_fed_the_whole(case):
    """The history of the 10:1 stage and the phases of both mixers carry from part to part: the events, the decimated samples
    and the (auto) threshold are those of one oracle behind the restatement of the whole input -- without a tune, of
    parity.fresh_oracle, which on 10x is oracle.decim10 of the whole."""
    in10x, hz, wide = SEGMENT_CASES[case]
    sizes, mult = ((2, 1, 2), 10) if in10x else ((3, 2, 3), 1)
    n = sum(sizes) * api.BLOCK_BYTES // 2 * mult
    bursts = [dict(proto=j, start=(20000 * mult + j * (n - 40000 * mult) // 3) // mult * mult, payload_seed=7 + 11 * j,
                   f0_hz=wide + hz, amp=50 + 10 * j) for j in range(3)]  # test_tune_gpu.make_input's bursts, at the tune
    x = synth.gen_scene(2100, sum(sizes), bursts, rate_mult=mult)
    cfg = (0x2F, 0, 0)
    seg = segments.Segment(0, cfg, hz, wide, in10x=in10x)
    for part in parity.cut(x[None, :], sizes, api.BLOCK_BYTES * mult):
        seg.feed(part[0])
    if hz == 0 and wide == 0:
        want = parity.fresh_oracle(x, *cfg, in10x=in10x, keep_dec=True)
    else:
        x16 = tune.s16_of_u8(x)
        want = O.Oracle(*cfg, keep_dec=True)
        want.process_s16(tune.mix_s16(tune.decim10_s16(tune.mix10_s16(x16, wide)) if in10x else x16, hz))
    assert seg.n == sum(sizes) * 4 * api.BLOCK_DEC
    assert len(want.events_full()) > 0 and parity.decoded(want) != []
    assert seg.orc.events_full() == want.events_full()
    assert np.array_equal(seg.orc.dec(), want.dec()) and len(want.dec()) == 2 * sum(sizes) * api.BLOCK_DEC
    assert seg.orc.thresh() == want.thresh()


# ---- the input runner's parts
@pytest.mark.parametrize("p,q,sizes", [(1, 1, (3, 3, 3, 3)), (4, 3, (3, 3, 3, 3)), (25, 16, (3, 3, 3, 3)), (25, 16, (1, 2, 1, 2))])
@pytest.mark.parametrize("fmt", ["u8", "s8", "s16", "f32"])
def test_cut_input_reproduces_the_byte_slices(fmt, p, q, sizes):
    lens = [formats.bytes_per_sample(fmt) * resample.input_samples(nb, p, q) for nb in sizes]
    rows = np.random.default_rng(4).integers(0, 256, (2, sum(lens)), dtype=np.uint8)
    parts = parity.cut_input(rows, sizes, fmt, p, q)
    assert [part.shape for part in parts] == [(2, n) for n in lens] and all(part.flags["C_CONTIGUOUS"] for part in parts)
    bounds = np.cumsum([0] + lens)
    for part, a, b in zip(parts, bounds, bounds[1:]):
        assert np.array_equal(part, rows[:, a:b])
    assert np.array_equal(np.concatenate(parts, axis=1), rows)
    if (fmt, p, q) == ("u8", 1, 1):
        assert all(np.array_equal(a, b) for a, b in zip(parts, parity.cut(rows, sizes)))
        assert all(np.array_equal(a, b) for a, b in zip(parity.cut_input(rows, sizes), parts))  # (the defaults)
    with pytest.raises(AssertionError):
        parity.cut_input(np.concatenate([rows, rows[:, :1]], axis=1), sizes, fmt, p, q)


def test_assert_stage0_names_the_stream_and_the_submit():
    sizes = (1, 2, 1)
    per = 2 * 4 * api.BLOCK_DEC
    want = np.random.default_rng(6).integers(-8192, 8192, (2, sum(sizes) * per)).astype(np.int16)
    bounds = np.cumsum((0,) + sizes) * per
    y0 = [[want[s, a:b].copy() for s in range(2)] for a, b in zip(bounds, bounds[1:])]
    for s in range(2):
        parity.assert_stage0(y0, sizes, want[s], s)
        parity.assert_stage0(y0, sizes, want[s], s, "label", tile=512)
    y0[2][1][-3] ^= 1  # one value of stream 1's last submit
    parity.assert_stage0(y0, sizes, want[0], 0)
    with pytest.raises(AssertionError, match=r"4/3 stream 1 submit 2$"):
        parity.assert_stage0(y0, sizes, want[1], 1, "4/3")
    with pytest.raises(AssertionError, match=r"stream 1 submit 2: first differing output %d \(mod 512: %d, mod 8: %d\), 1 values" % (
            per // 2 - 2, (per // 2 - 2) % 512, (per // 2 - 2) % 8)):
        parity.assert_stage0(y0, sizes, want[1], 1, tile=512)
    with pytest.raises(AssertionError, match=r"stream 0: 5 values expected behind submit 2"):  # `want` goes on behind the submits
        parity.assert_stage0(y0, sizes, np.concatenate([want[0], want[0][:5]]), 0)
    y0[0][1][0] ^= 1
    parity.assert_stage0(y0[:2] + [[y0[2][0], want[1, bounds[2]:]]], sizes, want[1, per:], 1, first=1)  # first=1 skips submit 0
    with pytest.raises(AssertionError, match=r"stream 1 submit 0"):
        parity.assert_stage0(y0, sizes, want[1], 1)


@pytest.mark.parametrize("mode", ["deep", "shallow", "serial_chains", "default_mode", "bits", "host"])
def test_mode_kwargs_is_the_table_the_modules_spelt_out(mode, monkeypatch):
    monkeypatch.delenv("TFREC_AMD_DEEP", raising=False)
    kw, layout, flags = parity.mode_kwargs(mode, monkeypatch)
    assert sorted(parity.MODES) == sorted(["deep", "shallow", "serial_chains", "default_mode", "bits", "host"])
    assert kw == dict(all_flushes=mode != "default_mode", bits=mode == "bits", serial_chains=mode == "serial_chains",
                      experiments=mode == "shallow")
    assert layout == {"shallow": 4, "serial_chains": 2}.get(mode, 6)
    assert layout == {"deep": 6, "shallow": 4, "serial_chains": 2, "default_mode": 6, "bits": 6, "host": 6}[mode]
    assert flags == dict(bits=mode == "bits", default_mode=mode == "default_mode", host=mode == "host")
    assert os.environ.get("TFREC_AMD_DEEP") == ("0" if mode == "shallow" else None)


def test_no_file_under_tests_imports_a_test_module():
    """What test modules share lives in plain modules (parity, segments, recorder, recorder_rows, input_rows, meter_rows,
    stream_count_rows): which tests are collected never decides which test modules are loaded."""
    assert parity.imports_of("<from>", "from test_levels_cpu import crafted_dec\n") == {"test_levels_cpu"}
    assert parity.imports_of("<inside>", "import os.path\n\n\ndef f():\n    import test_x as X\n    return X\n") == {"os", "test_x"}
    paths = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "*.py")))
    assert len(paths) > 50
    for p in paths:
        found = sorted(m for m in parity.imports_of(p) if m.startswith("test_"))
        assert not found, "%s imports %s" % (os.path.basename(p), found)
