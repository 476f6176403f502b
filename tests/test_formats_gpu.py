"""Sample formats on the GPU (tfrec_amd_create_format, tfrec_gpu -F), bit for bit.

Stage 0 is pinned by the restatement (formats.to_x ahead of resample.resample_x16 and tune.mix_in_s16), everything behind it by
the oracle's process_s16 fed that restatement's output.  The scenes are input_rows.py's, where every restatement and oracle of a
scene is computed once per session; test_formats_cpu.py asserts that the oracle decodes at least 8 telegrams from each."""
import functools
import subprocess

import numpy as np
import pytest

import parity
import segments
from input_rows import KINDS, SCENE_BLOCKS, THRESH, TYPES, format_stage0, scene, scene_oracle, scene_stage0, scene_u8
from oracle import oracle as O
from tfrec_amd import api, formats, resample, tune

pytestmark = pytest.mark.gpu

FOUR = (3, 3, 3, 3)


run_input = functools.partial(parity.run_input, types=TYPES, thresh=THRESH)


# ---- stage 0 equals the restatement
@pytest.mark.parametrize("p,q", [(4, 3), (25, 16), (1, 1)])
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_stage0_equals_the_restatement(kind, p, q):
    """The first submit and three following ones: the history carry and both history buffers; at 1/1 stage 0 is x itself."""
    rows = scene(kind, p, q)
    _, y0 = run_input(rows, FOUR, p, q, KINDS[kind], all_flushes=True)
    for s in range(len(rows)):
        parity.assert_stage0(y0, FOUR, scene_stage0(kind, p, q, s), s, kind)


@pytest.mark.parametrize("p,q", [(29, 4), (639, 64)])
@pytest.mark.parametrize("fmt", ["s8", "s16", "f32"])
def test_stage0_of_the_large_rates(fmt, p, q):
    """One stream, two submits of one block, full-scale input.  639/64: the tap table, the int16 image of a whole tile and the
    cosine table exceed the LDS limit, so the kernel runs tiles of 512 outputs (the half tile), as its U8
    instantiation (the tuned u8 resampler) does at this rate.  29/4 = 7.25 input samples per output has 44 taps per phase and a tile's image of 30 KB: the largest image among
    the rates with a small Q, still in whole tiles."""
    sizes = (1, 1)
    rows = parity.full_scale_row(fmt, resample.input_samples(2, p, q), 29)
    _, y0 = run_input(rows, sizes, p, q, fmt, all_flushes=True, max_events=1 << 16)
    parity.assert_stage0(y0, sizes, format_stage0(fmt, rows[0], p, q), 0, fmt)


EDGES = [np.nan, np.inf, -np.inf, 2.0, -2.0, 1.0, -1.0, 0.99993896, -0.99993896, 0.5 / 8192, 1.5 / 8192, 2.5 / 8192, -0.5 / 8192,
         -1.5 / 8192, -2.5 / 8192, 8190.5 / 8192, 8191.5 / 8192, -8191.5 / 8192, 1e-45, -1e-45, 1.1e-38, -1.1e-38, 3.4e38, -3.4e38,
         1e35, 0.0, -0.0, float(np.nextafter(np.float32(0.5 / 8192), np.float32(0))), 0.25, -0.25, 0.7 / 8192]


@pytest.mark.parametrize("p,q,nb", [(1, 1, 1), (4, 3, 3)])
def test_f32_edge_values(p, q, nb):
    """NaN, +-inf, +-2, ties and denormals among ordinary samples, every edge value on either rail and at every position of a
    chunk: stage 0 at 1/1 is to_x of the row, at 4/3 the resampled to_x."""
    n = resample.input_samples(nb, p, q)
    rng = np.random.default_rng(5)
    v = (rng.random(2 * n, dtype=np.float32) - np.float32(0.5)).astype("<f4")
    at = rng.permutation(2 * n)[:40 * len(EDGES)]
    v[at] = np.tile(np.asarray(EDGES, dtype="<f4"), 40)
    v[:len(EDGES)] = EDGES  # ... and a run of them at the row's start, where a 4/3 stream's history is silence
    rows = v.view(np.uint8).reshape(1, -1)
    x = formats.to_x("f32", rows[0])
    assert np.isnan(v).any() and x.min() == -8192 and x.max() == 8191
    _, y0 = run_input(rows, (nb,), p, q, "f32", all_flushes=True, max_events=1 << 16)
    parity.assert_stage0(y0, (nb,), format_stage0("f32", rows[0], p, q), 0)


# ---- events equal the oracle behind the restatement
EVENT_RUNS = ([("deep", k, 4, 3) for k in ("s8", "s16", "f32")]
              + [("shallow", "s16", 4, 3), ("serial_chains", "f32", 4, 3), ("default_mode", "s8", 4, 3), ("bits", "s16", 4, 3),
                 ("host", "f32", 4, 3)]
              + [(m, k, 1, 1) for m in ("deep", "host") for k in ("s8", "s16", "f32")])


@pytest.mark.parametrize("mode,kind,p,q", EVENT_RUNS)
def test_events_equal_the_oracle_behind_the_restatement(mode, kind, p, q, monkeypatch):
    kw, layout, flags = parity.mode_kwargs(mode, monkeypatch)
    rows = scene(kind, p, q)
    layouts = []
    evs, _ = run_input(rows, FOUR, p, q, KINDS[kind], host=flags["host"], stage0=False, before=lambda r, k: layouts.append(r.layout()),
                       **kw)
    assert layouts[0] == layout
    ev = np.concatenate(evs)
    total = telegrams = 0
    for s in range(len(rows)):
        orc = scene_oracle(kind, p, q, s, flags["bits"])
        total += parity.assert_stream(ev, s, orc, default_mode=flags["default_mode"])
        if flags["bits"]:
            assert parity.assert_bits(ev, s, orc, "stream %d" % s) > 1000
        telegrams += sum(1 for e in orc.events_full() if e[7] == 1)
    assert total >= 8 and telegrams >= 8


# ---- cross-format identities: no oracle needed
@functools.lru_cache(maxsize=None)
def sorted_events(fmt, kind, p, q):
    """The sorted event bytes of a receiver of the format (None: the older constructors') over a scene's rows."""
    rows = scene_u8(p, q) if kind == "u8" else scene(kind, p, q)
    evs, _ = run_input(rows, FOUR, p, q, fmt, stage0=False, all_flushes=True)
    ev = parity.sort_events(np.concatenate(evs))
    assert len(ev) > 20
    return ev.tobytes()


@functools.lru_cache(maxsize=None)
def encoded(fmt, p, q):
    """The u8 scene's x, encoded exactly in the format."""
    u = scene_u8(p, q)
    return np.stack([formats.encode(fmt, formats.to_x("u8", row)) for row in u])


@pytest.mark.parametrize("p,q", [(4, 3), (1, 1)])
def test_s8_of_flipped_bytes_equals_the_u8_context(p, q):
    """Against Receiver(input_rate=(4, 3)) and against a plain Receiver: neither a delay nor a difference in any event byte."""
    assert np.array_equal(scene("s8", p, q) ^ 0x80, scene_u8(p, q))
    assert sorted_events("s8", "s8", p, q) == sorted_events(None, "u8", p, q)


@pytest.mark.parametrize("p,q", [(4, 3), (1, 1)])
def test_s16_and_f32_of_the_same_x_give_the_same_events(p, q):
    s16 = run_input(encoded("s16", p, q), FOUR, p, q, "s16", stage0=False, all_flushes=True)[0]
    f32 = run_input(encoded("f32", p, q), FOUR, p, q, "f32", stage0=False, all_flushes=True)[0]
    s16, f32 = parity.sort_events(np.concatenate(s16)), parity.sort_events(np.concatenate(f32))
    assert len(s16) > 20 and s16.tobytes() == f32.tobytes() == sorted_events(None, "u8", p, q)


# ---- per-stream operations on an S16 4/3 context
def test_reset_in_mid_stream_equals_a_fresh_receiver():
    p, q, kind = 4, 3, "s16"
    rows = scene(kind, p, q)
    evs, y0 = run_input(rows, FOUR, p, q, "s16", all_flushes=True, before=lambda r, k: r.reset_streams([1]) if k == 2 else None)
    cut = 4 * resample.input_samples(6, p, q)
    after = format_stage0("s16", rows[1][cut:], p, q)  # zero history behind the cut
    whole = scene_stage0(kind, p, q, 1)
    parity.assert_segment(np.concatenate(evs), 0, scene_oracle(kind, p, q, 0), "stream 0")
    o1, o2 = O.Oracle(TYPES, THRESH, 0), O.Oracle(TYPES, THRESH, 0)
    o1.process_s16(whole[:2 * 6 * 4 * api.BLOCK_DEC])
    o2.process_s16(after)
    first = parity.assert_segment(np.concatenate(evs[:2]), 1, o1, "stream 1 before the reset")
    second = parity.assert_segment(np.concatenate(evs[2:]), 1, o2, "stream 1 after the reset")
    assert first > 0 and second > 0
    # the history is silence: the first outputs after the cut are the restatement's from zero history, not the carried stream's
    assert np.array_equal(y0[2][1], after[:len(y0[2][1])])
    assert not np.array_equal(y0[2][1][:16], whole[2 * 6 * 4 * api.BLOCK_DEC:][:16])
    assert np.array_equal(y0[3][1], after[len(y0[2][1]):])
    parity.assert_stage0(y0, FOUR, scene_stage0(kind, p, q, 0), 0)


def test_reset_at_the_base_rate_behind_the_conversion():
    """An s8 context at 1/1 has the format conversion for a pre-stage and no pre-stage history: a reset of stream 1 before the
    second of three one-block submits restores the front end's int16 history alone.  s8 of flipped bytes is the u8 context, so
    the segment harness's oracles are fed the u8 rows.  Blocks 3 .. 5 of the scene: stream 1 has flushes before the reset and in
    the block right behind it (asserted on the oracles)."""
    u = scene_u8(1, 1)[:, 3 * api.BLOCK_BYTES:6 * api.BLOCK_BYTES]
    hosts = parity.cut(u, (1, 1, 1))
    with api.Receiver(2, TYPES, THRESH, 0, max_blocks=1, all_flushes=True, input_format="s8") as r:
        total, segs = segments.run_segments(r, [h ^ 0x80 for h in hosts], {1: [("reset", [1])]}, (TYPES, THRESH, 0), hosts=hosts)
    assert [g.k for g in segs[1]] == [0, 1] and all(len(g.orc.events_full()) > 0 for g in segs[1])
    assert total > 0


def test_configure_works():
    """Stream 1 is configured to TFA_1 alone and a threshold of its own before the first submit; stream 0 keeps the context's."""
    p, q, kind = 4, 3, "s16"
    rows = scene(kind, p, q)

    def before(r, k):
        if k == 0:
            r.configure_streams([1], types_mask=0x01, thresh=700)

    evs, _ = run_input(rows, FOUR, p, q, "s16", stage0=False, all_flushes=True, before=before)
    ev = np.concatenate(evs)
    o = O.Oracle(0x01, 700, 0)
    o.process_s16(scene_stage0(kind, p, q, 1))
    assert parity.assert_segment(ev, 1, o, "stream 1, configured") > 0
    assert parity.assert_segment(ev, 0, scene_oracle(kind, p, q, 0), "stream 0") > 0


TUNES = (200000, -200000)


@pytest.mark.parametrize("shared", [False, True])
def test_tunes_and_a_shared_row(shared):
    """tune_streams at +-200 kHz acts on y0: the oracle behind tune.mix_s16 of the restatement.  shared: the two streams are mapped
    to row 0 and the submit carries one row; otherwise each reads its own copy."""
    p, q, sizes = 4, 3, (3, 3)
    row = parity.tuned_row(p, q, TUNES, "s16")

    def before(r, k):
        if k == 0:
            if shared:
                r.map_streams([0, 1], [0, 0])
            r.tune_streams([0, 1], TUNES)
            assert r.rows_in_use == (1 if shared else 2)

    evs, y0 = run_input(row if shared else np.repeat(row, 2, axis=0), sizes, p, q, "s16", n_streams=2, before=before, all_flushes=True)
    ev = np.concatenate(evs)
    for s, hz in enumerate(TUNES):
        orc = parity.tuned_oracle(p, q, TUNES, "s16", 0, hz, types=TYPES, thresh=THRESH)
        assert parity.assert_segment(ev, s, orc, "stream %d tune %d" % (s, hz)) > 0
        assert parity.decoded(orc) == [s]  # each receiver decodes the burst it is tuned to
        parity.assert_stage0(y0, sizes, format_stage0("s16", row[0], p, q), s)  # stage 0 is ahead of the tune


def test_input_tune_beside_an_untuned_stream():
    """tune_streams_input at +900 kHz on a 25/16 context, an untuned stream in the same launch."""
    p, q, sizes, freqs = 25, 16, (1, 2, 2, 1), (0, 900000)
    row = parity.tuned_row(p, q, freqs, "s16")

    def before(r, k):
        if k == 0:
            r.tune_streams_input([1], [900000])
            assert r.stream_tune_input(1) == 900000 and r.stream_tune_input(0) == 0

    evs, y0 = run_input(np.repeat(row, 2, axis=0), sizes, p, q, "s16", before=before, all_flushes=True)
    ev = np.concatenate(evs)
    x = formats.to_x("s16", row[0])
    for s, hz in enumerate(freqs):
        orc = parity.tuned_oracle(p, q, freqs, "s16", hz, 0, types=TYPES, thresh=THRESH)
        assert parity.assert_segment(ev, s, orc, "stream %d input tune %d" % (s, hz)) > 0
        assert parity.decoded(orc) == [s]
        parity.assert_stage0(y0, sizes, resample.resample_x16(tune.mix_in_s16(x, hz, p, q), p, q), s)


def test_results_do_not_depend_on_the_cut():
    p, q = 4, 3
    one, _ = run_input(scene("s16", p, q), (SCENE_BLOCKS,), p, q, "s16", stage0=False, all_flushes=True)
    a = parity.sort_events(np.concatenate(one))
    assert len(a) > 20 and a.tobytes() == sorted_events("s16", "s16", p, q)


# ---- refusals
def test_refusals_leave_the_context_usable():
    L = api.load_library()
    h = api.C.c_void_p()
    cfg = api.Config(2, TYPES, THRESH, 0, 0, 3, 4096, api.F_ALL_FLUSHES | api.F_INPUT_10X)
    for fmt in (1, 2, 3):  # the 15.36 MS/s input with a format other than u8
        assert L.tfrec_amd_create_format(api.C.byref(cfg), fmt, 1, 1, api.C.byref(h)) == api.E_INVAL and not h
    cfg.flags = api.F_ALL_FLUSHES
    for fmt in (-1, 4):  # an unknown format
        assert L.tfrec_amd_create_format(api.C.byref(cfg), fmt, 4, 3, api.C.byref(h)) == api.E_INVAL and not h
    with pytest.raises(api.TfrecAmdError) as e:
        api.Receiver(2, TYPES, THRESH, 0, max_blocks=3, input_10x=True, input_format="s16")
    assert e.value.code == api.E_INVAL
    rows = scene("s16", 1, 1)[:, :4 * 3 * 32768]
    with api.Receiver(2, TYPES, THRESH, 0, max_blocks=3, all_flushes=True, input_format="s16") as r:  # 1/1
        assert r.input_rate == (1, 1) and r.input_format == "s16" and r.block_bytes == 2 * api.BLOCK_BYTES
        for call in (r.tune_streams_input, r.tune_streams_wide):  # the tune of a 1/1 context is tune_streams
            with pytest.raises(api.TfrecAmdError) as e:
                call([0], [100000])
            assert e.value.code == api.E_INVAL
        import torch

        d = torch.from_numpy(np.ascontiguousarray(rows)).to("cuda:0")
        short = d[:, :rows.shape[1] // 2].contiguous()  # rows as long as a u8 context's: the stride is shorter than an s16 row
        with pytest.raises(api.TfrecAmdError) as e:
            r.submit(short, n_blocks=3)
        assert e.value.code == api.E_INVAL
        with pytest.raises(api.TfrecAmdError) as e:
            r.submit(np.ascontiguousarray(rows[:, :rows.shape[1] // 2]), n_blocks=3)
        assert e.value.code == api.E_INVAL
        assert r.submit(d) == 3  # nothing was queued or marked: the context is the fresh one
        ev = r.drain()
        for s in range(2):
            o = O.Oracle(TYPES, THRESH, 0)
            o.process_s16(scene_stage0("s16", 1, 1, s)[:2 * 3 * 32768])
            parity.assert_segment(ev, s, o, "stream %d" % s)
    with api.Receiver(2, TYPES, THRESH, 0, max_blocks=3, all_flushes=True, input_format="f32", input_rate=(4, 3)) as r:
        with pytest.raises(api.TfrecAmdError) as e:
            r.tune_streams_wide([0], [1000])
        assert e.value.code == api.E_INVAL
        for nb in (1, 2):  # the block-count rule is the rate's
            with pytest.raises(api.TfrecAmdError):
                r.input_bytes(nb)
        assert r.input_bytes(3) == 8 * resample.input_samples(3, 4, 3)


# ---- unchanged answers
def test_u8_is_the_older_constructors():
    """tfrec_amd_create_format(U8, 4, 3) and (U8, 1, 1) report the layout, the memory and the events of tfrec_amd_create_rate and
    tfrec_amd_create; an S16 context holds at least the u8 one's memory."""
    for p, q in ((4, 3), (1, 1)):
        rows = scene_u8(p, q)[:, :2 * resample.input_samples(3, p, q)]
        got = []
        for kw in (dict(input_format="u8", input_rate=(p, q)), dict(input_rate=(p, q)) if (p, q) != (1, 1) else dict(),
                   dict(input_format="s16", input_rate=(p, q))):
            with api.Receiver(2, TYPES, THRESH, 0, max_blocks=3, all_flushes=True, **kw) as r:
                mem = r.memory()
                ev = None
                if kw.get("input_format") != "s16":
                    assert r.input_format == "u8" and r.input_bytes(3) == rows.shape[1]
                    r.submit(rows)
                    ev = parity.sort_events(r.drain()).tobytes()
                    mem = (mem, r.memory())  # ... with submit_host's staging buffer
                got.append((r.layout(), r.input_rate, mem, ev))
        assert got[0] == got[1] and len(got[0][3]) > 0
        assert got[2][0] == got[0][0] and got[2][2]["device_bytes"] >= got[0][2][0]["device_bytes"]


def test_memory_counts_the_history_and_the_staging_buffer():
    with api.Receiver(4, TYPES, THRESH, 0, max_blocks=3, input_rate=(25, 16)) as r:
        u8 = r.memory()["device_bytes"]
    with api.Receiver(4, TYPES, THRESH, 0, max_blocks=3, input_rate=(25, 16), input_format="f32") as r:
        assert r.memory()["device_bytes"] - u8 == 2 * 4 * (256 - 128)  # 64 complex samples of x instead of 64 of u8, two buffers
        before = r.memory()["device_bytes"]
        rows = np.zeros((4, r.input_bytes(1)), dtype=np.uint8)
        assert r.submit(rows) == 1
        assert r.memory()["device_bytes"] - before == rows.size == 4 * 8 * 51200  # submit_host staged the larger rows
        r.drain()
    with api.Receiver(4, TYPES, THRESH, 0, max_blocks=3) as r:
        plain = r.memory()["device_bytes"]
    with api.Receiver(4, TYPES, THRESH, 0, max_blocks=3, input_format="s8") as r:
        # stage 0 (one buffer per set) and the int16 FIR history instead of the u8 one
        assert r.memory()["device_bytes"] - plain == api.FIFO_DEPTH * 4 * 4 * 3 * api.BLOCK_DEC * 4 + 2 * 4 * 112


# ---- tfrec_gpu -F
def test_cli_replays_s16_and_f32_dumps(tmp_path):
    """tfrec_gpu -r 2048000 -F s16 / f32 on the same scene written out as .cs16 and .cf32 files (the same x): both print the
    telegram lines of the host decoders fed by the oracle behind the restatement, and the same text as each other."""
    cli = parity.build_cli()
    p, q = 4, 3
    text = {}
    for fmt in ("s16", "f32"):
        rows = encoded(fmt, p, q)
        for s in range(len(rows)):
            f = tmp_path / ("s%d.c%s" % (s, fmt))
            np.concatenate([rows[s], np.zeros(1000, dtype=np.uint8)]).tofile(f)  # (a trailing partial piece is dropped)
            out = subprocess.run([cli, "-r", "2048000", "-F", fmt, "-T", "%x" % TYPES, "-t", str(THRESH), "-b", "4", "-L", str(f)],
                                 capture_output=True, text=True, timeout=600)
            assert out.returncode == 0 and "rounded up to 6" in out.stderr, out.stderr
            o = O.Oracle(TYPES, THRESH, 0)
            o.process_s16(format_stage0(fmt, rows[s], p, q))
            want = [ln for ln in o.text().splitlines() if ln.strip() and not ln.startswith("Inverted") and not ln.startswith("WHB:")]
            got = [ln for ln in out.stdout.splitlines() if ln.strip() and not ln.startswith("WHB:")]
            assert got == want and len(want) >= 4, (fmt, s)
            text[fmt, s] = out.stdout
    assert all(text["s16", s] == text["f32", s] for s in range(2))
