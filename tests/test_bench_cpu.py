"""bench.py's launcher logic that needs no GPU."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_refuses_a_world_size_that_is_not_gpus():
    """`--gpus 2` inside a job of another size: an error, never a line with a different n_gpus."""
    env = dict(os.environ, RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"],
                         capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert out.returncode != 0 and "--gpus 2" in out.stderr
    assert not [ln for ln in out.stdout.splitlines() if ln.startswith('{"metric"')]


def test_dump_outputs_writes_float_arrays_within_the_limit(tmp_path, monkeypatch):
    """--dump-outputs' writer: one float64 file per integer field of the events (float32 for rdata) in drain order, exact;
    past the size limit a fixed sample of rows, the same one every time, with its row numbers."""
    import numpy as np

    import bench
    from tfrec_amd import api

    rng = np.random.default_rng(5)
    ev = np.zeros(1000, dtype=api.EVENT_DTYPE)
    for f in ev.dtype.names:
        info = np.iinfo(ev.dtype[f].base)
        ev[f] = rng.integers(max(info.min, -(1 << 40)), min(info.max, 1 << 40), size=ev[f].shape, endpoint=True)
    res = bench.dump_outputs(str(tmp_path / "all"), ev)
    assert res == {"dir": str(tmp_path / "all"), "events": 1000, "events_written": 1000, "sampled": False}
    for f in ev.dtype.names:
        a = np.load(tmp_path / "all" / ("events_%s.npy" % f))
        assert a.dtype == (np.float32 if f == "rdata" else np.float64)
        assert np.array_equal(a, ev[f])
    assert np.array_equal(np.load(tmp_path / "all" / "events_row.npy"), np.arange(1000))

    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 16 * 1024 + 100 * 328)  # room for 100 rows of 328 bytes
    rows = []
    for k in range(2):
        d = tmp_path / ("part%d" % k)
        res = bench.dump_outputs(str(d), ev)
        assert res["events"] == 1000 and res["events_written"] == 100 and res["sampled"] is True
        r = np.load(d / "events_row.npy").astype(np.int64)
        assert np.all(np.diff(r) > 0)
        assert np.array_equal(np.load(d / "events_seq.npy"), ev["seq"][r])
        rows.append(r)
    assert np.array_equal(rows[0], rows[1])
