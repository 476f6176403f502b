"""bench.py itself, on the GPU box: the single-rank line and the N>1 code path (two ranks of bench.py on ONE device, gloo
for the barrier / scalar reduces -- the data path has no collective), so that the rendezvous, the barrier + MAX-reduce
bracket and the per-rank seeding have run before the driver's 8-GPU launch."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _line(out):
    return json.loads([ln for ln in out.splitlines() if ln.startswith('{"metric"')][-1])


COMMON = ["--steps", "3", "--warmup", "1", "--streams", "64", "--blocks", "8", "--cpu-budget", "0"]


def test_bench_single_rank_line():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full"] + COMMON + ["--h2d-steps", "2"],
                         capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    j = _line(out.stdout)
    assert j["n_gpus"] == 1 and j["value"] > 0 and j["unit"] == "MSamples/s"
    c = j["config"]
    assert c["parity_ok"] is True and c["parity_gate_streams"] == 64  # every stream of the batch
    assert c["atan_host_mismatch"] == 0
    # slow-path decisions beyond the per-submit log are exact by construction but not compared with this host's libm: none
    # unless a submit resolved more than the log holds
    assert c["atan_unverified"] == 0 or c["atan_resolved"] > 62
    # the batch AFTER the timed region (carried state, FIFO four deep) against the oracle continued over every repetition
    assert c["parity_after_timed"] is True and c["parity_after_timed_streams"] == 64
    assert c["parity_after_timed_batches_carried"] == 1 + 1 + 3
    rf = j["roofline"]
    assert rf["hbm_floor_ms"] > 0 and rf["algorithmic_valu_floor_ms"] > rf["hbm_floor_ms"]
    assert j["ms_min"] <= j["ms_median"] <= j["ms_max"]
    assert 0 < j["roofline"]["frac"] < 1 and 0 < j["roofline"]["whole_path_frac"] < 1
    assert j["h2d_included"]["value"] > 0 and j["h2d_included"]["value"] <= j["value"] * 1.05


def test_bench_two_ranks_gloo_on_one_device():
    port = _free_port()
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", LOCAL_RANK=str(r), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dist-backend", "gloo",
                                       "--same-device", "--full"] + COMMON, env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.PIPE, text=True, cwd=ROOT))
    outs = [p.communicate(timeout=900) for p in procs]
    assert all(p.returncode == 0 for p in procs), [o[1][-1500:] for o in outs]
    assert not [ln for ln in outs[1][0].splitlines() if ln.startswith('{"metric"')]  # only rank 0 prints
    j = _line(outs[0][0])
    assert j["n_gpus"] == 2 and j["scaling"] == "weak" and j["value"] > 0
    c = j["config"]
    assert c["parity_ok"] is True and c["dist_backend"] == "gloo" and c["atan_host_mismatch"] == 0
    assert len(c["rank_input_crc32"]) == 2 and c["rank_input_crc32"][0] != c["rank_input_crc32"][1]  # distinct streams per rank
    assert c["events_all_ranks"] > c["events_per_step"] * j["steps"]  # both ranks' events counted
    # value is the whole job: both ranks' samples over the slowest rank's time
    assert abs(j["value"] - 2 * 64 * 8 * 32768 * j["steps"] / (j["ms_per_step"] * j["steps"] * 1e-3) / 1e6) / j["value"] < 1e-3


def test_bench_gpus_2_launches_its_own_ranks():
    """Plain `python bench.py --gpus 2` (no RANK / WORLD_SIZE in the environment): bench.py starts the two ranks itself
    through torch.distributed.run and reports n_gpus = the ranks that really ran (it used to run ONE rank and
    print n_gpus 1)."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--same-device", "--dist-backend",
                          "gloo", "--full"] + COMMON, capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    j = _line(out.stdout)
    assert j["n_gpus"] == 2 and j["config"]["parity_ok"] is True
    assert len(j["config"]["rank_input_crc32"]) == 2


def test_bench_gpus_4_same_device():
    """BASELINE configs[3] dry run: FOUR ranks of bench.py (64 streams x 8 blocks each) on one device, gloo for the barrier and
    the scalar reduces -- rendezvous of N > 2, per-rank seeding, the barrier + MAX-reduce bracket, several contexts' memory and
    the whole-job value, before an 8-GPU node ever runs it.  Four ranks, not eight: together with this process no more than
    six processes may have one device open.  The rendezvous of eight ranks is covered without a GPU in test_sharding_gloo.py.
    No scaling figure is taken from this."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4", "--same-device", "--dist-backend",
                          "gloo", "--full"] + COMMON, capture_output=True, text=True, timeout=1500, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    j = _line(out.stdout)
    assert j["n_gpus"] == 4 and j["scaling"] == "weak" and j["value"] > 0
    c = j["config"]
    assert c["parity_ok"] is True and c["parity_after_timed"] is True and c["atan_host_mismatch"] == 0
    assert len(set(c["rank_input_crc32"])) == 4  # four distinct sets of streams
    assert c["events_all_ranks"] > 2 * c["events_per_step"] * j["steps"]
    assert abs(j["value"] - 4 * 64 * 8 * 32768 * j["steps"] / (j["ms_per_step"] * j["steps"] * 1e-3) / 1e6) / j["value"] < 1e-3


def test_bench_dump_outputs_are_the_same_run_to_run(tmp_path):
    """--dump-outputs: the events of the last timed step, written after the timed region; the same command line gives the same
    input and therefore the same files, and --steps sets the number of timed steps."""
    dumps = []
    for k in range(2):
        d = tmp_path / ("run%d" % k)
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--h2d-steps", "0", "--dump-outputs", str(d)] + COMMON,
                             capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert out.returncode == 0, out.stderr[-2000:]
        j = _line(out.stdout)
        assert j["steps"] == 3 and j["ms_per_step"] > 0 and len(j["step_ms"]) == 3
        assert j["dump_outputs"]["events"] > 0 and j["dump_outputs"]["sampled"] is False
        files = sorted(os.listdir(d))
        assert "events_stream.npy" in files and "events_rdata.npy" in files
        assert sum(os.path.getsize(d / f) for f in files) <= 64 * 10 ** 6
        arrs = {f[:-4]: np.load(d / f) for f in files}
        assert all(a.dtype in (np.float32, np.float64) for a in arrs.values())
        assert all(len(a) == j["dump_outputs"]["events"] for a in arrs.values())
        assert arrs["events_stream"].min() >= 0 and arrs["events_stream"].max() < 64
        dumps.append(arrs)
    assert dumps[0].keys() == dumps[1].keys()
    for f in dumps[0]:
        assert np.array_equal(dumps[0][f], dumps[1][f]), f


def test_bench_plain_run_leaves_the_checks_to_full_and_dumps_the_same(tmp_path):
    """A plain run times the steps and prints the line without the oracle gates, the CPU baseline or the PCIe leg; it still
    submits the gate's batch first, so the timed steps see the same state as under --full and write the same outputs."""
    lines, dumps = {}, {}
    for mode in ("plain", "full"):
        d = tmp_path / mode
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--dump-outputs", str(d), "--h2d-steps", "2",
                              "--steps", "3", "--warmup", "1", "--streams", "64", "--blocks", "8", "--cpu-budget", "1"]
                             + (["--full"] if mode == "full" else []), capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert out.returncode == 0, out.stderr[-2000:]
        lines[mode] = _line(out.stdout)
        dumps[mode] = {f: np.load(d / f) for f in sorted(os.listdir(d))}
    p, f = lines["plain"], lines["full"]
    for k in ("metric", "unit", "higher_is_better", "dtype", "steps", "warmup"):
        assert p[k] == f[k], k
    assert p["value"] > 0 and p["ms_per_step"] > 0 and len(p["step_ms"]) == 3
    assert p["config"]["parity_ok"] is None and p["config"]["parity_after_timed"] is None
    assert p["config"]["atan_host_mismatch"] == 0
    assert not {"cpu_baseline", "h2d_included", "other_configs"} & p.keys()
    assert f["config"]["parity_ok"] is True and f["config"]["parity_after_timed"] is True
    assert {"cpu_baseline", "h2d_included"} <= f.keys()
    assert p["config"]["events_per_step"] == f["config"]["events_per_step"]
    assert p["dump_outputs"]["events"] > 0 and dumps["plain"].keys() == dumps["full"].keys()
    for name in dumps["plain"]:
        assert np.array_equal(dumps["plain"][name], dumps["full"][name]), name
