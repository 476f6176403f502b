"""Cost of the burst track's phase mode: kernel times of carrier_head_kernel, phase_kernel and phase_carry_kernel
beside track_kernel's in frequency mode, on the track's cost input (track_cost.py's), in the same session and process.

    python profiles/ubench/phase_cost.py [--out DIR] [--streams 1024] [--blocks 48] [--submits 12] [--bursts 6] [--smooth 11] [--head 1024]
                                         [--lag 10]

starts `rocprofv3 --kernel-trace --stats -- python phase_cost.py --workload ...` as a child process under a time limit (a kernel
trace in a run of its own, nothing else traced), reads the kernel trace it wrote and prints, per kernel, the median and the range of
the launches.  Two contexts one after the other, each with the recorder and a pool for every sample: one with the phase track
(K = `--head`, m = `--lag`), one with the frequency track.  The floor named beside the kernels' times is one read of the captured pairs.
A record, not a gate.
"""
from __future__ import annotations

import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from resample_cost import HBM_PEAK, WARMUP, durations  # noqa: E402
from track_cost import TIME_LIMIT  # noqa: E402

KERNELS = ("carrier_head_kernel", "phase_kernel", "phase_carry_kernel", "centre_carry_kernel", "track_kernel",
           "run_records_init_kernel<tfrec_amd_track_centre>", "run_records_init_kernel<tfrec_amd_track>", "track_carry_kernel",
           "capture_copy_kernel")
KINDS = ("phase", "frequency")


def workload(n_streams: int, n_blocks: int, submits: int, bursts: int, smooth: int, head: int, lag: int) -> None:
    import torch

    from tfrec_amd import api

    g = torch.Generator(device="cuda:0").manual_seed(3)  # track_cost.py's input, byte for byte
    iq = torch.randint(124, 133, (n_streams, n_blocks * api.BLOCK_BYTES), dtype=torch.uint8, device="cuda:0", generator=g)
    where = torch.randint(0, api.BLOCK_BYTES - 4000, (n_blocks * bursts,), generator=torch.Generator().manual_seed(4)).tolist()
    for k, off in enumerate(where):
        a = (k // bursts) * api.BLOCK_BYTES + off
        iq[:, a:a + 4000] = torch.randint(0, 256, (n_streams, 4000), dtype=torch.uint8, device="cuda:0", generator=g)
    torch.cuda.synchronize()
    samples = n_streams * n_blocks * api.BLOCK_DEC
    max_runs = n_streams * (n_blocks * api.BLOCK_DEC // 356 + 3)
    for kind in KINDS:
        with api.Receiver(n_streams, 0x2F, 500, 0, max_blocks=n_blocks) as r:
            r.enable_capture(max_runs, samples)  # a pool for every sample: what the bitmap is sized by
            if kind == "phase":
                r.enable_burst_track_phase(smooth, head, lag)
            else:
                r.enable_burst_track(smooth)
            t0 = 0.0
            nr, npairs = api.C.c_uint32(0), api.C.c_uint64(0)
            for k in range(WARMUP + submits):
                if k == WARMUP:
                    r.sync()
                    t0 = time.perf_counter()
                r.submit(iq, n_blocks)
                r.L.tfrec_amd_read_captures(r.h, None, 0, api.C.byref(nr), None, 0, api.C.byref(npairs))
                r.drain()
            r.sync()
            print("phase_cost period: %s context %.3f ms per submit (submit, the counts, drain; %d submits)"
                  % (kind, 1e3 * (time.perf_counter() - t0) / submits, submits), flush=True)
            print("phase_cost totals: %d runs, %d pairs of %d samples per submit (captured share %.4f)"
                  % (nr.value, npairs.value, samples, npairs.value / samples), flush=True)


def report(trace_dir: str, n_streams: int, n_blocks: int, submits: int, pairs: int) -> str:
    d = durations(trace_dir)
    lines = ["phase_cost: %d streams x %d blocks per submit, %d timed submits per context after %d warm-up submits" % (
        n_streams, n_blocks, submits, WARMUP)]
    for kernel in KERNELS:
        t = sum((d[k] for k in sorted(d) if kernel in k), [])
        if not t:
            lines.append("%-46s no launches found" % kernel)
            continue
        lines.append("%-46s median %8.3f ms  range %8.3f .. %8.3f ms  (%d launches, warm-up included)" % (
            kernel, statistics.median(t) / 1e6, min(t) / 1e6, max(t) / 1e6, len(t)))
    lines.append("traffic floor of either kernel (the captured pairs read once: %.3f GB) %.3f ms at 8 TB/s" % (
        4 * pairs / 1e9, 1e3 * 4 * pairs / HBM_PEAK))
    return "\n".join(lines)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", action="store_true", help="run the submits (what the profiler traces)")
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "phase_cost"))
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--blocks", type=int, default=48)
    ap.add_argument("--submits", type=int, default=12)
    ap.add_argument("--bursts", type=int, default=6)
    ap.add_argument("--smooth", type=int, default=11)
    ap.add_argument("--head", type=int, default=1024)
    ap.add_argument("--lag", type=int, default=10)
    a = ap.parse_args()
    if a.workload:
        workload(a.streams, a.blocks, a.submits, a.bursts, a.smooth, a.head, a.lag)
        return 0
    os.makedirs(a.out, exist_ok=True)
    cmd = ["timeout", "-k", "10", str(TIME_LIMIT), "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", a.out,
           "-o", "phase_cost", "--", sys.executable, os.path.abspath(__file__), "--workload", "--streams", str(a.streams),
           "--blocks", str(a.blocks), "--submits", str(a.submits), "--bursts", str(a.bursts), "--smooth", str(a.smooth),
           "--head", str(a.head), "--lag", str(a.lag)]
    child = subprocess.run(cmd, check=True, capture_output=True, text=True)
    info = [ln for ln in child.stdout.splitlines() if ln.startswith("phase_cost ")]
    pairs = 0
    for ln in info:
        if ln.startswith("phase_cost totals:"):
            pairs = int(ln.split()[4])
    text = report(a.out, a.streams, a.blocks, a.submits, pairs) + "\n" + "\n".join(info)
    print(text)
    with open(os.path.join(a.out, "phase_cost.txt"), "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
