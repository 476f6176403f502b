"""Cost of the pulse slicer: kernel time of pulse_kernel and pulse_pack_kernel beside amplitude_kernel's in ONE context
with the amplitude track, on the track's cost input (track_cost.py's) in the same submits.

    python profiles/ubench/pulse_cost.py [--out DIR] [--streams 1024] [--blocks 48] [--submits 12] [--bursts 6] [--smooth 11]

starts `rocprofv3 --kernel-trace --stats -- python pulse_cost.py --workload ...` as a child process under a time limit (a kernel
trace in a run of its own, nothing else traced), reads the kernel trace it wrote and prints, per kernel, the median and the range of
the launches.  The slicer is in WIDTH mode with FS20's widths (100, 192, 300); the input's bursts are noise, so nearly every pulse
is a glitch: what a submit full of real pulse-width traffic costs is not what this measures.  A record, not a gate.
"""
from __future__ import annotations

import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from resample_cost import WARMUP, durations  # noqa: E402
from track_cost import TIME_LIMIT  # noqa: E402

KERNELS = ("pulse_kernel", "pulse_pack_kernel", "pulse_zero_kernel", "run_records_init_kernel<tfrec_amd_burst_symbols>", "linecode_carry_kernel",
           "amplitude_kernel", "capture_copy_kernel")


def workload(n_streams: int, n_blocks: int, submits: int, bursts: int, smooth: int, level: int) -> None:
    import numpy as np
    import torch

    from tfrec_amd import api, pulsecode

    g = torch.Generator(device="cuda:0").manual_seed(3)  # track_cost.py's input, byte for byte
    iq = torch.randint(124, 133, (n_streams, n_blocks * api.BLOCK_BYTES), dtype=torch.uint8, device="cuda:0", generator=g)
    where = torch.randint(0, api.BLOCK_BYTES - 4000, (n_blocks * bursts,), generator=torch.Generator().manual_seed(4)).tolist()
    for k, off in enumerate(where):
        a = (k // bursts) * api.BLOCK_BYTES + off
        iq[:, a:a + 4000] = torch.randint(0, 256, (n_streams, 4000), dtype=torch.uint8, device="cuda:0", generator=g)
    torch.cuda.synchronize()
    samples = n_streams * n_blocks * api.BLOCK_DEC
    with api.Receiver(n_streams, 0x2F, 500, 0, max_blocks=n_blocks) as r:
        r.enable_capture(n_streams * (n_blocks * api.BLOCK_DEC // 356 + 3), samples)  # a pool for every sample
        r.enable_burst_track_amplitude(smooth)
        r.set_burst_track_level(range(n_streams), level)
        r.enable_burst_symbols(pulsecode.WIDTH, 100, 192, 300)
        for k in range(WARMUP + submits):
            r.submit(iq, n_blocks)
            if k == WARMUP + submits - 1:
                recs = r.read_burst_symbols()[0]
                print("pulse_cost totals: %d runs, %d samples captured of %d, %d symbols, %d breaks, %d glitches" % (
                    len(recs), int(recs["n_samples"].astype(np.int64).sum()), samples, int(recs["n_symbols"].astype(np.int64).sum()),
                    int(recs["n_breaks"].astype(np.int64).sum()), int(recs["n_glitches"].astype(np.int64).sum())), flush=True)
            r.drain()
        r.sync()


def report(trace_dir: str, n_streams: int, n_blocks: int, submits: int) -> str:
    d = durations(trace_dir)
    lines = ["pulse_cost: %d streams x %d blocks per submit, %d submits after %d warm-up submits, one context" % (n_streams, n_blocks, submits, WARMUP)]
    for kernel in KERNELS:
        t = sum((d[k] for k in sorted(d) if kernel in k), [])
        if not t:
            lines.append("%-50s no launches found" % kernel)
            continue
        lines.append("%-50s median %8.3f ms  range %8.3f .. %8.3f ms  (%d launches, warm-up included)" % (
            kernel, statistics.median(t) / 1e6, min(t) / 1e6, max(t) / 1e6, len(t)))
    return "\n".join(lines)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", action="store_true", help="run the submits (what the profiler traces)")
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "pulse_cost"))
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--blocks", type=int, default=48)
    ap.add_argument("--submits", type=int, default=12)
    ap.add_argument("--bursts", type=int, default=6)
    ap.add_argument("--smooth", type=int, default=11)
    ap.add_argument("--level", type=int, default=3000)
    a = ap.parse_args()
    if a.workload:
        workload(a.streams, a.blocks, a.submits, a.bursts, a.smooth, a.level)
        return 0
    os.makedirs(a.out, exist_ok=True)
    cmd = ["timeout", "-k", "10", str(TIME_LIMIT), "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", a.out,
           "-o", "pulse_cost", "--", sys.executable, os.path.abspath(__file__), "--workload", "--streams", str(a.streams),
           "--blocks", str(a.blocks), "--submits", str(a.submits), "--bursts", str(a.bursts), "--smooth", str(a.smooth),
           "--level", str(a.level)]
    child = subprocess.run(cmd, check=True, capture_output=True, text=True)
    text = report(a.out, a.streams, a.blocks, a.submits) + "\n" + "\n".join(ln for ln in child.stdout.splitlines() if ln.startswith("pulse_cost "))
    print(text)
    with open(os.path.join(a.out, "pulse_cost.txt"), "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
