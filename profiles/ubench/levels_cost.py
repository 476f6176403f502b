"""Cost of the level meter: kernel time of level_sum_kernel and level_trig_kernel at 1024 streams x 48 blocks, next
to their floor -- the decimated samples and the trigger mask read once, 4 B + 1/8 B per decimated sample, at the 8 TB/s HBM peak.

    python profiles/ubench/levels_cost.py [--out DIR] [--streams 1024] [--blocks 48] [--submits 12]

starts `rocprofv3 --kernel-trace --stats -- python levels_cost.py --workload ...` as a child process under a time limit (a kernel
trace in a run of its own, nothing else traced), reads the kernel trace it wrote and prints, per kernel, the median and the range
of the timed launches, the bytes a launch reads and the achieved bandwidth.  The first two submits are warm-up and are left out.
The input is near-silence: nothing triggers, so the demodulator chains beside the meter are idle and the kernels are timed alone
(beside a busy pipeline they run at low priority and stretch).  It also prints the wall-clock period per submit of the flagged
context and of an unflagged one on the same input, for information.  A record, not a gate.
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

TIME_LIMIT = 600  # seconds, for the traced child


def workload(n_streams: int, n_blocks: int, submits: int) -> None:
    import torch

    from tfrec_amd import api

    iq = torch.randint(124, 133, (n_streams, n_blocks * api.BLOCK_BYTES), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    for flagged in (True, False):
        with api.Receiver(n_streams, 0x2F, 500, 0, max_blocks=n_blocks, levels=flagged) as r:
            t0 = 0.0
            for k in range(WARMUP + submits):
                if k == WARMUP:
                    r.sync()
                    t0 = time.perf_counter()
                r.submit(iq, n_blocks)
                if flagged:
                    r.read_levels()
                r.drain()
            r.sync()
            print("levels_cost period: %s context %.3f ms per submit (submit, %sdrain; quiet input, %d submits)"
                  % ("flagged" if flagged else "plain", 1e3 * (time.perf_counter() - t0) / submits, "read_levels, " if flagged else "",
                     submits), flush=True)


def report(trace_dir: str, n_streams: int, n_blocks: int, submits: int) -> str:
    d = durations(trace_dir)
    samples = n_streams * n_blocks * 8192
    lines = ["levels_cost: %d streams x %d blocks per submit, %d timed submits after %d warm-up submits" % (n_streams, n_blocks, submits, WARMUP)]
    # level_sum_kernel reads the samples and the mask; level_trig_kernel the mask alone
    for kernel, nbytes in (("level_sum_kernel", samples * 4 + samples // 8), ("level_trig_kernel", samples // 8)):
        t = sum((d[k] for k in sorted(d) if kernel in k), [])[WARMUP:]
        if not t:
            lines.append("%-20s no launches found" % kernel)
            continue
        med = statistics.median(t)
        lines.append("%-20s median %8.3f ms  range %8.3f .. %8.3f ms  (%d launches)  reads %6.3f GB  floor %6.3f ms at 8 TB/s  achieved %5.2f TB/s"
                     % (kernel, med / 1e6, min(t) / 1e6, max(t) / 1e6, len(t), nbytes / 1e9, 1e3 * nbytes / HBM_PEAK, nbytes / med * 1e9 / 1e12))
    lines.append("floor of both together (samples and mask read once, 4 B + 1/8 B per decimated sample): %.3f ms"
                 % (1e3 * (samples * 4 + samples // 8) / HBM_PEAK))
    return "\n".join(lines)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", action="store_true", help="run the submits (what the profiler traces)")
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "levels_cost"))
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--blocks", type=int, default=48)
    ap.add_argument("--submits", type=int, default=12)
    a = ap.parse_args()
    if a.workload:
        workload(a.streams, a.blocks, a.submits)
        return 0
    os.makedirs(a.out, exist_ok=True)
    cmd = ["timeout", "-k", "10", str(TIME_LIMIT), "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", a.out,
           "-o", "levels_cost", "--", sys.executable, os.path.abspath(__file__), "--workload", "--streams", str(a.streams),
           "--blocks", str(a.blocks), "--submits", str(a.submits)]
    child = subprocess.run(cmd, check=True, capture_output=True, text=True)
    periods = [ln for ln in child.stdout.splitlines() if ln.startswith("levels_cost period")]
    text = report(a.out, a.streams, a.blocks, a.submits) + "\n" + "\n".join(periods)
    print(text)
    with open(os.path.join(a.out, "levels_cost.txt"), "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
