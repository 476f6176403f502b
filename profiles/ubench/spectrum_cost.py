"""Cost of the power spectrum: kernel time of spectrum_kernel at N = 256, one input row and 64 input rows of 48 blocks
each, next to its two floors -- every complex input sample read once (2 bytes at the 8 TB/s HBM peak), and 4 N real multiply-adds
per complex sample, which the kernel issues as 2 N v_dot2_i32_i16 per sample (256 CUs x 4 SIMDs x 16 lanes at 2.4 GHz).

    python profiles/ubench/spectrum_cost.py [--out DIR] [--bins 256] [--blocks 48] [--submits 8]

starts `rocprofv3 --kernel-trace --stats -- python spectrum_cost.py --workload ...` as a child process under a time limit (a kernel
trace in a run of its own, nothing else traced), reads the kernel trace it wrote and prints, per row count, the median and the
range of the timed launches.  The first two submits of each context are warm-up and are left out.  The input is near-silence:
nothing triggers, so the demodulator chains beside the spectrum are idle and the kernel is timed alone (beside a busy pipeline it
runs at low priority and stretches).  It also prints the wall-clock period per submit of each context with and without the
spectrum, for information.  A record, not a gate.
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
ROWS = (1, 64)
LANE_RATE = 256 * 4 * 16 * 2.4e9  # vector lane-instructions per second of the whole chip


def workload(n_bins: int, n_blocks: int, submits: int) -> None:
    import torch

    from tfrec_amd import api

    for rows in ROWS:
        iq = torch.randint(124, 133, (rows, n_blocks * api.BLOCK_BYTES), dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        for enabled in (True, False):
            with api.Receiver(rows, 0x2F, 500, 0, max_blocks=n_blocks) as r:
                if enabled:
                    r.enable_spectrum(n_bins, max(1, api.BLOCK_BYTES // 2 // n_bins))
                t0 = 0.0
                for k in range(WARMUP + submits):
                    if k == WARMUP:
                        r.sync()
                        t0 = time.perf_counter()
                    r.submit(iq, n_blocks)
                    if enabled:
                        r.read_spectrum(0)
                    r.drain()
                r.sync()
                print("spectrum_cost period: %d rows, %s context %.3f ms per submit (submit, %sdrain; quiet input, %d submits)"
                      % (rows, "spectrum" if enabled else "plain", 1e3 * (time.perf_counter() - t0) / submits,
                         "read_spectrum, " if enabled else "", submits), flush=True)
        del iq


def report(trace_dir: str, n_bins: int, n_blocks: int, submits: int) -> str:
    d = durations(trace_dir)
    t = sum((d[k] for k in sorted(d) if "spectrum_kernel" in k), [])
    lines = ["spectrum_cost: N = %d, %d blocks per submit, %d timed submits per context after %d warm-up submits"
             % (n_bins, n_blocks, submits, WARMUP)]
    per = WARMUP + submits
    for i, rows in enumerate(ROWS):  # the contexts launch in this order
        mine = t[i * per:(i + 1) * per][WARMUP:]
        if not mine:
            lines.append("%3d rows: no launches found" % rows)
            continue
        samples = rows * n_blocks * 32768
        med = statistics.median(mine)
        lines.append("%3d rows: median %8.3f ms  range %8.3f .. %8.3f ms  (%d launches)  %.1f M complex samples  floor %.4f ms reading "
                     "(2 B per sample at 8 TB/s), %.4f ms arithmetic (2 N dot2 per sample)  %.2f ns per sample"
                     % (rows, med / 1e6, min(mine) / 1e6, max(mine) / 1e6, len(mine), samples / 1e6, 1e3 * samples * 2 / HBM_PEAK,
                        1e3 * samples * 2 * n_bins / LANE_RATE, med / samples))
    return "\n".join(lines)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", action="store_true", help="run the submits (what the profiler traces)")
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "spectrum_cost"))
    ap.add_argument("--bins", type=int, default=256)
    ap.add_argument("--blocks", type=int, default=48)
    ap.add_argument("--submits", type=int, default=8)
    a = ap.parse_args()
    if a.workload:
        workload(a.bins, a.blocks, a.submits)
        return 0
    os.makedirs(a.out, exist_ok=True)
    cmd = ["timeout", "-k", "10", str(TIME_LIMIT), "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", a.out,
           "-o", "spectrum_cost", "--", sys.executable, os.path.abspath(__file__), "--workload", "--bins", str(a.bins),
           "--blocks", str(a.blocks), "--submits", str(a.submits)]
    child = subprocess.run(cmd, check=True, capture_output=True, text=True)
    periods = [ln for ln in child.stdout.splitlines() if ln.startswith("spectrum_cost period")]
    text = report(a.out, a.bins, a.blocks, a.submits) + "\n" + "\n".join(periods)
    print(text)
    with open(os.path.join(a.out, "spectrum_cost.txt"), "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
