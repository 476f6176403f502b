"""Cost of the occupancy detector: kernel time of occupancy_kernel at N = 256 and N = 1024, on one input row and on
64 input rows of 48 blocks each, next to its floor -- every spectrum record read once (16 N bytes) and 16 + N / 8 bytes written, at
the 8 TB/s HBM peak -- and to the work of its selection, N^2 64-bit compares per record.  The record is the frames of one block's
input, as tfrec_gpu -A takes it: 48 records per row and submit.

    python profiles/ubench/occupancy_cost.py [--out DIR] [--blocks 48] [--submits 4]

starts `rocprofv3 --kernel-trace --stats -- python occupancy_cost.py --workload ...` as a child process under a time limit (a kernel
trace in a run of its own, nothing else traced), reads the kernel trace it wrote and prints, per N and row count, the median and the
range of the timed launches of occupancy_kernel and, beside it, of spectrum_kernel, whose records it reads.  The first two submits of
each context are warm-up and are left out.  The detector's work does not depend on the data; the input is near-silence, so that the
demodulator chains beside it are idle.  A record, not a gate.
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

from resample_cost import HBM_PEAK, WARMUP, durations  # noqa: E402

TIME_LIMIT = 600  # seconds, for the traced child
BINS = (256, 1024)
ROWS = (1, 64)


def workload(n_blocks: int, submits: int) -> None:
    import torch

    from tfrec_amd import api

    for n_bins in BINS:
        for rows in ROWS:
            iq = torch.randint(124, 133, (rows, n_blocks * api.BLOCK_BYTES), dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            with api.Receiver(rows, 0x2F, 500, 0, max_blocks=n_blocks) as r:
                r.enable_spectrum(n_bins, max(1, api.BLOCK_BYTES // 2 // n_bins))
                r.enable_occupancy()
                for _ in range(WARMUP + submits):
                    r.submit(iq, n_blocks)
                    r.read_occupancy(0)
                    r.drain()
                r.sync()
            del iq


def report(trace_dir: str, n_blocks: int, submits: int) -> str:
    d = durations(trace_dir)
    occ = sum((d[k] for k in sorted(d) if "occupancy_kernel" in k), [])
    spec = sum((d[k] for k in sorted(d) if "spectrum_kernel" in k), [])
    lines = ["occupancy_cost: %d blocks (= records) per row and submit, %d timed submits per context after %d warm-up submits"
             % (n_blocks, submits, WARMUP)]
    per = WARMUP + submits
    i = 0
    for n_bins in BINS:  # the contexts launch in this order
        for rows in ROWS:
            mine, theirs = occ[i * per:(i + 1) * per][WARMUP:], spec[i * per:(i + 1) * per][WARMUP:]
            i += 1
            if not mine or not theirs:
                lines.append("N %4d, %2d rows: no launches found" % (n_bins, rows))
                continue
            records = rows * n_blocks
            med = statistics.median(mine)
            lines.append("N %4d, %2d rows: occupancy_kernel median %8.2f us  range %8.2f .. %8.2f us  (%d launches)  %d records, %.2f us "
                         "per record; floor %.3f us (16 N + 16 + N / 8 bytes per record at 8 TB/s); %.1f M compares; spectrum_kernel "
                         "beside it: median %.3f ms"
                         % (n_bins, rows, med / 1e3, min(mine) / 1e3, max(mine) / 1e3, len(mine), records, med / 1e3 / records,
                            1e6 * records * (16 * n_bins + 16 + n_bins // 8) / HBM_PEAK, records * n_bins * n_bins / 1e6,
                            statistics.median(theirs) / 1e6))
    return "\n".join(lines)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", action="store_true", help="run the submits (what the profiler traces)")
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "occupancy_cost"))
    ap.add_argument("--blocks", type=int, default=48)
    ap.add_argument("--submits", type=int, default=4)
    a = ap.parse_args()
    if a.workload:
        workload(a.blocks, a.submits)
        return 0
    os.makedirs(a.out, exist_ok=True)
    cmd = ["timeout", "-k", "10", str(TIME_LIMIT), "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", a.out,
           "-o", "occupancy_cost", "--", sys.executable, os.path.abspath(__file__), "--workload", "--blocks", str(a.blocks),
           "--submits", str(a.submits)]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    text = report(a.out, a.blocks, a.submits)
    print(text)
    with open(os.path.join(a.out, "occupancy_cost.txt"), "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
