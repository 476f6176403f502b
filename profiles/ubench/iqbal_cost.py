"""Cost of the IQ balancer: kernel times of its three kernels -- csrc/correct.h's instantiations with the balancer,
printed under the names they had as kernels of their own: iq_sums_kernel, iq_estimate_kernel and iq_apply_kernel -- on 1 and 64 input
rows of 48 blocks, u8 at 1/1 and s16 at 25/16 -- and, in the same run and on the same rows, of the DC blocker's three kernels
(dc_cost.py), which they replace on a balancer context: the yardstick.  The floor is the blocker's: the row is read twice in its
stored format (once for the sums, once to be corrected) and 4 bytes per complex sample are written and, by the pre-stage behind
them, read again -- at the 8 TB/s HBM peak.  The estimate kernels are one wave per row and move next to nothing: latency, not traffic.

    python profiles/ubench/iqbal_cost.py [--out DIR] [--blocks 48] [--submits 4]

starts `rocprofv3 --kernel-trace --stats -- python iqbal_cost.py --workload ...` as a child process under a time limit (a kernel trace
in a run of its own, nothing else traced), reads the kernel trace it wrote and prints, per context, the median and the range of the
timed launches of each kernel.  The first two submits of each context are warm-up and are left out.  The input is near-silence with
a little noise on both rails, so that the demodulator chains beside the pre-stages are idle and no guard of the balancer trips.  A
record, not a gate.
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

from dc_cost import launches  # noqa: E402
from resample_cost import HBM_PEAK, WARMUP, durations  # noqa: E402

TIME_LIMIT = 600  # seconds, for the traced child
CONTEXTS = (("u8", 1, 1, 2), ("s16", 25, 16, 4))  # format, P, Q, bytes per complex sample
ROWS = (1, 64)
K = 2048
FAMILIES = (("dc", ("dc_sums_kernel", "dc_estimate_kernel", "dc_apply_kernel")), ("iq", ("iq_sums_kernel", "iq_estimate_kernel", "iq_apply_kernel")))


def workload(n_blocks: int, submits: int) -> None:
    import torch

    from tfrec_amd import api

    for fmt, p, q, bps in CONTEXTS:
        for rows in ROWS:
            iq = None
            for kw in (dict(dc_windows=K), dict(dc_windows=K, iq_windows=K)):  # the blocker alone, then the balancer behind it
                with api.Receiver(rows, 0x2F, 500, 0, max_blocks=n_blocks, input_format=fmt, input_rate=(p, q), **kw) as r:
                    n = r.input_bytes(n_blocks)
                    if iq is None and fmt == "u8":
                        iq = torch.randint(124, 133, (rows, n), dtype=torch.uint8, device="cuda:0")
                    elif iq is None:
                        iq = torch.randint(-300, 300, (rows, n // 2), dtype=torch.int16, device="cuda:0").view(torch.uint8)
                    torch.cuda.synchronize()
                    for _ in range(WARMUP + submits):
                        r.submit(iq, n_blocks)
                        r.read_dc(0)
                        r.drain()
                    r.sync()
            del iq


def report(trace_dir: str, n_blocks: int, submits: int) -> str:
    d = durations(trace_dir)
    per_kernel = launches(d, [name for _, names in FAMILIES for name in names])
    lines = ["iqbal_cost: %d blocks per row and submit, K = %d, %d timed submits per context after %d warm-up submits"
             % (n_blocks, K, submits, WARMUP)]
    per = WARMUP + submits
    i = 0
    for fmt, p, q, bps in CONTEXTS:  # the contexts launch in this order; a kernel's instantiations sort by format, as CONTEXTS does
        for rows in ROWS:
            n_in = n_blocks * 32768 * p // q
            floor = 1e6 * rows * n_in * (2 * bps + 4 + 4) / HBM_PEAK
            totals, parts = [], []
            for family, names in FAMILIES:  # (each family runs in one of the two receivers of the context: the same index)
                total = 0.0
                for name in names:
                    t = per_kernel[name][i * per:(i + 1) * per][WARMUP:]
                    if not t:
                        parts.append("%s: no launches found" % name)
                        continue
                    med = statistics.median(t)
                    total += med
                    parts.append("%-18s median %8.2f us  range %8.2f .. %8.2f us (%d launches)" % (name, med / 1e3, min(t) / 1e3, max(t) / 1e3, len(t)))
                totals.append(total)
            i += 1
            lines.append("%-3s %2d/%-2d %2d rows, %7d samples per row: the balancer's three kernels %8.2f us, the blocker's %8.2f us; floor %7.2f us "
                         "(%d B per sample read twice, 4 B written and read again, at 8 TB/s)"
                         % (fmt, p, q, rows, n_in, totals[1] / 1e3, totals[0] / 1e3, floor, bps))
            lines.extend("    " + s for s in parts)
    return "\n".join(lines)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", action="store_true", help="run the submits (what the profiler traces)")
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "iqbal_cost"))
    ap.add_argument("--blocks", type=int, default=48)
    ap.add_argument("--submits", type=int, default=4)
    a = ap.parse_args()
    if a.workload:
        workload(a.blocks, a.submits)
        return 0
    os.makedirs(a.out, exist_ok=True)
    cmd = ["timeout", "-k", "10", str(TIME_LIMIT), "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", a.out,
           "-o", "iqbal_cost", "--", sys.executable, os.path.abspath(__file__), "--workload", "--blocks", str(a.blocks),
           "--submits", str(a.submits)]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    text = report(a.out, a.blocks, a.submits)
    print(text)
    with open(os.path.join(a.out, "iqbal_cost.txt"), "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
