"""Cost of the squelched recorder: kernel time of capture_scan_kernel, capture_offsets_kernel and capture_copy_kernel,
next to their floor -- the trigger mask read once (1/8 B per decimated sample) and the captured pairs read and written once (8 B
each) at the 8 TB/s HBM peak.

    python profiles/ubench/capture_cost.py [--out DIR] [--streams 1024] [--blocks 48] [--submits 12] [--bursts 6]

starts `rocprofv3 --kernel-trace --stats -- python capture_cost.py --workload ...` as a child process under a time limit (a kernel
trace in a run of its own, nothing else traced), reads the kernel trace it wrote and prints, per kernel, the median and the range of
the timed launches.  The first two submits are warm-up and are left out.  The input is near-silence with `--bursts` stretches of
full-scale noise, 2000 raw samples each, per stream and block: the captured share is what the run reports (the workload prints the
true totals of its last submit), not a property of the benchmark's input.  It also prints the wall-clock period per submit of the
recording context and of a plain one on the same input, for information.  A record, not a gate.
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
KERNELS = ("capture_scan_kernel", "capture_offsets_kernel", "capture_copy_kernel")


def workload(n_streams: int, n_blocks: int, submits: int, bursts: int) -> None:
    import torch

    from tfrec_amd import api

    g = torch.Generator(device="cuda:0").manual_seed(3)
    iq = torch.randint(124, 133, (n_streams, n_blocks * api.BLOCK_BYTES), dtype=torch.uint8, device="cuda:0", generator=g)
    where = torch.randint(0, api.BLOCK_BYTES - 4000, (n_blocks * bursts,), generator=torch.Generator().manual_seed(4)).tolist()
    for k, off in enumerate(where):  # (the same places in every stream: the share, not the pattern, is what matters here)
        a = (k // bursts) * api.BLOCK_BYTES + off
        iq[:, a:a + 4000] = torch.randint(0, 256, (n_streams, 4000), dtype=torch.uint8, device="cuda:0", generator=g)
    torch.cuda.synchronize()
    samples = n_streams * n_blocks * api.BLOCK_DEC
    for recording in (True, False):
        with api.Receiver(n_streams, 0x2F, 500, 0, max_blocks=n_blocks) as r:
            if recording:
                r.enable_capture(n_streams * (n_blocks * api.BLOCK_DEC // 356 + 3), samples)
            t0 = 0.0
            for k in range(WARMUP + submits):
                if k == WARMUP:
                    r.sync()
                    t0 = time.perf_counter()
                r.submit(iq, n_blocks)
                if recording:  # the table and the counts; the pool stays on the device (its copy is the caller's choice)
                    nr, npairs = api.C.c_uint32(0), api.C.c_uint64(0)
                    r.L.tfrec_amd_read_captures(r.h, None, 0, api.C.byref(nr), None, 0, api.C.byref(npairs))
                r.drain()
            r.sync()
            print("capture_cost period: %s context %.3f ms per submit (submit, %sdrain; %d submits)"
                  % ("recording" if recording else "plain", 1e3 * (time.perf_counter() - t0) / submits,
                     "the counts, " if recording else "", submits), flush=True)
            if recording:
                print("capture_cost totals: %d runs, %d pairs of %d samples per submit (captured share %.4f)"
                      % (nr.value, npairs.value, samples, npairs.value / samples), flush=True)


def report(trace_dir: str, n_streams: int, n_blocks: int, submits: int, pairs: int) -> str:
    d = durations(trace_dir)
    samples = n_streams * n_blocks * 8192
    floor_bytes = samples // 8 + 8 * pairs
    lines = ["capture_cost: %d streams x %d blocks per submit, %d timed submits after %d warm-up submits" % (n_streams, n_blocks, submits, WARMUP)]
    total = 0.0
    for kernel in KERNELS:
        t = sum((d[k] for k in sorted(d) if kernel in k), [])[WARMUP:]
        if not t:
            lines.append("%-24s no launches found" % kernel)
            continue
        med = statistics.median(t)
        total += med
        lines.append("%-24s median %8.3f ms  range %8.3f .. %8.3f ms  (%d launches)" % (kernel, med / 1e6, min(t) / 1e6, max(t) / 1e6, len(t)))
    lines.append("the three together: %.3f ms (sum of the medians); floor (mask read once, %d captured pairs read and written once: %.3f GB) "
                 "%.3f ms at 8 TB/s" % (total / 1e6, pairs, floor_bytes / 1e9, 1e3 * floor_bytes / HBM_PEAK))
    return "\n".join(lines)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", action="store_true", help="run the submits (what the profiler traces)")
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "capture_cost"))
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--blocks", type=int, default=48)
    ap.add_argument("--submits", type=int, default=12)
    ap.add_argument("--bursts", type=int, default=6)
    a = ap.parse_args()
    if a.workload:
        workload(a.streams, a.blocks, a.submits, a.bursts)
        return 0
    os.makedirs(a.out, exist_ok=True)
    cmd = ["timeout", "-k", "10", str(TIME_LIMIT), "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", a.out,
           "-o", "capture_cost", "--", sys.executable, os.path.abspath(__file__), "--workload", "--streams", str(a.streams),
           "--blocks", str(a.blocks), "--submits", str(a.submits), "--bursts", str(a.bursts)]
    child = subprocess.run(cmd, check=True, capture_output=True, text=True)
    info = [ln for ln in child.stdout.splitlines() if ln.startswith("capture_cost ")]
    pairs = 0
    for ln in info:
        if ln.startswith("capture_cost totals:"):
            pairs = int(ln.split()[4])
    text = report(a.out, a.streams, a.blocks, a.submits, pairs) + "\n" + "\n".join(info)
    print(text)
    with open(os.path.join(a.out, "capture_cost.txt"), "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
