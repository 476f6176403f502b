"""Cost of the envelope clock: kernel time of keying_list_kernel and keying_product_kernel beside clock_accum_kernel's
in the same submits of one context with both stages on.

    python profiles/ubench/keying_cost.py [--out DIR] [--streams 1024] [--blocks 48] [--submits 12] [--raw 44000]

starts `rocprofv3 --kernel-trace --stats -- python keying_cost.py --workload ...` as a child process under a time limit (a kernel
trace in a run of its own, nothing else traced), reads the kernel trace it wrote and prints, per kernel, the median and the range of
the launches.  The input is the recorder's cost input (clock_cost.py's: near-silence with stretches of full-scale noise at the same
places in every stream) with ONE stretch of `--raw` raw samples per two blocks instead of six of 2000 per block: a run of 500 decimated samples holds
no 4096-sample segment, so on the six short stretches this stage would have nothing to do.  Useful work: keying_product_kernel
1048576 multiply-adds (128 bins, 4096 samples, two components) per counted segment, the plane factor of 4 not counted;
clock_accum_kernel 262144 per counted segment.  The segments are counted from one more submit's records.  A record, not a gate.
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

TIME_LIMIT = 600  # seconds, for the traced child
KERNELS = {"keying_list_kernel": 0, "keying_product_kernel": 1048576, "clock_accum_kernel": 262144}  # useful multiply-adds a segment


def workload(n_streams: int, n_blocks: int, submits: int, raw: int) -> None:
    import torch

    from tfrec_amd import api

    g = torch.Generator(device="cuda:0").manual_seed(3)
    iq = torch.randint(124, 133, (n_streams, n_blocks * api.BLOCK_BYTES), dtype=torch.uint8, device="cuda:0", generator=g)
    where = torch.randint(0, 2 * api.BLOCK_BYTES - 2 * raw, (n_blocks // 2,), generator=torch.Generator().manual_seed(4)).tolist()
    for k, off in enumerate(where):
        a = 2 * (k * api.BLOCK_BYTES + off // 2)
        iq[:, a:a + 2 * raw] = torch.randint(0, 256, (n_streams, 2 * raw), dtype=torch.uint8, device="cuda:0", generator=g)
    torch.cuda.synchronize()
    max_runs = n_streams * (n_blocks * api.BLOCK_DEC // 356 + 3)
    with api.Receiver(n_streams, 0x2F, 500, 0, max_blocks=n_blocks) as r:
        r.enable_capture(max_runs, 1)  # the table alone: a pool of one pair
        r.enable_burst_clock()
        r.enable_burst_keying()
        for _ in range(WARMUP + submits):
            r.submit(iq, n_blocks)
            r.drain()
        r.submit(iq, n_blocks)  # one more, for its records: the segments the kernels transformed
        key, clk = r.read_burst_keyings(), r.read_burst_clocks()
        r.drain()
        print("keying_cost totals: %d runs per submit; keying %d segments (%d silent), clock %d segments (%d silent)" % (
            len(key), int(key["n_segments"].sum()), int(key["n_silent"].sum()), int(clk["n_segments"].sum()), int(clk["n_silent"].sum())),
            flush=True)


def report(trace_dir: str, a, segments: dict) -> str:
    d = durations(trace_dir)
    lines = ["keying_cost: %d streams x %d blocks per submit, one stretch of %d raw samples per two blocks, %d submits after %d warm-up submits" % (
        a.streams, a.blocks, a.raw, a.submits, WARMUP)]
    for kernel, macs in KERNELS.items():
        t = sum((d[k] for k in sorted(d) if kernel in k), [])
        if not t:
            lines.append("%-24s no launches found" % kernel)
            continue
        med = statistics.median(t)
        lines.append("%-24s median %8.3f ms  range %8.3f .. %8.3f ms  (%d launches, warm-up included)" % (
            kernel, med / 1e6, min(t) / 1e6, max(t) / 1e6, len(t)))
        if macs:
            n = segments["clock" if kernel.startswith("clock") else "keying"]
            lines.append("%-24s %d segments, %.2f G useful multiply-adds per submit: %.2f T per second" % (
                "", n, n * macs / 1e9, n * macs / (med / 1e9) / 1e12))
    return "\n".join(lines)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", action="store_true", help="run the submits (what the profiler traces)")
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "keying_cost"))
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--blocks", type=int, default=48)
    ap.add_argument("--submits", type=int, default=12)
    ap.add_argument("--raw", type=int, default=44000)
    a = ap.parse_args()
    if a.workload:
        workload(a.streams, a.blocks, a.submits, a.raw)
        return 0
    os.makedirs(a.out, exist_ok=True)
    cmd = ["timeout", "-k", "10", str(TIME_LIMIT), "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", a.out,
           "-o", "keying_cost", "--", sys.executable, os.path.abspath(__file__), "--workload", "--streams", str(a.streams),
           "--blocks", str(a.blocks), "--submits", str(a.submits), "--raw", str(a.raw)]
    child = subprocess.run(cmd, check=True, capture_output=True, text=True)
    info = [ln for ln in child.stdout.splitlines() if ln.startswith("keying_cost ")]
    segments = {"keying": 0, "clock": 0}
    for ln in info:
        if ln.startswith("keying_cost totals:"):
            w = ln.split()
            segments = {"keying": int(w[7]), "clock": int(w[12])}
    text = report(a.out, a, segments) + "\n" + "\n".join(info)
    print(text)
    with open(os.path.join(a.out, "keying_cost.txt"), "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
