"""Cost of the burst correlator: kernel time of corr_soft_kernel, corr_list_kernel, corr_product_kernel and
corr_carry_kernel beside capture_copy_kernel's -- one read of the captured pairs -- in the same submits of one context.

    python profiles/ubench/corr_cost.py [--out DIR] [--streams 1024] [--blocks 48] [--submits 12] [--bursts 6]

starts `rocprofv3 --kernel-trace --stats -- python corr_cost.py --workload ...` as a child process under a time limit (a kernel
trace in a run of its own, nothing else traced), reads the kernel trace it wrote and prints, per kernel, the median and the range of
the launches.  The input is the recorder's cost input as clock_cost.py makes it: near-silence with `--bursts` stretches of 2000 raw
samples of full-scale noise per block, at the same places in every stream.  The bank is the golden table's: 2dd4 at 17240, 9600,
8842, 38400 and 6000 bit/s and aa2dd4 at 17240, Kp = 1024.  Useful work of corr_product_kernel, counted from one more submit's
records: unpadded, K_t multiply-adds per defined position of template t; padded, 16 Kp per sample of a run (what the instruction
does, undefined and masked positions and the zero taps included).  A record, not a gate.
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
BANK = [(0x2DD4, 16, 17240), (0x2DD4, 16, 9600), (0x2DD4, 16, 8842), (0xAA2DD4, 24, 17240), (0x2DD4, 16, 38400), (0x2DD4, 16, 6000)]
KERNELS = ("capture_copy_kernel", "corr_soft_kernel", "corr_list_kernel", "corr_product_kernel", "corr_carry_kernel")


def workload(n_streams: int, n_blocks: int, submits: int, bursts: int) -> None:
    import torch

    from tfrec_amd import api, corr

    g = torch.Generator(device="cuda:0").manual_seed(3)
    iq = torch.randint(124, 133, (n_streams, n_blocks * api.BLOCK_BYTES), dtype=torch.uint8, device="cuda:0", generator=g)
    where = torch.randint(0, api.BLOCK_BYTES - 4000, (n_blocks * bursts,), generator=torch.Generator().manual_seed(4)).tolist()
    for k, off in enumerate(where):  # (clock_cost.py's input: the same places in every stream)
        a = (k // bursts) * api.BLOCK_BYTES + off
        iq[:, a:a + 4000] = torch.randint(0, 256, (n_streams, 4000), dtype=torch.uint8, device="cuda:0", generator=g)
    torch.cuda.synchronize()
    st = corr.Settings(BANK)
    max_runs = n_streams * (n_blocks * api.BLOCK_DEC // 356 + 3)
    with api.Receiver(n_streams, 0x2F, 500, 0, max_blocks=n_blocks) as r:
        r.enable_capture(max_runs, n_streams * n_blocks * api.BLOCK_DEC)  # a pool for every sample, as -y's
        r.enable_burst_corr(BANK)
        for _ in range(WARMUP + submits):
            r.submit(iq, n_blocks)
            r.drain()
        r.submit(iq, n_blocks)  # one more, for its records: the positions the kernel scored
        recs = r.read_burst_corrs()
        r.drain()
        samples = int(recs["n_samples"].astype("int64").sum())
        unpadded = sum(int(recs["t"]["n_pos"][:, t].astype("int64").sum()) * k for t, k in enumerate(st.K))
        print("corr_cost totals: %d runs per submit, %d samples, %d tiles; multiply-adds unpadded %d padded %d" % (
            len(recs), samples, int(((recs["n_samples"].astype("int64") + 255) // 256).sum()), unpadded, 16 * st.Kp * samples), flush=True)


def report(trace_dir: str, a, macs: dict) -> str:
    d = durations(trace_dir)
    lines = ["corr_cost: %d streams x %d blocks per submit, %d stretches of 2000 raw samples per block, %d submits after %d warm-up submits" % (
        a.streams, a.blocks, a.bursts, a.submits, WARMUP)]
    med = {}
    for kernel in KERNELS:
        t = sum((d[k] for k in sorted(d) if kernel in k), [])
        if not t:
            lines.append("%-24s no launches found" % kernel)
            continue
        med[kernel] = statistics.median(t)
        lines.append("%-24s median %8.3f ms  range %8.3f .. %8.3f ms  (%d launches, warm-up included)" % (
            kernel, med[kernel] / 1e6, min(t) / 1e6, max(t) / 1e6, len(t)))
    if "corr_product_kernel" in med:
        for name, n in macs.items():
            lines.append("%-24s %s: %.2f G multiply-adds per submit, %.2f T per second" % (
                "", name, n / 1e9, n / (med["corr_product_kernel"] / 1e9) / 1e12))
    if "corr_soft_kernel" in med and "capture_copy_kernel" in med:
        lines.append("%-24s corr_soft_kernel takes %.2f times capture_copy_kernel, one read of the captured pairs" % (
            "", med["corr_soft_kernel"] / med["capture_copy_kernel"]))
    return "\n".join(lines)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", action="store_true", help="run the submits (what the profiler traces)")
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "corr_cost"))
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
           "-o", "corr_cost", "--", sys.executable, os.path.abspath(__file__), "--workload", "--streams", str(a.streams),
           "--blocks", str(a.blocks), "--submits", str(a.submits), "--bursts", str(a.bursts)]
    child = subprocess.run(cmd, check=True, capture_output=True, text=True)
    info = [ln for ln in child.stdout.splitlines() if ln.startswith("corr_cost ")]
    macs = {}
    for ln in info:
        if ln.startswith("corr_cost totals:"):
            w = ln.split("multiply-adds")[1].split()  # unpadded N padded N
            macs = {w[0]: int(w[1]), w[2]: int(w[3])}
    text = report(a.out, a, macs) + "\n" + "\n".join(info)
    print(text)
    with open(os.path.join(a.out, "corr_cost.txt"), "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
