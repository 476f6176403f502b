"""Cost of the burst demodulator: kernel time of its corr_soft_kernel launch, demod_list_kernel, demod_timing_kernel,
demod_symbol_kernel and demod_carry_kernel beside capture_copy_kernel's -- one read of the captured pairs -- in the same submits of
one context.

    python profiles/ubench/demod_cost.py [--out DIR] [--streams 1024] [--blocks 48] [--submits 12] [--bursts 6] [--rate 17240] [--code nrz]

starts `rocprofv3 --kernel-trace --stats -- python demod_cost.py --workload ...` as a child process under a time limit (a kernel
trace in a run of its own, nothing else traced), reads the kernel trace it wrote and prints, per kernel, the median and the range of
the launches.  The input is the recorder's cost input as clock_cost.py makes it: near-silence with `--bursts` stretches of 2000 raw
samples of full-scale noise per block, at the same places in every stream.  From one more submit's records: the runs, their
samples, the decisions written and the runs timed.  A record, not a gate.
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
KERNELS = ("capture_copy_kernel", "corr_soft_kernel", "demod_list_kernel", "demod_timing_kernel", "demod_symbol_kernel", "demod_carry_kernel")


def workload(n_streams: int, n_blocks: int, submits: int, bursts: int, rate: int, code: str) -> None:
    import torch

    from tfrec_amd import api, demod

    g = torch.Generator(device="cuda:0").manual_seed(3)
    iq = torch.randint(124, 133, (n_streams, n_blocks * api.BLOCK_BYTES), dtype=torch.uint8, device="cuda:0", generator=g)
    where = torch.randint(0, api.BLOCK_BYTES - 4000, (n_blocks * bursts,), generator=torch.Generator().manual_seed(4)).tolist()
    for k, off in enumerate(where):  # (clock_cost.py's input: the same places in every stream)
        a = (k // bursts) * api.BLOCK_BYTES + off
        iq[:, a:a + 4000] = torch.randint(0, 256, (n_streams, 4000), dtype=torch.uint8, device="cuda:0", generator=g)
    torch.cuda.synchronize()
    max_runs = n_streams * (n_blocks * api.BLOCK_DEC // 356 + 3)
    with api.Receiver(n_streams, 0x2F, 500, 0, max_blocks=n_blocks) as r:
        r.enable_capture(max_runs, n_streams * n_blocks * api.BLOCK_DEC)  # a pool for every sample, as -w's
        r.enable_burst_demod(rate, code)
        for _ in range(WARMUP + submits):
            r.submit(iq, n_blocks)
            r.drain()
        r.submit(iq, n_blocks)  # one more, for its records
        recs, _ = r.read_burst_demods()
        r.drain()
        print("demod_cost totals: %d runs per submit, %d samples, %d tiles, %d decisions, %d runs timed and %d flagged" % (
            len(recs), int(recs["n_samples"].astype("int64").sum()), int(((recs["n_samples"].astype("int64") + 4095) // 4096).sum()),
            int(recs["n_symbols"].astype("int64").sum()), int((recs["timing"] == demod.MEASURED).sum()),
            int((recs["timing"] == demod.FLAGGED).sum())), flush=True)


def report(trace_dir: str, a) -> str:
    d = durations(trace_dir)
    lines = ["demod_cost: %d streams x %d blocks per submit, %d stretches of 2000 raw samples per block, %d bit/s %s, %d submits after %d warm-up submits" % (
        a.streams, a.blocks, a.bursts, a.rate, a.code, a.submits, WARMUP)]
    med = {}
    for kernel in KERNELS:
        t = sum((d[k] for k in sorted(d) if kernel in k), [])
        if not t:
            lines.append("%-24s no launches found" % kernel)
            continue
        med[kernel] = statistics.median(t)
        lines.append("%-24s median %8.3f ms  range %8.3f .. %8.3f ms  (%d launches, warm-up included)" % (
            kernel, med[kernel] / 1e6, min(t) / 1e6, max(t) / 1e6, len(t)))
    if "demod_symbol_kernel" in med and "capture_copy_kernel" in med:
        lines.append("%-24s demod_symbol_kernel takes %.2f times capture_copy_kernel, one read of the captured pairs" % (
            "", med["demod_symbol_kernel"] / med["capture_copy_kernel"]))
    return "\n".join(lines)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", action="store_true", help="run the submits (what the profiler traces)")
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "demod_cost"))
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--blocks", type=int, default=48)
    ap.add_argument("--submits", type=int, default=12)
    ap.add_argument("--bursts", type=int, default=6)
    ap.add_argument("--rate", type=int, default=17240)
    ap.add_argument("--code", default="nrz")
    a = ap.parse_args()
    if a.workload:
        workload(a.streams, a.blocks, a.submits, a.bursts, a.rate, a.code)
        return 0
    os.makedirs(a.out, exist_ok=True)
    cmd = ["timeout", "-k", "10", str(TIME_LIMIT), "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", a.out,
           "-o", "demod_cost", "--", sys.executable, os.path.abspath(__file__), "--workload", "--streams", str(a.streams),
           "--blocks", str(a.blocks), "--submits", str(a.submits), "--bursts", str(a.bursts), "--rate", str(a.rate), "--code", a.code]
    child = subprocess.run(cmd, check=True, capture_output=True, text=True)
    info = [ln for ln in child.stdout.splitlines() if ln.startswith("demod_cost ")]
    text = report(a.out, a) + "\n" + "\n".join(info)
    print(text)
    with open(os.path.join(a.out, "demod_cost.txt"), "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
