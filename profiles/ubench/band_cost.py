"""Cost of the burst band: kernel time of band_list_kernel and band_product_kernel beside clock_accum_kernel's and
keying_product_kernel's in the same submits of one context with the three stages on.

    python profiles/ubench/band_cost.py [--out DIR] [--streams 1024] [--blocks 48] [--submits 12] [--bursts 6]

starts `rocprofv3 --kernel-trace --stats -- python band_cost.py --workload ...` as a child process under a time limit (a kernel
trace in a run of its own, nothing else traced), reads the kernel trace it wrote and prints, per kernel, the median and the range of
the launches.  The input is the recorder's cost input as clock_cost.py makes it: near-silence with `--bursts` stretches of 2000 raw
samples of full-scale noise per block, at the same places in every stream.  A run of 500 decimated samples and the trigger's hold
holds one or two 512-sample segments and no 4096-sample one, so keying_product_kernel has an empty list here (keying_cost.py uses
longer stretches for it).  Useful work: band_product_kernel 524288 multiply-adds (256 bins, 512 samples, two components of two
terms) per counted segment, the plane factor of 4 not counted; clock_accum_kernel 262144 and keying_product_kernel 1048576 per
counted segment of theirs.  The segments are counted from one more submit's records.  A record, not a gate.
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
# kernel -> (useful multiply-adds a segment, whose segments)
KERNELS = {"band_list_kernel": (0, ""), "band_product_kernel": (524288, "band"), "clock_accum_kernel": (262144, "clock"),
           "keying_product_kernel": (1048576, "keying")}


def workload(n_streams: int, n_blocks: int, submits: int, bursts: int) -> None:
    import torch

    from tfrec_amd import api

    g = torch.Generator(device="cuda:0").manual_seed(3)
    iq = torch.randint(124, 133, (n_streams, n_blocks * api.BLOCK_BYTES), dtype=torch.uint8, device="cuda:0", generator=g)
    where = torch.randint(0, api.BLOCK_BYTES - 4000, (n_blocks * bursts,), generator=torch.Generator().manual_seed(4)).tolist()
    for k, off in enumerate(where):  # (clock_cost.py's input: the same places in every stream)
        a = (k // bursts) * api.BLOCK_BYTES + off
        iq[:, a:a + 4000] = torch.randint(0, 256, (n_streams, 4000), dtype=torch.uint8, device="cuda:0", generator=g)
    torch.cuda.synchronize()
    max_runs = n_streams * (n_blocks * api.BLOCK_DEC // 356 + 3)
    with api.Receiver(n_streams, 0x2F, 500, 0, max_blocks=n_blocks) as r:
        r.enable_capture(max_runs, 1)  # the table alone: a pool of one pair
        r.enable_burst_clock()
        r.enable_burst_keying()
        r.enable_burst_band()
        for _ in range(WARMUP + submits):
            r.submit(iq, n_blocks)
            r.drain()
        r.submit(iq, n_blocks)  # one more, for its records: the segments the kernels transformed
        recs = {"band": r.read_burst_bands(), "keying": r.read_burst_keyings(), "clock": r.read_burst_clocks()}
        r.drain()
        print("band_cost totals: %d runs per submit; segments (silent): %s" % (len(recs["band"]), " ".join(
            "%s %d (%d)" % (k, int(v["n_segments"].sum()), int(v["n_silent"].sum())) for k, v in recs.items())), flush=True)


def report(trace_dir: str, a, segments: dict) -> str:
    d = durations(trace_dir)
    lines = ["band_cost: %d streams x %d blocks per submit, %d stretches of 2000 raw samples per block, %d submits after %d warm-up submits" % (
        a.streams, a.blocks, a.bursts, a.submits, WARMUP)]
    for kernel, (macs, whose) in KERNELS.items():
        t = sum((d[k] for k in sorted(d) if kernel in k), [])
        if not t:
            lines.append("%-24s no launches found" % kernel)
            continue
        med = statistics.median(t)
        lines.append("%-24s median %8.3f ms  range %8.3f .. %8.3f ms  (%d launches, warm-up included)" % (
            kernel, med / 1e6, min(t) / 1e6, max(t) / 1e6, len(t)))
        if macs:
            n = segments.get(whose, 0)
            lines.append("%-24s %d segments, %.2f G useful multiply-adds per submit: %.2f T per second" % (
                "", n, n * macs / 1e9, n * macs / (med / 1e9) / 1e12))
    return "\n".join(lines)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", action="store_true", help="run the submits (what the profiler traces)")
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "band_cost"))
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
           "-o", "band_cost", "--", sys.executable, os.path.abspath(__file__), "--workload", "--streams", str(a.streams),
           "--blocks", str(a.blocks), "--submits", str(a.submits), "--bursts", str(a.bursts)]
    child = subprocess.run(cmd, check=True, capture_output=True, text=True)
    info = [ln for ln in child.stdout.splitlines() if ln.startswith("band_cost ")]
    segments = {}
    for ln in info:
        if ln.startswith("band_cost totals:"):
            w = ln.split("segments (silent):")[1].split()  # band N (S) keying N (S) clock N (S)
            segments = {w[i]: int(w[i + 1]) for i in range(0, len(w), 3)}
    text = report(a.out, a, segments) + "\n" + "\n".join(info)
    print(text)
    with open(os.path.join(a.out, "band_cost.txt"), "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
