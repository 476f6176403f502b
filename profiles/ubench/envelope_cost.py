"""Cost of the burst envelope: kernel time of run_records_init_kernel<tfrec_amd_envelope>, envelope_mask_kernel (pass A) and
envelope_accum_kernel (pass B), and the period per submit of a context with the envelope against one with the burst meter, one with the
recorder's table alone and a plain one, on the same input in the same session.

    python profiles/ubench/envelope_cost.py [--out DIR] [--streams 1024] [--blocks 48] [--submits 12] [--bursts 6]

starts `rocprofv3 --kernel-trace --stats -- python envelope_cost.py --workload ...` as a child process under a time limit (a kernel
trace in a run of its own, nothing else traced), reads the kernel trace it wrote and prints, per kernel, the median and the range of
the timed launches.  The first two submits of every context are warm-up and are left out.  The input is burst_cost.py's
(capture_cost.py's): near-silence with `--bursts` stretches of full-scale noise, 2000 raw samples each, per stream and block; the
captured share is what the run reports, not a property of the benchmark's input.  Pass B's floor is the captured pairs read once (4 B
each), pass A's the mask read once (1 bit per sample).  A record, not a gate.
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
KERNELS = ("run_records_init_kernel<tfrec_amd_envelope>", "envelope_mask_kernel", "envelope_accum_kernel", "burst_accum_kernel", "capture_copy_kernel")
KINDS = ("envelope", "meter", "table", "plain")


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
    max_runs = n_streams * (n_blocks * api.BLOCK_DEC // 356 + 3)
    for kind in KINDS:
        with api.Receiver(n_streams, 0x2F, 500, 0, max_blocks=n_blocks) as r:
            if kind != "plain":
                r.enable_capture(max_runs, 1)  # the table alone: a pool of one pair
            if kind == "meter":
                r.enable_burst_meter()
            if kind == "envelope":
                r.enable_burst_envelope()
            t0 = 0.0
            nr, npairs = api.C.c_uint32(0), api.C.c_uint64(0)
            for k in range(WARMUP + submits):
                if k == WARMUP:
                    r.sync()
                    t0 = time.perf_counter()
                r.submit(iq, n_blocks)
                if kind != "plain":  # the counts; the records stay on the device (their copy is the caller's choice)
                    r.L.tfrec_amd_read_captures(r.h, None, 0, api.C.byref(nr), None, 0, api.C.byref(npairs))
                r.drain()
            r.sync()
            print("envelope_cost period: %s context %.3f ms per submit (submit, %sdrain; %d submits)"
                  % (kind, 1e3 * (time.perf_counter() - t0) / submits, "" if kind == "plain" else "the counts, ", submits), flush=True)
            if kind == "envelope":
                print("envelope_cost totals: %d runs, %d pairs of %d samples per submit (captured share %.4f)"
                      % (nr.value, npairs.value, samples, npairs.value / samples), flush=True)


def report(trace_dir: str, n_streams: int, n_blocks: int, submits: int, pairs: int, samples: int) -> str:
    d = durations(trace_dir)
    lines = ["envelope_cost: %d streams x %d blocks per submit, %d timed submits per context after %d warm-up submits" % (
        n_streams, n_blocks, submits, WARMUP)]
    for kernel in KERNELS:
        t = sum((d[k] for k in sorted(d) if kernel in k), [])
        if not t:
            lines.append("%-24s no launches found" % kernel)
            continue
        med = statistics.median(t)
        lines.append("%-24s median %8.3f ms  range %8.3f .. %8.3f ms  (%d launches, warm-up included)" % (
            kernel, med / 1e6, min(t) / 1e6, max(t) / 1e6, len(t)))
    lines.append("floor of pass B (%d captured pairs read once: %.3f GB) %.3f ms at 8 TB/s" % (pairs, 4 * pairs / 1e9, 1e3 * 4 * pairs / HBM_PEAK))
    lines.append("floor of pass A (the mask of %d samples read once: %.3f GB) %.3f ms at 8 TB/s" % (
        samples, samples / 8e9, 1e3 * samples / 8 / HBM_PEAK))
    return "\n".join(lines)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", action="store_true", help="run the submits (what the profiler traces)")
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "envelope_cost"))
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
           "-o", "envelope_cost", "--", sys.executable, os.path.abspath(__file__), "--workload", "--streams", str(a.streams),
           "--blocks", str(a.blocks), "--submits", str(a.submits), "--bursts", str(a.bursts)]
    child = subprocess.run(cmd, check=True, capture_output=True, text=True)
    info = [ln for ln in child.stdout.splitlines() if ln.startswith("envelope_cost ")]
    pairs = samples = 0
    for ln in info:
        if ln.startswith("envelope_cost totals:"):
            pairs, samples = int(ln.split()[4]), int(ln.split()[7])
    text = report(a.out, a.streams, a.blocks, a.submits, pairs, samples) + "\n" + "\n".join(info)
    print(text)
    with open(os.path.join(a.out, "envelope_cost.txt"), "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
