"""Cost of the channel-rate front end: kernel time of decin_kernel<false> (dense rows) and decin_kernel<true> (sparse
submits) beside frontend_kernel in the same run, next to their floor -- 4 bytes read and 4 bytes written per decimated sample plus
the mask (1/8 byte) at the 8 TB/s HBM peak; the sparse kernel reads only the captured share -- and the bytes a sparse submit moves
over PCIe against a dense one.

    python profiles/ubench/decin_cost.py [--out DIR] [--streams 1024] [--blocks 48] [--submits 6] [--bursts 6]

starts `rocprofv3 --kernel-trace --stats -- python decin_cost.py --workload ...` as a child process under a time limit (a kernel
trace in a run of its own, nothing else traced), reads the kernel trace it wrote and prints, per kernel, the median and the range of
the timed launches.  The first two submits of every context are warm-up and are left out.  Three contexts, one after the other: a
u8 context with the recorder and its pre samples on capture_cost.py's input (near-silence with `--bursts` stretches of full-scale
noise per stream and block) -- its frontend_kernel is the yardstick, its last submit's capture the sparse input --; a channel-rate
context fed dense quiet rows; a channel-rate context fed that capture through tfrec_amd_submit_runs.  A record, not a gate.
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
KERNELS = ("frontend_kernel", "decin_kernel<false>", "decin_kernel<true>", "capture_pre_kernel")


def workload(n_streams: int, n_blocks: int, submits: int, bursts: int) -> None:
    import torch

    from tfrec_amd import api

    g = torch.Generator(device="cuda:0").manual_seed(3)
    iq = torch.randint(124, 133, (n_streams, n_blocks * api.BLOCK_BYTES), dtype=torch.uint8, device="cuda:0", generator=g)
    where = torch.randint(0, api.BLOCK_BYTES - 4000, (n_blocks * bursts,), generator=torch.Generator().manual_seed(4)).tolist()
    for k, off in enumerate(where):
        a = (k // bursts) * api.BLOCK_BYTES + off
        iq[:, a:a + 4000] = torch.randint(0, 256, (n_streams, 4000), dtype=torch.uint8, device="cuda:0", generator=g)
    torch.cuda.synchronize()
    samples = n_streams * n_blocks * api.BLOCK_DEC
    with api.Receiver(n_streams, 0x2F, 500, 0, max_blocks=n_blocks) as r:
        r.enable_capture(n_streams * (n_blocks * api.BLOCK_DEC // 356 + 3), samples)
        r.enable_capture_pre()
        for k in range(WARMUP + submits):
            r.reset_streams(range(n_streams))  # every submit a fresh stream: its table is submit-relative and complete
            r.submit(iq, n_blocks)
            if k == WARMUP + submits - 1:
                runs, pool, pre = r.read_captures(pre=True)
            r.drain()
    del iq
    with api.Receiver(n_streams, 0x2F, 500, 0, max_blocks=n_blocks, decimated=True) as r:
        rows = torch.randint(-40, 41, (n_streams, n_blocks * api.BLOCK_DEC * 2), dtype=torch.int16, device="cuda:0", generator=g)
        rows = rows.view(torch.uint8)
        torch.cuda.synchronize()
        for _ in range(WARMUP + submits):
            r.submit(rows, n_blocks)
            r.drain()
        del rows
    with api.Receiver(n_streams, 0x2F, 500, 0, max_blocks=n_blocks, decimated=True) as r:
        r.enable_runs_input(len(runs), len(pool))
        for _ in range(WARMUP + submits):
            r.reset_streams(range(n_streams))
            r.submit_runs(runs, pool, pre, n_blocks)
            r.drain()
    sparse = len(runs) * 20 + len(pool) * 4 + (n_streams + 1) * 4 + n_streams * 8
    print("decin_cost totals: %d runs, %d pairs of %d samples per submit (captured share %.4f)"
          % (len(runs), len(pool), samples, len(pool) / samples), flush=True)
    print("decin_cost pcie: a sparse submit moves %d bytes (table 16 and pre 4 per run, pool 4 per pair, first_run and overrides), "
          "the dense submit of the same rows %d bytes: %.4f of it" % (sparse, 4 * samples, sparse / (4.0 * samples)), flush=True)


def report(trace_dir: str, n_streams: int, n_blocks: int, submits: int, pairs: int) -> str:
    d = durations(trace_dir)
    samples = n_streams * n_blocks * 8192
    lines = ["decin_cost: %d streams x %d blocks per submit, %d timed submits per context after %d warm-up submits"
             % (n_streams, n_blocks, submits, WARMUP)]
    for kernel in KERNELS:
        t = sum((d[k] for k in sorted(d) if kernel in k), [])[WARMUP:]
        if not t:
            lines.append("%-24s no launches found" % kernel)
            continue
        lines.append("%-24s median %8.3f ms  range %8.3f .. %8.3f ms  (%d launches)"
                     % (kernel, statistics.median(t) / 1e6, min(t) / 1e6, max(t) / 1e6, len(t)))
    dense = samples * (4 + 4) + samples // 8
    sparse = samples * 4 + samples // 8 + pairs * 4
    lines.append("floor at 8 TB/s: dense (4 B read, 4 B written per sample, the mask) %.3f GB, %.3f ms; sparse (4 B written per sample, "
                 "the mask, %d pairs read) %.3f GB, %.3f ms; frontend_kernel reads 8 B per decimated sample instead of 4"
                 % (dense / 1e9, 1e3 * dense / HBM_PEAK, pairs, sparse / 1e9, 1e3 * sparse / HBM_PEAK))
    return "\n".join(lines)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", action="store_true", help="run the submits (what the profiler traces)")
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "decin_cost"))
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--blocks", type=int, default=48)
    ap.add_argument("--submits", type=int, default=6)
    ap.add_argument("--bursts", type=int, default=6)
    a = ap.parse_args()
    if a.workload:
        workload(a.streams, a.blocks, a.submits, a.bursts)
        return 0
    os.makedirs(a.out, exist_ok=True)
    cmd = ["timeout", "-k", "10", str(TIME_LIMIT), "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", a.out,
           "-o", "decin_cost", "--", sys.executable, os.path.abspath(__file__), "--workload", "--streams", str(a.streams),
           "--blocks", str(a.blocks), "--submits", str(a.submits), "--bursts", str(a.bursts)]
    child = subprocess.run(cmd, check=True, capture_output=True, text=True)
    info = [ln for ln in child.stdout.splitlines() if ln.startswith("decin_cost ")]
    pairs = 0
    for ln in info:
        if ln.startswith("decin_cost totals:"):
            pairs = int(ln.split()[4])
    text = report(a.out, a.streams, a.blocks, a.submits, pairs) + "\n" + "\n".join(info)
    print(text)
    with open(os.path.join(a.out, "decin_cost.txt"), "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
