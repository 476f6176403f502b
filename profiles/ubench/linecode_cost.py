"""Cost of the line code: kernel time of run_records_init_kernel<tfrec_amd_track> (the track's and the code's: one
instantiation), linecode_kernel and linecode_carry_kernel beside sync_kernel's and track_kernel's, for the G3RUH taps {12, 17} and for
NRZI's {1} at 17240 bit/s, each with a 16-bit sync on the coded track, and the period per submit of those contexts against one
with the track alone (the same recorder and pool), on the same input in the same session.

    python profiles/ubench/linecode_cost.py [--out DIR] [--streams 1024] [--blocks 48] [--submits 12] [--bursts 6] [--rate 17240]

starts `rocprofv3 --kernel-trace --stats -- python linecode_cost.py --workload ...` as a child process under a time limit (a kernel
trace in a run of its own, nothing else traced), reads the kernel trace it wrote and prints, per kernel, the median and the range of
the timed launches; linecode_kernel's are split by context, which run one after the other.  The first two submits of every context
are warm-up and are left out of the periods.  The input is the track's cost input (track_cost.py's, which is capture_cost.py's):
near-silence with `--bursts` stretches of full-scale noise per stream and block.  Its track is noise, so about half the coded bits
are ones and nearly every lane issues its atomic ORs.  The floor named beside linecode_kernel's time is one read of the captured
samples' track words.  A record, not a gate.
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
KERNELS = ("run_records_init_kernel<tfrec_amd_track>", "linecode_kernel", "linecode_carry_kernel", "sync_kernel", "track_kernel")
WORD = (0xB42B, 16)  # the sync on the coded track
# context -> the taps; None: the track alone
KINDS = (("g3ruh", 0x10800), ("nrzi", 1), ("track", None))


def workload(n_streams: int, n_blocks: int, submits: int, bursts: int, rate: int) -> None:
    import torch

    from tfrec_amd import api, track

    g = torch.Generator(device="cuda:0").manual_seed(3)
    iq = torch.randint(124, 133, (n_streams, n_blocks * api.BLOCK_BYTES), dtype=torch.uint8, device="cuda:0", generator=g)
    where = torch.randint(0, api.BLOCK_BYTES - 4000, (n_blocks * bursts,), generator=torch.Generator().manual_seed(4)).tolist()
    for k, off in enumerate(where):  # (the same places in every stream: the share, not the pattern, is what matters here)
        a = (k // bursts) * api.BLOCK_BYTES + off
        iq[:, a:a + 4000] = torch.randint(0, 256, (n_streams, 4000), dtype=torch.uint8, device="cuda:0", generator=g)
    torch.cuda.synchronize()
    samples = n_streams * n_blocks * api.BLOCK_DEC
    max_runs = n_streams * (n_blocks * api.BLOCK_DEC // 356 + 3)
    for kind, taps in KINDS:
        with api.Receiver(n_streams, 0x2F, 500, 0, max_blocks=n_blocks) as r:
            r.enable_capture(max_runs, samples)  # a pool for every sample: what the bitmaps are sized by
            r.enable_burst_track(track.smooth_of(rate))
            if taps:
                r.enable_burst_code(rate, taps)
                r.enable_burst_sync(rate, WORD[0], WORD[1], 0)
            t0 = 0.0
            nr, npairs = api.C.c_uint32(0), api.C.c_uint64(0)
            for k in range(WARMUP + submits):
                if k == WARMUP:
                    r.sync()
                    t0 = time.perf_counter()
                r.submit(iq, n_blocks)
                # the counts; the records and the words stay on the device (their copy is the caller's choice)
                r.L.tfrec_amd_read_captures(r.h, None, 0, api.C.byref(nr), None, 0, api.C.byref(npairs))
                r.drain()
            r.sync()
            print("linecode_cost period: %s context %.3f ms per submit (submit, the counts, drain; %d submits)"
                  % (kind, 1e3 * (time.perf_counter() - t0) / submits, submits), flush=True)
            if kind == "track":
                print("linecode_cost totals: %d runs, %d pairs of %d samples per submit (captured share %.4f)"
                      % (nr.value, npairs.value, samples, npairs.value / samples), flush=True)


def _line(name, t):
    return "%-42s median %8.3f ms  range %8.3f .. %8.3f ms  (%d launches, warm-up included)" % (
        name, statistics.median(t) / 1e6, min(t) / 1e6, max(t) / 1e6, len(t))


def report(trace_dir: str, n_streams: int, n_blocks: int, submits: int, pairs: int) -> str:
    d = durations(trace_dir)
    lines = ["linecode_cost: %d streams x %d blocks per submit, %d timed submits per context after %d warm-up submits" % (
        n_streams, n_blocks, submits, WARMUP)]
    for kernel in KERNELS:
        t = sum((d[k] for k in sorted(d) if kernel in k), [])
        if not t:
            lines.append("%-42s no launches found" % kernel)
        elif kernel == "linecode_kernel" and len(t) % 2 == 0:  # the two coded contexts, in the order they ran
            lines.append(_line("linecode_kernel, taps 12 17", t[:len(t) // 2]))
            lines.append(_line("linecode_kernel, tap 1", t[len(t) // 2:]))
        else:
            lines.append(_line(kernel, t))
    lines.append("traffic floor of linecode_kernel (the captured samples' track words read once: %.3f GB) %.4f ms at 8 TB/s" % (
        pairs / 8 / 1e9, 1e3 * pairs / 8 / HBM_PEAK))
    return "\n".join(lines)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", action="store_true", help="run the submits (what the profiler traces)")
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "linecode_cost"))
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--blocks", type=int, default=48)
    ap.add_argument("--submits", type=int, default=12)
    ap.add_argument("--bursts", type=int, default=6)
    ap.add_argument("--rate", type=int, default=17240)
    a = ap.parse_args()
    if a.workload:
        workload(a.streams, a.blocks, a.submits, a.bursts, a.rate)
        return 0
    os.makedirs(a.out, exist_ok=True)
    cmd = ["timeout", "-k", "10", str(TIME_LIMIT), "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", a.out,
           "-o", "linecode_cost", "--", sys.executable, os.path.abspath(__file__), "--workload", "--streams", str(a.streams),
           "--blocks", str(a.blocks), "--submits", str(a.submits), "--bursts", str(a.bursts), "--rate", str(a.rate)]
    child = subprocess.run(cmd, check=True, capture_output=True, text=True)
    info = [ln for ln in child.stdout.splitlines() if ln.startswith("linecode_cost ")]
    pairs = 0
    for ln in info:
        if ln.startswith("linecode_cost totals:"):
            pairs = int(ln.split()[4])
    text = report(a.out, a.streams, a.blocks, a.submits, pairs) + "\n" + "\n".join(info)
    print(text)
    with open(os.path.join(a.out, "linecode_cost.txt"), "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
