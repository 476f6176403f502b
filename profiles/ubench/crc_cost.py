"""Cost of the frame check: kernel time of run_records_init_kernel<tfrec_amd_burst_crc>, crc_kernel and crc_carry_kernel
beside sync_kernel's (P = 16) and track_kernel's, for the TFA_2 family's CRC (W = 8, N = 5 at 17240 bit/s: 40 terms) and for WHB's (W =
32, N = 23 behind a skipped byte at 6000 bit/s: 176 terms), each with a 16-bit sync on the same track, and the period per submit of
those contexts against one with the track alone (the same recorder and pool), on the same input in the same session.

    python profiles/ubench/crc_cost.py [--out DIR] [--streams 1024] [--blocks 48] [--submits 12] [--bursts 6] [--rate 17240]

starts `rocprofv3 --kernel-trace --stats -- python crc_cost.py --workload ...` as a child process under a time limit (a kernel trace in
a run of its own, nothing else traced), reads the kernel trace it wrote and prints, per kernel, the median and the range of the timed
launches; crc_kernel's and sync_kernel's are split by context, which run one after the other.  The first two submits of every
context are warm-up and are left out of the periods.  The input is the track's cost input (track_cost.py's, which is
capture_cost.py's): near-silence with `--bursts` stretches of full-scale noise per stream and block.  Its runs are about 1900
samples long: longer than the small setting's D = 891, so most of their samples are defined there, and shorter than WHB's D = 11776,
so within a submit none is -- a lane without a defined sample skips the term loop, and what WHB's setting costs there is the LDS fill
and the run loop.  A fourth context therefore runs WHB's setting on a second input, full-scale noise throughout: one run per stream
that never ends, every sample captured and, from the second block on, defined -- WHB's term loop at every lane --, with sync_kernel
and track_kernel on that input beside it.  The floor named beside crc_kernel's time is one read of the captured samples' track
words of the bursty input.  A record, not a gate.
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
KERNELS = ("run_records_init_kernel<tfrec_amd_burst_crc>", "crc_kernel", "crc_carry_kernel", "sync_kernel", "track_kernel")
WORD = (0x2DD4, 16)  # the sync beside the check
# context -> enable_burst_crc's arguments (rate, N, W, poly, init, xorout, skip, lsb); None: the track alone
WHB = (6000, 23, 32, 0x04C11DB7, 0xF59C5A1E, 0, 1, True)
# (context, its arguments, the input): the bursty cost input, or noise throughout
KINDS = (("crc8", (17240, 5, 8, 0x31), "bursts"), ("whb", WHB, "bursts"), ("track", None, "bursts"), ("whb_long", WHB, "noise"))


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
    for kind, taps, which in KINDS:
        if which == "noise":  # the second input, in the first one's place
            iq.random_(0, 256, generator=g)
            torch.cuda.synchronize()
        with api.Receiver(n_streams, 0x2F, 500, 0, max_blocks=n_blocks) as r:
            r.enable_capture(max_runs, samples)  # a pool for every sample: what the bitmaps are sized by
            r.enable_burst_track(track.smooth_of(rate))
            if taps:
                r.enable_burst_sync(taps[0], WORD[0], WORD[1], 0)
                r.enable_burst_crc(*taps)
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
            print("crc_cost period: %s context %.3f ms per submit (submit, the counts, drain; %d submits)"
                  % (kind, 1e3 * (time.perf_counter() - t0) / submits, submits), flush=True)
            if kind == "whb_long":
                print("crc_cost noise: %d runs, %d pairs of %d samples per submit (captured share %.4f)"
                      % (nr.value, npairs.value, samples, npairs.value / samples), flush=True)
            if kind == "track":
                print("crc_cost totals: %d runs, %d pairs of %d samples per submit (captured share %.4f)"
                      % (nr.value, npairs.value, samples, npairs.value / samples), flush=True)


def _line(name, t):
    return "%-42s median %8.3f ms  range %8.3f .. %8.3f ms  (%d launches, warm-up included)" % (
        name, statistics.median(t) / 1e6, min(t) / 1e6, max(t) / 1e6, len(t))


def report(trace_dir: str, n_streams: int, n_blocks: int, submits: int, pairs: int) -> str:
    d = durations(trace_dir)
    per = WARMUP + submits  # launches of a kernel per context
    lines = ["crc_cost: %d streams x %d blocks per submit, %d timed submits per context after %d warm-up submits" % (
        n_streams, n_blocks, submits, WARMUP)]
    for kernel in KERNELS:
        t = sum((d[k] for k in sorted(d) if kernel in k), [])
        if not t:
            lines.append("%-42s no launches found" % kernel)
        elif kernel == "crc_kernel":  # an instantiation per width; W = 32 ran in two contexts, one after the other
            t8 = sum((d[k] for k in sorted(d) if "crc_kernel<8>" in k.replace(" ", "")), [])
            t32 = sum((d[k] for k in sorted(d) if "crc_kernel<32>" in k.replace(" ", "")), [])
            lines.append(_line("crc_kernel, W = 8, N = 5 at 17240 bit/s", t8) if t8 else "%-42s no launches found" % "crc_kernel<8>")
            if t32 and len(t32) == 2 * per:
                lines.append(_line("crc_kernel, W = 32, N = 23 at 6000 bit/s", t32[:per]))
                lines.append(_line("crc_kernel, W = 32, N = 23, noise input", t32[per:]))
            else:
                lines.append(_line("crc_kernel, W = 32 (every launch)", t32) if t32 else "%-42s no launches found" % "crc_kernel<32>")
        elif kernel == "sync_kernel" and len(t) == 3 * per:  # the three checked contexts, in the order they ran
            lines.append(_line("sync_kernel, P = 16 at 17240 bit/s", t[:per]))
            lines.append(_line("sync_kernel, P = 16 at 6000 bit/s", t[per:2 * per]))
            lines.append(_line("sync_kernel, P = 16 at 6000, noise input", t[2 * per:]))
        elif kernel == "track_kernel" and len(t) == 4 * per:
            lines.append(_line("track_kernel", t[:3 * per]))
            lines.append(_line("track_kernel, noise input", t[3 * per:]))
        else:
            lines.append(_line(kernel, t))
    lines.append("traffic floor of crc_kernel (the captured samples' track words read once: %.3f GB) %.4f ms at 8 TB/s" % (
        pairs / 8 / 1e9, 1e3 * pairs / 8 / HBM_PEAK))
    return "\n".join(lines)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", action="store_true", help="run the submits (what the profiler traces)")
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "crc_cost"))
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
           "-o", "crc_cost", "--", sys.executable, os.path.abspath(__file__), "--workload", "--streams", str(a.streams),
           "--blocks", str(a.blocks), "--submits", str(a.submits), "--bursts", str(a.bursts), "--rate", str(a.rate)]
    child = subprocess.run(cmd, check=True, capture_output=True, text=True)
    info = [ln for ln in child.stdout.splitlines() if ln.startswith("crc_cost ")]
    pairs = 0
    for ln in info:
        if ln.startswith("crc_cost totals:"):
            pairs = int(ln.split()[4])
    text = report(a.out, a.streams, a.blocks, a.submits, pairs) + "\n" + "\n".join(info)
    print(text)
    with open(os.path.join(a.out, "crc_cost.txt"), "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
