"""Cost of the packet check: kernel time of packet_kernel and packet_carry_kernel beside sync_kernel's (P = 16) and
crc_kernel<16>'s (N = 12: 96 terms) in ONE context at 38400 bit/s, on the same input in the same submits: the CC1101's settings
(CRC-16 0x8005 from 0xFFFF, PN9, lengths 0 .. 160) on crc_cost.py's bursty input -- near-silence with `--bursts` stretches of
full-scale noise per stream and block, on which a 16-bit word matches by chance about once in 65536 captured samples, so the
candidates are as sparse as the stage expects them.

    python profiles/ubench/packet_cost.py [--out DIR] [--streams 1024] [--blocks 48] [--submits 12] [--bursts 6]

starts `rocprofv3 --kernel-trace --stats -- python packet_cost.py --workload ...` as a child process under a time limit (a kernel trace
in a run of its own, nothing else traced), reads the kernel trace it wrote and prints, per kernel, the median and the range of the
launches.  A record, not a gate.
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
KERNELS = ("run_records_init_kernel<tfrec_amd_burst_packet>", "packet_kernel", "packet_carry_kernel", "crc_kernel", "sync_kernel", "track_kernel")
RATE = 38400


def workload(n_streams: int, n_blocks: int, submits: int, bursts: int) -> None:
    import torch

    from tfrec_amd import api, packet, track

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
        r.enable_burst_track(track.smooth_of(RATE))
        r.enable_burst_sync(RATE, 0x2DD4, 16, 0)
        r.enable_burst_crc(RATE, 12, 16, 0x8005, 0xFFFF)
        r.enable_burst_packets(RATE, 160, 16, 0x8005, 0xFFFF, whiten=packet.pn9(274))
        for k in range(WARMUP + submits):
            r.submit(iq, n_blocks)
            if k == WARMUP + submits - 1:
                got, _ = r.read_burst_packets()
                print("packet_cost totals: %d runs, %d samples captured of %d, %d candidates evaluated, %d ok" % (
                    len(got), int(got["n_samples"].sum()), samples, int(got["n_seen"].sum()), int(got["n_ok"].sum())), flush=True)
            r.drain()
        r.sync()


def report(trace_dir: str, n_streams: int, n_blocks: int, submits: int) -> str:
    d = durations(trace_dir)
    lines = ["packet_cost: %d streams x %d blocks per submit, %d submits after %d warm-up submits, one context at %d bit/s" % (
        n_streams, n_blocks, submits, WARMUP, RATE)]
    for kernel in KERNELS:
        t = sum((d[k] for k in sorted(d) if kernel in k), [])
        lines.append("%-50s median %8.3f ms  range %8.3f .. %8.3f ms  (%d launches, warm-up included)" % (
            kernel, statistics.median(t) / 1e6, min(t) / 1e6, max(t) / 1e6, len(t)) if t else "%-50s no launches found" % kernel)
    return "\n".join(lines)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", action="store_true", help="run the submits (what the profiler traces)")
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "packet_cost"))
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
           "-o", "packet_cost", "--", sys.executable, os.path.abspath(__file__), "--workload", "--streams", str(a.streams),
           "--blocks", str(a.blocks), "--submits", str(a.submits), "--bursts", str(a.bursts)]
    child = subprocess.run(cmd, check=True, capture_output=True, text=True)
    text = report(a.out, a.streams, a.blocks, a.submits) + "\n" + "\n".join(ln for ln in child.stdout.splitlines() if ln.startswith("packet_cost "))
    print(text)
    with open(os.path.join(a.out, "packet_cost.txt"), "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
