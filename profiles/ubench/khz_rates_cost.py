"""Cost of the resampling stage at the whole-kHz rates (Q | 1536) against the neighbouring rate with Q <= 64 and the
same T: kernel time per output of the u8 untuned kernel and of the s16 kernel, for 256 streams x 6 units of blocks per submit (one
unit of 24 blocks at Q = 1536, whose rows are ten times as long).

    python profiles/ubench/khz_rates_cost.py [--out DIR] [--streams 256] [--submits 6]

    new rate      T    neighbour      kernels at the new rate
    125/96        8    4/3            staged table (resample_kernel, resample_fmt_kernel)
    625/384      10    13/8           staged table, the largest one (3840 taps)
    625/96       40    417/64         staged table, the largest one
    3125/384     50    521/64         resample_stream_kernel: 19200 taps from global memory
    735/512      10    13/8           resample_stream_kernel: 5120 taps
    1537/1536     8    4/3            resample_stream_kernel: 12288 taps, every output of a tile another phase
    15359/1536   60    639/64         resample_stream_kernel: 92160 taps (360 KB)

starts `rocprofv3 --kernel-trace --stats -- python khz_rates_cost.py --workload ...` as a child process (a kernel trace in a run of
its own, nothing else traced), reads the trace and prints, per context, the median and the range of the timed launches and the
time per output sample.  The first two submits of every context are warm-up and are left out.  The input is near-silence: nothing
triggers, so the chains behind the front end are idle.  A record, not a gate: no number here is asserted.
"""
from __future__ import annotations

import argparse
import csv
import glob
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PAIRS = [((125, 96), (4, 3)), ((625, 384), (13, 8)), ((625, 96), (417, 64)), ((3125, 384), (521, 64)), ((735, 512), (13, 8)),
         ((1537, 1536), (4, 3)), ((15359, 1536), (639, 64))]
FORMATS = ("u8", "s16")
WARMUP = 2
UNITS = 6


def contexts():
    """(rate, format, blocks per submit) in launch order: each new rate, then its neighbour (a neighbour once)."""
    from tfrec_amd import resample

    seen, out = set(), []
    for pair in PAIRS:
        for p, q in pair:
            if (p, q) in seen:
                continue
            seen.add((p, q))
            unit = resample.permitted_blocks(q)
            for fmt in FORMATS:
                out.append(((p, q), fmt, unit * (1 if q == 1536 else UNITS)))
    return out


def workload(n_streams: int, submits: int) -> None:
    import torch

    from tfrec_amd import api

    for rate, fmt, n_blocks in contexts():
        kw = {"input_rate": rate} if fmt == "u8" else {"input_rate": rate, "input_format": fmt}
        with api.Receiver(n_streams, 0x2F, 500, 0, max_blocks=n_blocks, **kw) as r:
            nbytes = r.input_bytes(n_blocks)
            if fmt == "u8":
                iq = torch.randint(124, 133, (n_streams, nbytes), dtype=torch.uint8, device="cuda:0")
            else:  # int16 values of a few hundred: the low byte random, the high byte 0
                iq = torch.randint(0, 256, (n_streams, nbytes), dtype=torch.uint8, device="cuda:0")
                iq[:, 1::2] = 0
            torch.cuda.synchronize()
            for _ in range(WARMUP + submits):
                r.submit(iq, n_blocks)
                r.drain()
            r.sync()
        del iq
        torch.cuda.empty_cache()


def report(trace_dir: str, n_streams: int, submits: int) -> str:
    rows = []  # every resampling launch in start order: the contexts run one after the other, one such kernel per submit
    for f in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(f, newline="") as fd:
            rows += [r for r in csv.DictReader(fd) if "resample_" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    launches = [(r["Kernel_Name"], int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) for r in rows]
    per = WARMUP + submits
    ctx = contexts()
    assert len(launches) == per * len(ctx), "%d resampling launches in the trace, %d expected" % (len(launches), per * len(ctx))
    lines = ["khz_rates_cost: %d streams x %d units of blocks per submit (1 unit at Q = 1536), %d timed submits per context after %d warm-up submits"
             % (n_streams, UNITS, submits, WARMUP)]
    per_out = {}
    for i, (rate, fmt, n_blocks) in enumerate(ctx):
        mine = launches[i * per + WARMUP:(i + 1) * per]
        names = {n.split("(")[0] for n, _ in launches[i * per:(i + 1) * per]}
        assert len(names) == 1, names
        t = [v for _, v in mine]
        n_out = n_streams * n_blocks * 32768
        med = statistics.median(t)
        per_out[rate, fmt] = (med / n_out * 1e3, min(t) / n_out * 1e3, max(t) / n_out * 1e3)
        name = names.pop().replace("tfrec::", "").replace("void ", "")
        lines.append("%-11s %-3s %3d blocks  %-28s median %8.3f ms  range %8.3f .. %8.3f ms  (%d launches)  %7.3f ps per output (%.3f .. %.3f)"
                     % ("%d/%d" % rate, fmt, n_blocks, name[:28], med / 1e6, min(t) / 1e6, max(t) / 1e6, len(t), *per_out[rate, fmt]))
    lines.append("per output, new rate against its neighbour of the same T (medians):")
    for new, old in PAIRS:
        for fmt in FORMATS:
            a, b = per_out[new, fmt], per_out[old, fmt]
            lines.append("%-11s vs %-7s %-3s  %7.3f vs %7.3f ps  ratio %.3f" % ("%d/%d" % new, "%d/%d" % old, fmt, a[0], b[0], a[0] / b[0]))
    return "\n".join(lines)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", action="store_true", help="run the submits (what the profiler traces)")
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "khz_rates_cost"))
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--submits", type=int, default=6)
    a = ap.parse_args()
    if a.workload:
        workload(a.streams, a.submits)
        return 0
    os.makedirs(a.out, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", a.out, "-o", "khz_rates_cost", "--",
           sys.executable, os.path.abspath(__file__), "--workload", "--streams", str(a.streams), "--submits", str(a.submits)]
    subprocess.run(cmd, check=True)
    text = report(a.out, a.streams, a.submits)
    print(text)
    with open(os.path.join(a.out, "khz_rates_cost.txt"), "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
