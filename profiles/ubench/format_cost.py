"""Cost of the sample formats: kernel time of resample_fmt_kernel for S8, S16 and F32 input at P/Q = 4/3
(2.048 MS/s) and 25/16 (2.4 MS/s), of ingest_kernel at the base rate 1/1, and -- the yardstick, on the same machine in the same
run -- of resample_kernel on u8 at the two rates, all for 1024 streams x 48 blocks.

    python profiles/ubench/format_cost.py [--out DIR] [--streams 1024] [--blocks 48] [--submits 12]

starts `rocprofv3 --kernel-trace --stats -- python format_cost.py --workload ...` as a child process under a time limit (a
kernel trace in a run of its own, nothing else traced), reads the kernel trace it wrote and prints, per kernel and rate, the
median and the range of the timed launches, the input bytes a launch streams and the achieved input bandwidth against the
8 TB/s HBM peak.  The first two submits of every context are warm-up and are left out.  The input is near-silence (|x| <= 256 in
every format): nothing triggers, so the demodulator chains behind the front end are idle.  The comparison is with the u8 rows of
this run and with profiles/resample_cost.txt (6f), not with earlier runs of this script.  A record, not a gate.
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

from resample_cost import HBM_PEAK, RATES, WARMUP, durations  # noqa: E402

FORMATS = ["s8", "s16", "f32"]
BYTES = {"u8": 2, "s8": 2, "s16": 4, "f32": 8}
TAG = {"s8": "Li1E", "s16": "Li2E", "f32": "Li3E"}  # the template argument in a mangled kernel name
# the contexts in launch order: u8 at every rate, every format at every rate, every format at 1/1
CONTEXTS = [("u8", r) for r in RATES] + [(f, r) for f in FORMATS for r in RATES] + [(f, (1, 1)) for f in FORMATS]
TIME_LIMIT = 900  # seconds, for the traced child


def quiet_rows(fmt: str, n_streams: int, nbytes: int):
    """Near-silent rows of the format as a uint8 tensor on the GPU."""
    import torch

    n = n_streams * nbytes // (BYTES[fmt] // 2)
    if fmt == "u8":
        return torch.randint(124, 133, (n_streams, nbytes), dtype=torch.uint8, device="cuda:0")
    if fmt == "s8":
        return torch.randint(-4, 5, (n,), dtype=torch.int8, device="cuda:0").view(torch.uint8).view(n_streams, nbytes)
    if fmt == "s16":
        return torch.randint(-1024, 1025, (n,), dtype=torch.int16, device="cuda:0").view(torch.uint8).view(n_streams, nbytes)
    return ((torch.rand((n,), dtype=torch.float32, device="cuda:0") - 0.5) / 16).view(torch.uint8).view(n_streams, nbytes)


def workload(n_streams: int, n_blocks: int, submits: int) -> None:
    import torch

    from tfrec_amd import api

    for fmt, rate in CONTEXTS:
        kw = {"input_rate": rate} if fmt == "u8" else {"input_rate": rate, "input_format": fmt}
        with api.Receiver(n_streams, 0x2F, 500, 0, max_blocks=n_blocks, **kw) as r:
            iq = quiet_rows(fmt, n_streams, r.input_bytes(n_blocks))
            torch.cuda.synchronize()
            for _ in range(WARMUP + submits):
                r.submit(iq, n_blocks)
                r.drain()
            r.sync()
        del iq
        torch.cuda.empty_cache()


def report(trace_dir: str, n_streams: int, n_blocks: int, submits: int) -> str:
    d = durations(trace_dir)
    lines = ["format_cost: %d streams x %d blocks per submit, %d timed submits per context after %d warm-up submits"
             % (n_streams, n_blocks, submits, WARMUP)]

    def launches(kernel, mangled, arg):
        """the launches of kernel<arg>, whether the trace names it mangled or not"""
        names = [k for k in d if kernel + mangled in k or "%s<%s>" % (kernel, arg) in k]
        return sum((d[k] for k in sorted(names)), [])

    per = WARMUP + submits
    rows = []
    u8 = sum((d[k] for k in sorted(d) if "resample_kernel" in k), [])  # (no stream is tuned: the plain u8 kernel)
    for i, (p, q) in enumerate(RATES):
        rows.append(("resample_kernel u8 %d/%d" % (p, q), u8[i * per + WARMUP:(i + 1) * per], n_streams * n_blocks * 65536 * p // q))
    for k, fmt in enumerate(FORMATS):
        t = launches("resample_fmt_kernel", "I" + TAG[fmt], k + 1)
        for i, (p, q) in enumerate(RATES):
            rows.append(("resample_fmt_kernel %s %d/%d" % (fmt, p, q), t[i * per + WARMUP:(i + 1) * per],
                         n_streams * n_blocks * 32768 * BYTES[fmt] * p // q))
    for k, fmt in enumerate(FORMATS):
        t = launches("ingest_kernel", "I" + TAG[fmt], k + 1)
        rows.append(("ingest_kernel %s 1/1" % fmt, t[WARMUP:per], n_streams * n_blocks * 32768 * BYTES[fmt]))
    for name, t, nbytes in rows:
        if not t:
            lines.append("%-36s no launches found" % name)
            continue
        med = statistics.median(t)
        lines.append("%-36s median %8.3f ms  range %8.3f .. %8.3f ms  (%d launches)  input %7.2f GB  %6.2f TB/s = %4.1f %% of 8 TB/s"
                     % (name, med / 1e6, min(t) / 1e6, max(t) / 1e6, len(t), nbytes / 1e9, nbytes / med * 1e9 / 1e12,
                        100.0 * nbytes / med * 1e9 / HBM_PEAK))
    return "\n".join(lines)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", action="store_true", help="run the submits (what the profiler traces)")
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "format_cost"))
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--blocks", type=int, default=48)
    ap.add_argument("--submits", type=int, default=12)
    a = ap.parse_args()
    if a.blocks % 3:
        ap.error("--blocks must be a multiple of 3 (the 4/3 rate)")
    if a.workload:
        workload(a.streams, a.blocks, a.submits)
        return 0
    os.makedirs(a.out, exist_ok=True)
    cmd = ["timeout", "-k", "10", str(TIME_LIMIT), "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", a.out,
           "-o", "format_cost", "--", sys.executable, os.path.abspath(__file__), "--workload", "--streams", str(a.streams),
           "--blocks", str(a.blocks), "--submits", str(a.submits)]
    subprocess.run(cmd, check=True)
    text = report(a.out, a.streams, a.blocks, a.submits)
    print(text)
    with open(os.path.join(a.out, "format_cost.txt"), "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
