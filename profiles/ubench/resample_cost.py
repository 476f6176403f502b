"""Cost of the resampling stage and of the input-rate tune ahead of it (6g): kernel time of resample_kernel at
P/Q = 4/3 (2.048 MS/s) and 25/16 (2.4 MS/s) for 1024 streams x 48 blocks, untuned (resample_kernel) and with every stream
tuned at the input rate (resample_fmt_kernel<kFmtU8>, the format kernel's U8 instantiation), and -- for scale, on the same machine in the same run -- of the plain front end
of an unresampled context at the same size.

    python profiles/ubench/resample_cost.py [--out DIR] [--streams 1024] [--blocks 48] [--submits 12]

starts `rocprofv3 --kernel-trace --stats -- python resample_cost.py --workload ...` as a child process (a kernel trace in a
run of its own, nothing else traced), reads the kernel trace it wrote and prints, per kernel, the median and the range of the
timed launches, the input bytes a launch streams and the achieved input bandwidth against the 8 TB/s HBM peak.  The first
two submits of every context are warm-up and are left out.  The input is near-silence (u8 128 +- 4): nothing triggers, so the
demodulator chains behind the front end are idle and the launches of consecutive submits do not share the device with them.
A record, not a gate: no number here is asserted.
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

RATES = [(4, 3), (25, 16)]
WARMUP = 2
HBM_PEAK = 8.0e12  # bytes / s


def workload(n_streams: int, n_blocks: int, submits: int) -> None:
    import torch

    from tfrec_amd import api

    # per rate an untuned context, then one with every stream tuned at the input rate; the plain context last
    for rate, tuned in [(r, t) for r in RATES for t in (False, True)] + [(None, False)]:
        kw = {} if rate is None else {"input_rate": rate}
        with api.Receiver(n_streams, 0x2F, 500, 0, max_blocks=n_blocks, **kw) as r:
            if tuned:
                half = 768000 * rate[0] // rate[1]
                r.tune_streams_input(range(n_streams), [((s % 13) - 6) * (half // 7) + 30000 for s in range(n_streams)])
            nbytes = r.input_bytes(n_blocks)
            iq = torch.randint(124, 133, (n_streams, nbytes), dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            for _ in range(WARMUP + submits):
                r.submit(iq, n_blocks)
                r.drain()
            r.sync()
        del iq
        torch.cuda.empty_cache()


def durations(trace_dir: str) -> dict:
    """kernel name (up to the first '(' or '<') -> launch durations in ns, in launch order."""
    out = {}
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise RuntimeError("no kernel trace under %s" % trace_dir)
    rows = []
    for f in files:
        with open(f, newline="") as fd:
            rows += list(csv.DictReader(fd))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    for r in rows:
        out.setdefault(r["Kernel_Name"], []).append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    return out


def report(trace_dir: str, n_streams: int, n_blocks: int, submits: int) -> str:
    d = durations(trace_dir)
    lines = ["resample_cost: %d streams x %d blocks per submit, %d timed submits per context after %d warm-up submits"
             % (n_streams, n_blocks, submits, WARMUP)]

    def pick(sub):
        names = [k for k in d if sub in k]
        return sum((d[k] for k in sorted(names)), []) if names else []

    def variant(tuned):
        if tuned:  # the template argument 0 = kFmtU8, whether the trace names the kernel mangled or not
            names = [k for k in d if "resample_fmt_kernelILi0E" in k or "resample_fmt_kernel<0>" in k]
        else:
            names = [k for k in d if "resample_kernel" in k]
        return sum((d[k] for k in sorted(names)), [])

    per = WARMUP + submits
    rows = []
    for tuned in (False, True):
        rs = variant(tuned)
        for i, (p, q) in enumerate(RATES):
            rows.append(("%s %d/%d" % ("resample_fmt_kernel<U8> tuned" if tuned else "resample_kernel", p, q),
                         rs[i * per + WARMUP:(i + 1) * per],
                         n_streams * n_blocks * 65536 * p // q))
    # the plain context's front end: the u8 instantiation (the rate contexts run the int16 one)
    fe = [k for k in d if "frontend_kernel" in k and "Lb0ELb0" in k.replace(" ", "")] or [k for k in d if "frontend_kernel<false, false" in k]
    plain = sum((d[k] for k in fe), [])
    rows.append(("frontend_kernel (plain context)", plain[-submits:], n_streams * n_blocks * 65536))
    fe16 = [k for k in d if "frontend_kernel" in k and k not in fe]
    in16 = sum((d[k] for k in fe16), [])
    for i, (p, q) in enumerate(RATES):
        rows.append(("frontend_kernel behind %d/%d (int16 input)" % (p, q), in16[2 * i * per + WARMUP:(2 * i + 1) * per],
                     n_streams * n_blocks * 32768 * 4))
    for name, t, nbytes in rows:
        if not t:
            lines.append("%-44s no launches found" % name)
            continue
        med = statistics.median(t)
        lines.append("%-44s median %8.3f ms  range %8.3f .. %8.3f ms  (%d launches)  input %7.2f GB  %6.2f TB/s = %4.1f %% of 8 TB/s"
                     % (name, med / 1e6, min(t) / 1e6, max(t) / 1e6, len(t), nbytes / 1e9, nbytes / med * 1e9 / 1e12,
                        100.0 * nbytes / med * 1e9 / HBM_PEAK))
    return "\n".join(lines)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", action="store_true", help="run the submits (what the profiler traces)")
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "resample_cost"))
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
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", a.out, "-o", "resample_cost", "--",
           sys.executable, os.path.abspath(__file__), "--workload", "--streams", str(a.streams), "--blocks", str(a.blocks),
           "--submits", str(a.submits)]
    subprocess.run(cmd, check=True)
    text = report(a.out, a.streams, a.blocks, a.submits)
    print(text)
    with open(os.path.join(a.out, "resample_cost.txt"), "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
