"""Cost of tfrec_amd_save_streams and tfrec_amd_load_streams: the wall-clock time of one save and of one load of every
stream of a 0x2f context, the pipeline idle, and the size of a blob.

    python profiles/ubench/state_cost.py [--out DIR] [--streams 1024] [--blocks 8] [--repeats 7]

starts itself as a child process under a time limit and prints what it measured.  The context runs one submit first, so that the state
it moves is a receiver's; each call is then timed with nothing queued -- the wait for the pipeline, which is the calls' documented
price, is NOT in these figures: it is whatever the submits in flight still take.  The first save also makes the staging buffer; it is
reported apart.  The blobs are loaded back into the streams they came from.  A record, not a gate.
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

TIME_LIMIT = 300  # seconds, for the child


def workload(n_streams: int, n_blocks: int, repeats: int) -> None:
    import torch

    from tfrec_amd import api, synth

    iq = torch.from_numpy(synth.gen_batch(5, 0, n_streams, n_blocks)).to("cuda:0")
    with api.Receiver(n_streams, 0x2F, 500, 0, max_blocks=n_blocks) as r:
        r.submit(iq, n_blocks)
        r.drain()
        r.sync()
        streams = list(range(n_streams))
        t0 = time.perf_counter()
        blobs = r.save_streams(streams)
        first = time.perf_counter() - t0
        save, load = [], []
        for _ in range(repeats):
            t0 = time.perf_counter()
            again = r.save_streams(streams)
            save.append(time.perf_counter() - t0)
            assert again.tobytes() == blobs.tobytes()
            t0 = time.perf_counter()
            r.load_streams(streams, blobs)
            load.append(time.perf_counter() - t0)
        print("state_cost: %d streams, types 0x2f, blob %d bytes (header 128), %.3f MB in all" % (n_streams, r.state_bytes, blobs.nbytes / 1e6))
        print("state_cost: first save (makes the staging buffer) %.3f ms" % (1e3 * first))
        for name, t in (("save", save), ("load", load)):
            print("state_cost: %s median %.3f ms  range %.3f .. %.3f ms  (%d calls, pipeline idle, Python binding included)"
                  % (name, 1e3 * statistics.median(t), 1e3 * min(t), 1e3 * max(t), len(t)), flush=True)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", action="store_true", help="run the calls (the child process)")
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "state_cost"))
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--blocks", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=7)
    a = ap.parse_args()
    if a.workload:
        workload(a.streams, a.blocks, a.repeats)
        return 0
    os.makedirs(a.out, exist_ok=True)
    cmd = ["timeout", "-k", "10", str(TIME_LIMIT), sys.executable, os.path.abspath(__file__), "--workload", "--streams", str(a.streams),
           "--blocks", str(a.blocks), "--repeats", str(a.repeats)]
    child = subprocess.run(cmd, check=True, capture_output=True, text=True)
    text = "\n".join(ln for ln in child.stdout.splitlines() if ln.startswith("state_cost"))
    print(text)
    with open(os.path.join(a.out, "state_cost.txt"), "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
