"""Cost of digital tuning (tfrec_amd_tune_streams) at the benchmark size: 1024 streams x 48 blocks, all five protocols, -t 500,
the FIFO kept full.  Two contexts on the same input: one untuned (the kernels of every untuned context), one with every
stream tuned (offsets from -275 kHz to +325 kHz: the tuned front end rotates every sample).  Legs in A B B A order, three
rounds; prints one JSON line: per leg the wall time per submit of each leg run (ms, 40 submits after 8 warm-up ones, the
first of which carries the tune's restart) and the median.

    python profiles/ubench/tune_cost.py [out.json]
"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tfrec_amd import api, synth  # noqa: E402

N, NB, STEPS, WARM = 1024, 48, 40, 8


def leg(r, d):
    pending = 0
    for k in range(STEPS + WARM):
        if k == WARM:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        if pending == api.FIFO_DEPTH:
            r.drain()
            pending -= 1
        r.submit(d)
        pending += 1
    while pending:
        r.drain()
        pending -= 1
    return (time.perf_counter() - t0) / STEPS * 1e3


def main():
    base = synth.gen_batch(5, 0, 64, NB)
    d = torch.from_numpy(np.tile(base, (N // 64, 1))).to("cuda:0")
    out = {"none": [], "tuned": []}
    with api.Receiver(N, 0x2F, 500, 0, max_blocks=NB) as a, api.Receiver(N, 0x2F, 500, 0, max_blocks=NB) as b:
        b.tune_streams(range(N), [((s % 7) - 3) * 100000 + 25000 for s in range(N)])
        for _ in range(3):
            for name, r in (("none", a), ("tuned", b), ("tuned", b), ("none", a)):
                out[name].append(round(leg(r, d), 3))
    res = {"ms_per_submit": out, "median": {k: statistics.median(v) for k, v in out.items()},
           "config": "%d streams x %d blocks, types 0x2f, -t 500, FIFO depth %d, A B B A x 3" % (N, NB, api.FIFO_DEPTH)}
    print(json.dumps(res))
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
