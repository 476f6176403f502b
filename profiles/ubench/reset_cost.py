"""Cost of a submit that carries stream resets (tfrec_amd_reset_streams) at the benchmark size: 1024 streams x 48 blocks,
all five protocols, -t 500, the FIFO kept full.  Legs, in turn, three rounds each: no reset, 1 % of the streams (every
100th) reset before every submit, every stream reset before every submit.  Prints one JSON line: per leg the wall time per
submit of each round (ms, 40 submits after 8 warm-up ones) and the median.

    python profiles/ubench/reset_cost.py [out.json]
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


def leg(r, d, rs):
    pending = 0
    for k in range(STEPS + WARM):
        if k == WARM:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        if rs:
            r.reset_streams(rs)
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
    legs = {"none": [], "1pct": list(range(0, N, 100)), "all": list(range(N))}
    out = {k: [] for k in legs}
    with api.Receiver(N, 0x2F, 500, 0, max_blocks=NB) as r:
        for _ in range(3):
            for name, rs in legs.items():
                out[name].append(round(leg(r, d, rs), 3))
    res = {"ms_per_submit": out, "median": {k: statistics.median(v) for k, v in out.items()},
           "config": "%d streams x %d blocks, types 0x2f, -t 500, FIFO depth %d" % (N, NB, api.FIFO_DEPTH)}
    print(json.dumps(res))
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
