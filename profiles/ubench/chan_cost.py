"""Cost of shared inputs and the wideband tune.

    python profiles/ubench/chan_cost.py kernels [n_streams]   # run under rocprofv3 --kernel-trace --stats: decim10_kernel<false> / <true>
    python profiles/ubench/chan_cost.py hostfed [out.json]    # K = 8 receivers of one row against 8 copies of the row, host-fed

kernels: two TFREC_AMD_F_INPUT_10X contexts of n_streams (default 512) x 48 blocks on the same device-resident input, one plain,
one with every stream wide-tuned; six submits each.  hostfed: default input, 8 streams x 48 blocks, every stream tuned
(tfrec_amd_tune_streams) in both legs; leg "copies" submits an 8-row host batch to an unmapped context (the kernels and the copy
of a context before inputs could be shared), leg "shared" a 1-row batch to a context whose streams are mapped to row 0.  A B B A
x 3, wall time per submit over 24 submits after 6 warm-up ones, FIFO kept full; pageable host memory in both legs."""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tfrec_amd import api, synth  # noqa: E402

NB = 48


def leg(r, d, steps, warm):
    pending, t0 = 0, 0.0
    for k in range(steps + warm):
        if k == warm:
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
    return (time.perf_counter() - t0) / steps * 1e3


def kernels(n):
    row = torch.from_numpy(synth.gen_scene(5, NB, [dict(proto=1, start=300000, payload_seed=5, f0_hz=3300000)], rate_mult=10))
    d = row.to("cuda:0").repeat(n, 1)
    for wide in (False, True):
        with api.Receiver(n, 0x2F, 500, 0, max_blocks=NB, input_10x=True) as r:
            if wide:
                r.tune_streams_wide(range(n), [((s % 13) - 6) * 1000000 + 300000 for s in range(n)])
            leg(r, d, 5, 1)


def hostfed(path):
    x = synth.gen_batch(5, 0, 1, NB)
    one, eight = np.ascontiguousarray(x), np.ascontiguousarray(np.tile(x, (8, 1)))
    tunes = [(s - 4) * 100000 + 25000 for s in range(8)]
    out = {"copies": [], "shared": []}
    with api.Receiver(8, 0x2F, 500, 0, max_blocks=NB) as a, api.Receiver(8, 0x2F, 500, 0, max_blocks=NB) as b:
        a.tune_streams(range(8), tunes)
        b.tune_streams(range(8), tunes)
        b.map_streams(range(8), 0)
        for _ in range(3):
            for name, r, d in (("copies", a, eight), ("shared", b, one), ("shared", b, one), ("copies", a, eight)):
                out[name].append(round(leg(r, d, 24, 6), 3))
    res = {"ms_per_submit": out, "median": {k: statistics.median(v) for k, v in out.items()},
           "config": "8 streams x %d blocks, default input, types 0x2f, -t 500, host-fed from pageable memory, A B B A x 3" % NB}
    print(json.dumps(res))
    if path:
        with open(path, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    if sys.argv[1] == "kernels":
        kernels(int(sys.argv[2]) if len(sys.argv) > 2 else 512)
    else:
        hostfed(sys.argv[2] if len(sys.argv) > 2 else None)
