"""The randomised campaign of tests/recorder_campaign.py on the GPU: the recorder's table and pool, the level records, and the burst
meter's, the envelope's, the clock's and the track's records and bitmap, byte for byte against the restatements, on rows whose runs
land on the kernels' own strides -- and the layouts no hand-aimed module reaches: more runs in a stream's submit than a workgroup
has lanes, a dense stream beside sparse ones at 65 streams, and the four measurements alone and together.  Everything is an exact
integer; nothing here has a tolerance.  tests/test_recorder_campaign_cpu.py shows that the fixed seeds reach every edge class.

The fixed campaign: seeds recorder_campaign.SEEDS = (12, 19, 21, 24), recorder_campaign.ROUNDS = 6 rounds each.  Wall times measured
on an MI355X host (the restatements on the CPU dominate; the first case also loads the library and starts the device):
  test_campaign[12] 8.3 s, [19] 0.6 s, [21] 0.5 s, [24] 0.7 s
  test_densest_runs_overrun_every_lookup_stride 1.0 s, test_dense_stream_beside_sparse_ones_at_65_streams 0.9 s,
  test_each_measurement_alone_equals_all_four_together 0.3 s; the module 13 s.
python tests/recorder_campaign.py <seed> 50 reported 0 mismatches for the seeds 1001 and 2002, which are not in the list.
"""
import numpy as np
import pytest

import recorder_campaign as RC
from tfrec_amd import capture

pytestmark = pytest.mark.gpu

B = RC.B
ALL = RC.MEASURES


@pytest.mark.parametrize("seed", RC.SEEDS)
def test_campaign(seed):
    assert RC.campaign(seed, RC.ROUNDS, verbose=False) == 0


def pieces(reads, m):
    return [g[m] for g in reads]


def test_densest_runs_overrun_every_lookup_stride():
    """Mask 0x02's densest legal input, one over sample every 357: 276 runs per stream in one submit of 12 blocks, so every
    `for (k = t; k < nr; k += THREADS)` makes a second trip and dozens of runs meet each block's [lo, hi) lookup; the staging has
    room for 279."""
    x = np.stack([RC.dense(12)] * 3)
    centres = [0, 20000, -192000]
    whole = RC.run_plan(RC.make_plan(x, 0x02, [0x02] * 3, (12,), L=5, centres=centres))
    runs = whole[0]["table"][0]
    stage_cap = 12 * B // 356 + 3
    for s in range(3):
        mine = runs[runs["stream"] == s]
        assert 256 < len(mine) <= stage_cap and mine[-1]["flags"] == capture.RUN_OPEN
    for m in ALL:
        assert len(whole[0][m][0] if m == "track" else whole[0][m]) == len(runs) == 3 * 276
    # the same rows cut as (5, 7), both submits queued before the first read: the merged chains are the uncut ones
    cut = RC.run_plan(RC.make_plan(x, 0x02, [0x02] * 3, (5, 7), L=5, centres=centres, drains=[None, None]))
    assert all(max(np.count_nonzero(g["table"][0]["stream"] == s) for s in range(3)) > 100 for g in cut)
    for m in ALL:
        RC.same_chains(m, RC.merged(m, pieces(cut, m)), RC.merged(m, pieces(whole, m)), "cut (5, 7)")


def test_dense_stream_beside_sparse_ones_at_65_streams():
    """Every fourth stream is the dense row under its own mask 0x02, the others generated rows under the context's 0x2F: the run
    lookup, a W per stream and a stream count past one wave together; two submits, both queued before the first read."""
    n, nb = 65, 2
    masks = [0x02 if s % 4 == 0 else 0x2F for s in range(n)]
    x = RC.rows(np.random.default_rng(65), n, nb, [RC.window(m) for m in masks], cuts=(1,))
    x[::4] = RC.dense(nb)
    p = RC.make_plan(x, 0x2F, masks, (1, 1), L=7, centres=[(0, 20000, -35000)[s % 3] for s in range(n)], drains=[None, None])
    assert p["configured"] == list(range(0, n, 4))
    reads = RC.run_plan(p)
    for g in reads:
        per = np.bincount(g["table"][0]["stream"], minlength=n)
        assert (per[::4] >= B // RC.DENSE_PERIOD).all() and per[64] >= 22 and np.delete(per, np.arange(0, n, 4)).min() >= 1
    assert (reads[1]["table"][0]["flags"] & capture.RUN_CONTINUES).any()


def test_each_measurement_alone_equals_all_four_together():
    """The kernels share one low-priority lane and the recorder's buffers: what one measurement reads does not depend on which others
    run beside it, and the table and the pool are a recorder-only context's."""
    rng = np.random.default_rng(4)
    masks = [0x2F, 0x02, 0x21, 0x08, 0x2F]
    x = RC.rows(rng, 5, 3, [RC.window(m) for m in masks], cuts=(1,))
    p = RC.make_plan(x, 0x2F, masks, (1, 2), L=9, centres=[0, 192000, -192000, 20000, -35000], drains=[None, None])
    assert sum(len(e["table"][0]) for e in p["expect"]) >= 40
    plain = RC.run_plan(p, measure=())
    every = RC.run_plan(p, measure=ALL)
    for k, (a, b) in enumerate(zip(plain, every)):
        assert a["table"][0].tobytes() == b["table"][0].tobytes() and a["table"][1].tobytes() == b["table"][1].tobytes(), k
    for m in ALL:
        alone = RC.run_plan(p, measure=(m,))
        for k, (a, b, c) in enumerate(zip(alone, every, plain)):
            assert a["table"][0].tobytes() == c["table"][0].tobytes() and a["table"][1].tobytes() == c["table"][1].tobytes(), (m, k)
            if m == "track":
                assert a[m][0].tobytes() == b[m][0].tobytes() and a[m][1].tobytes() == b[m][1].tobytes(), (m, k)
            else:
                RC.same_records(a[m], b[m], "%s alone, submit %d" % (m, k))
