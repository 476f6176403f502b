#!/usr/bin/env python3
"""bench.py -- IQ MSamples/s through full demod+decode on batched synthetic 1.536 MS/s streams.

Contract: `python bench.py --gpus N --steps K --warmup W` (N>1 launched by torch.distributed.run, one rank
per GPU).  A step = one pass of the hot path (front-end FIR kernel + demodulator/decoder chains + event
drain to the host) over one batch of synthetic input that is already resident in HBM.

Workload (BASELINE.json configs[2], the configuration the "batched streams" metric is quoted on):
1024 streams x 48 blocks (1.024 s of signal each = 1 572 864 complex samples) x all five protocols,
fixed threshold -t 500, per GPU.  With N GPUs every rank gets its own 1024 streams (configs[3] at N=8:
8192 streams, weak scaling, no collective on the data path -- streams are independent).

A plain run does what its headline figure needs: it sets up, warms up, times the steps, writes --dump-outputs and prints
the line.  `--full` adds everything else the benchmark measures or checks: the oracle parity gates before and after the
timed region, the CPU baseline, the PCIe-inclusive leg and the other configurations.  Both runs submit the same batches in
the same order (the gate's batch included), so their timed steps and dumped outputs are the same.

Rank 0 prints ONE JSON line with the contract fields plus
  "roofline":     dominant kernel (longest live HIP-event span) vs the HBM roofline (algorithmic bytes = 2 B per complex input
                  sample), the whole path's fraction; from the builder's committed rocprofv3 runs of this command (named in the
                  block): that kernel's average in the kernel trace, HBM traffic, and "valu" = the batch's VALU instruction mix
                  against the measured issue cost per class ("state both numbers"),
  "cpu_baseline": (--full) the reference CPU path timed on this box's host cores (1 thread) on a bounded sample,
  "h2d_included": (--full) the same batches fed from page-locked HOST memory through the submit/drain FIFO (PCIe-inclusive
                  rate; never `value`),
  "other_configs": (--full) short measurements of the other single-GPU configurations of BASELINE.json,
  "ms_min/ms_median/ms_max": per-step dispersion (time between consecutive drains inside the timed region);
  "ms_per_step_steady": the same without the steps in which the FIFO fills and drains.
  "host_ms":      the host's side of the timed region: every submit's duration, the longest gap between two drains, pauses of
                  Python's garbage collector (a stalled host starves the pipeline without showing in any kernel's interval).
  "roofline" also states what binds: hbm_floor_ms (2 B per input sample at 8 TB/s), algorithmic_valu_floor_ms (the reference's
                  arithmetic 64 lanes wide at one instruction per SIMD and quad-cycle: derivation above ALG_OPS and in
                  DESIGN.md 3), chain_floor_ms (the longest kernel alone on the chip: the serial WHB chains),
                  period_over_max_floor, frontend = {ms_alone, frac}; valu_profiled.* and traffic* come from the builder's
                  committed rocprofv3 runs of this command (profiles/, named in the block), not from this run.
  "roofline.kernel" is the kernel with the longest live HIP-event span inside the overlapped pipeline (it includes the
                  kernel's waits for issue slots beside the other streams' kernels).
The steps ROTATE through config.distinct_batches (3) distinct synthetic batches of their own seeds -- A, B, C, A, ... -- so that
no stream is given the same block twice in a row (engine.cpp:63-93) and every one of the library's four buffer sets holds
every batch in turn.
Parity gates (--full): BEFORE the timed region, on fresh state, EVERY stream of the batch at N=1 (128 spread over the batch per
rank at N>1) against the CPU oracle; AFTER it one more batch through the same context (carried decoder / biquad / slicer
state, FIFO four deep) with 64-256 streams against the oracle run over the TRUE concatenation of all batches the context has
seen, in their order (config.parity_after_timed*).  In every run: the discriminator's self-check counters (config.atan_*:
samples decided by the exact slow path / differing from this host's libm; the library compares them at every drain).  A
mismatch in any of them fails the run.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak (MI355X_MICROARCH.md)
SAMPLES_PER_BLOCK = 32768


def usable_cores() -> int:
    """Host threads this process may really use: affinity mask, capped by the cgroup CPU quota of the container."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    for path in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            txt = open(path).read().split()
            if path.endswith("cpu.max"):
                if txt[0] != "max":
                    n = min(n, max(1, int(float(txt[0]) / float(txt[1]) + 0.5)))
            else:
                q = int(txt[0])
                per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
                if q > 0:
                    n = min(n, max(1, int(q / per + 0.5)))
            break
        except Exception:
            continue
    return n


def cpu_baseline(iq_sample: np.ndarray, types: int, thresh: int, budget_s: float, all_cores: bool = True):
    """Time the reference CPU path, 1 thread, on a bounded sample of the same workload.

    kind "reference": the real reference hot path (oracle/_ref/ref_driver, compiled from /root/reference
    in the build container) -- used when the binary travelled with the tree; else kind "port": the C
    restatement oracle/tfrec_oracle.c (proven equal to the reference by tests/golden)."""
    from oracle import oracle as O

    n_streams = iq_sample.shape[0]
    samples_per_stream = iq_sample.shape[1] // 2
    # port
    t0 = time.perf_counter()
    done = 0
    for s in range(n_streams):
        o = O.Oracle(types, thresh, 0, quiet=True)
        o.process(iq_sample[s])
        o.close()
        done += 1
        if time.perf_counter() - t0 > budget_s:
            break
    t_port = time.perf_counter() - t0
    port = done * samples_per_stream / t_port / 1e6
    res = dict(value=round(port, 3), unit="MSamples/s", cores=1, kind="port",
               sample="%d streams x %d blocks of the bench batch, oracle/tfrec_oracle.c, 1 thread" % (
                   done, samples_per_stream // SAMPLES_PER_BLOCK))
    if os.path.exists(O.REF_DRIVER):
        with tempfile.TemporaryDirectory() as tmp:
            p = os.path.join(tmp, "s.iq")
            k = max(1, min(n_streams, done))
            np.ascontiguousarray(iq_sample[:k]).tofile(p)  # streams back to back: one long stream for the reference
            try:
                out = subprocess.run([O.REF_DRIVER, "time", "%x" % types, str(thresh), "0", p, "1"],
                                     capture_output=True, text=True, check=True, timeout=600)
                line = [ln for ln in out.stderr.splitlines() if ln.startswith('{"seconds"')][-1]
                r = json.loads(line)
                res = dict(value=round(r["msps"], 3), unit="MSamples/s", cores=1, kind="reference",
                           sample="%d streams x %d blocks of the bench batch concatenated, real reference hot path "
                                  "(oracle/_ref/ref_driver, g++ -O3 -ffast-math as the reference Makefile), 1 thread"
                                  % (k, samples_per_stream // SAMPLES_PER_BLOCK),
                           port_value=round(port, 3))
            except Exception as e:  # keep the port number
                res["reference_error"] = str(e)[:200]
    if not all_cores:
        return res
    # (ii) of SURVEY 8(d): one stream per thread over all host cores (OpenMP inside the C restatement)
    try:
        ncpu = usable_cores()
        a_ = np.ascontiguousarray(iq_sample)
        n_jobs = max(256, 32 * ncpu)  # about a second of work on every thread
        dt = O.lib().orc_time_many(types, thresh, 0, a_.ctypes.data, a_.strides[0], a_.shape[1], n_streams, n_jobs, ncpu)
        res["all_cores"] = dict(value=round(n_jobs * samples_per_stream / dt / 1e6, 1), unit="MSamples/s", cores=ncpu,
                                kind="port", sample="%d streams x %d blocks, one receiver per stream, %d threads (of %d "
                                "logical CPUs; affinity / cgroup quota of this container)" % (
                                    n_jobs, samples_per_stream // SAMPLES_PER_BLOCK, ncpu, os.cpu_count() or 1))
    except Exception as e:
        res["all_cores_error"] = str(e)[:200]
    return res


# ---- the algorithmic instruction floor of the path (SURVEY 8d "state both numbers"; derivation: DESIGN.md section 3)
# Wave instructions the REFERENCE's arithmetic needs when every operation runs 64 lanes wide at one wave instruction per
# SIMD and quad-cycle -- no control flow, no loads, no serial chain: what an ideal lane-parallel evaluation would issue.
#   per complex INPUT sample:  9 packed FMAs (8 taps at 1/2 rate + 20 taps at 1/4 rate, I and Q per v_pk_fma_f32:
#                              dsp_stuff.cpp:184-198, 213-226 -- the per-tap >>16 forbids folding symmetric taps) + 2 byte
#                              conversions + 0.25 x (2 conversions back, |I|+|Q| > thresh: 3)                          = 12.25
#   per decimated sample inside a TFA_2-family window (union of the three): fm_dev, dsp_stuff.cpp:284-292 = 6 fp64 for the
#                              cross terms + atan2 (one division ~ 8, odd degree-21 polynomial 12, octant fix-up 6) + scale
#                              and truncate 2                                                                         = 34
#   per in-window sample of ONE TFA_2-family chain: iir2::step 9 fp64 (dsp_stuff.cpp:47-56) + 2 conversions + slicer
#                              compares / threshold updates (tfa2.cpp:363-412) 8                                       = 19
#   per in-window sample of TFA_1: fm_dev_nrzs 3 + peak detector 4 + pulse test 3 (tfa1.cpp:152-178)                   = 10
#   per in-window sample of WHB: fm_dev_nrzs 3 + conversion 1 + iir 9 + (int) 1 + 0.5*dev and iir_avg 10 (while unsynced)
#                              + (int), two compares, spacing test 4 (whb.cpp:651-664)                                 = 28
# duty = the fraction of decimated samples inside a window of the chain, measured on the benchmark batch
# (TFREC_AMD_DEBUG_WINHIST=1: profiles/r04_winhist.txt); bits, decoders and CRCs are per telegram: negligible.
ALG_OPS = {"front": 12.25, "fm_dev": 34.0, "tfa2_chain": 19.0, "tfa1": 10.0, "whb": 28.0}
ALG_DUTY = {"tfa1": 0.457, "tfa2": 0.455, "tfa3": 0.469, "tx22": 0.472, "whb": 0.463}  # profiles/r04_winhist.txt
SIMDS, CLOCK_GHZ = 1024, 2.36  # (measured under load: profiles/r05_clocks_power.txt)


def algorithmic_floor_ms(n_streams: int, n_blocks: int, types: int) -> dict:
    n_in = float(n_streams) * n_blocks * SAMPLES_PER_BLOCK
    n_dec = n_in / 4
    lane_ops = ALG_OPS["front"] * n_in
    fam = [k for k, bit in (("tfa2", 1), ("tfa3", 2), ("tx22", 3)) if types & (1 << bit)]
    if fam:
        lane_ops += ALG_OPS["fm_dev"] * n_dec * max(ALG_DUTY[k] for k in fam)
        lane_ops += sum(ALG_OPS["tfa2_chain"] * n_dec * ALG_DUTY[k] for k in fam)
    if types & 1:
        lane_ops += ALG_OPS["tfa1"] * n_dec * ALG_DUTY["tfa1"]
    if types & 0x20:
        lane_ops += ALG_OPS["whb"] * n_dec * ALG_DUTY["whb"]
    wave_insts = lane_ops / 64
    return {"wave_instructions": round(wave_insts), "front_end_share": round(ALG_OPS["front"] * n_in / lane_ops, 3),
            "ms": round(wave_insts * 4 / (SIMDS * CLOCK_GHZ * 1e9) * 1e3, 4)}


def alg_bytes_ms(n_streams, n_blocks, rate):
    """the HBM floor: 2 B per complex input sample at the 8 TB/s peak"""
    return round(2.0 * n_streams * n_blocks * SAMPLES_PER_BLOCK * rate / (HBM_PEAK_GBS * 1e9) * 1e3, 4)


def a_steps_in_profile(root, ptag):
    """launches of the front end in the committed kernel trace = batches it covers"""
    try:
        for ln in open(os.path.join(root, "profiles", ptag + "_kernel_stats.txt")):
            if "frontend_kernel" in ln:
                return int(ln.split()[-4])
    except Exception:
        pass
    return None


DUMP_LIMIT_BYTES = 64 * 10 ** 6  # every file of a dump together, .npy headers included


def dump_outputs(out_dir: str, events: np.ndarray) -> dict:
    """The events of one drain as DIR/events_<field>.npy, one row per event in drain order (stream, slot, seq): every integer
    field as float64 (exact below 2^53), rdata as float32 [n, 64].  Past DUMP_LIMIT_BYTES a fixed sample of rows (seed 0) is
    written, in drain order, with its row numbers in events_row.npy."""
    n = len(events)
    scalars = [f for f in events.dtype.names if f != "rdata"]
    row_bytes = 8 * (len(scalars) + 1) + 4 * events.dtype["rdata"].shape[0]
    keep = max(1, (DUMP_LIMIT_BYTES - 16 * 1024) // row_bytes)
    rows = np.arange(n) if n <= keep else np.sort(np.random.default_rng(0).choice(n, keep, replace=False))
    sel = events[rows]
    os.makedirs(out_dir, exist_ok=True)
    for f in scalars:
        col = sel[f].astype(np.int64)
        assert np.all(np.abs(col) < (1 << 53)), "events_%s: not exact in float64" % f
        np.save(os.path.join(out_dir, "events_%s.npy" % f), col.astype(np.float64))
    np.save(os.path.join(out_dir, "events_rdata.npy"), sel["rdata"].astype(np.float32))
    np.save(os.path.join(out_dir, "events_row.npy"), rows.astype(np.float64))
    return {"dir": out_dir, "events": n, "events_written": len(rows), "sampled": len(rows) < n}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--streams", type=int, default=1024, help="streams per GPU")
    ap.add_argument("--blocks", type=int, default=48, help="65536-byte blocks per stream per step")
    ap.add_argument("--types", type=lambda x: int(x, 16), default=0x2F)
    ap.add_argument("--thresh", type=int, default=500)
    ap.add_argument("--unique", type=int, default=0,
                    help="distinct synthetic streams to generate per GPU, tiled over the batch (0 = every stream distinct)")
    ap.add_argument("--cpu-budget", type=float, default=12.0,
                    help="--full: upper bound in seconds for each single-thread leg of the CPU baseline (0 = skip)")
    ap.add_argument("--parity-streams", type=int, default=-1,
                    help="--full: streams of the first batch checked against the CPU oracle: -1 = all at N=1, 128 spread over "
                         "the batch per rank at N>1; 0 = none.  Unless 0, every run submits that batch before the warm-up")
    ap.add_argument("--parity-after-streams", type=int, default=0,
                    help="--full: streams of the batch AFTER the timed region checked against the oracle continued over all "
                         "repetitions of the input (0 = 256 on runs of up to 32 batches, down to 64 on long ones; a quarter of "
                         "it per rank at N>1; needs --parity-streams != 0)")
    ap.add_argument("--dist-backend", choices=("nccl", "gloo"), default="nccl",
                    help="backend of the barrier / scalar reduces at N>1 (the data path has no collective)")
    ap.add_argument("--same-device", action="store_true", help="tests: every rank uses cuda:0")
    ap.add_argument("--h2d-steps", type=int, default=4, help="--full: batches of the PCIe-inclusive leg (0 = skip; N=1 only)")
    ap.add_argument("--no-extra-configs", action="store_true",
                    help="--full: skip the short secondary measurements of the other BASELINE configs (N=1 only)")
    ap.add_argument("--depth", type=int, default=4, help="batches kept in the submit/drain FIFO (1..4)")
    ap.add_argument("--bg-traffic-gb", type=float, default=0.0,
                    help="EXPERIMENT (what binds?): beside every batch, a device-to-device copy of this many GB of HBM traffic (half read, "
                         "half written, coalesced) on a stream of its own; the line then carries config.bg_traffic_gb and is not a result")
    ap.add_argument("--distinct-batches", type=int, default=3,
                    help="distinct synthetic batches (own seeds) the steps rotate through: A, B, C, A, ...  A stream never sees "
                         "the same block twice in a row (engine.cpp:63-93), and with 3 batches over the library's 4 buffer sets "
                         "every set holds every batch in turn: a stale buffer cannot pass the gate behind the timed region")
    ap.add_argument("--experiments", action="store_true",
                    help="A/B sessions only: load libtfrec_amd_exp.so (environment knobs compiled in, csrc/knobs.h) instead of the "
                         "product library; the line then carries config.library = 'experiments' and is not a result")
    ap.add_argument("--input-10x", action="store_true",
                    help="BASELINE config 5 instead of config 2: 15.36 MS/s input through the 10:1 front end "
                         "(secondary measurement; the default line stays config 2)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the flush events the last timed step drained (rank 0) to DIR/events_<field>.npy "
                         "(float64; rdata float32), at most 64 MB in all: the outputs of two builds can be compared file by file")
    ap.add_argument("--full", action="store_true",
                    help="also run what the headline figure does not need: the parity gates against the CPU oracle before and "
                         "after the timed region, the CPU baseline, the PCIe-inclusive leg and the other configurations")
    a = ap.parse_args()
    if a.steps < 1:
        sys.exit("bench.py: --steps must be >= 1")
    rate = 10 if a.input_10x else 1

    if a.gpus < 1:
        sys.exit("bench.py: --gpus must be >= 1")
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # plain `python bench.py --gpus N`: launch the N ranks ourselves (one process per GPU, as the driver's
        # torch.distributed.run command line does) instead of silently measuring one rank
        import socket

        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(a.gpus),
               "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
        sys.exit(subprocess.call(cmd))

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != a.gpus:  # never report a line for another job size than the one asked for
        sys.exit("bench.py: --gpus %d but %d rank(s) were launched (WORLD_SIZE)" % (a.gpus, world))

    import torch
    import torch.distributed as dist

    from tfrec_amd import api, shard, synth

    dev_index = 0 if a.same_device else local_rank
    torch.cuda.set_device(dev_index)
    dev = torch.device("cuda", dev_index)
    if world > 1:
        if a.dist_backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group("gloo")
        if dist.get_world_size() != a.gpus:
            sys.exit("bench.py: %d ranks met at the rendezvous, --gpus %d" % (dist.get_world_size(), a.gpus))
    red_dev = dev if (world > 1 and a.dist_backend == "nccl") else None  # where the reduced scalars live

    n_streams, n_blocks = a.streams, a.blocks
    row = n_blocks * api.BLOCK_BYTES * rate
    # ---- synthetic input: distinct seeds per rank; generate `unique` streams and tile them over the batch
    # (the input depends on the arguments alone, never on the host: the same command line gives the same batches everywhere)
    unique = a.unique if a.unique > 0 else n_streams
    t0 = time.perf_counter()
    n_distinct = max(1, a.distinct_batches)
    if rate != 1:
        unique = min(unique, 32)
    # batch b of the rotation: its own seed (1000 + rank + 7919 b); batch q of the run is hosts[q % n_distinct]
    hosts = []
    for b in range(n_distinct):
        if rate == 1:
            hosts.append(synth.gen_batch(1000 + rank + 7919 * b, rank * n_streams, unique, n_blocks))
        else:
            hosts.append(np.stack([synth.gen_stream(1000 + rank + 7919 * b, rank * n_streams + s, n_blocks, 0x1F, 256, rate_mult=rate)
                                   for s in range(unique)]))
    host = hosts[0]
    t_gen = time.perf_counter() - t0
    import zlib
    input_crc = shard.gather_ints(zlib.crc32(host[0].tobytes()), red_dev)  # every rank generates its own streams
    d_batches = []
    for hb in hosts:
        d_b = torch.empty((n_streams, row), dtype=torch.uint8, device=dev)
        d_u = torch.from_numpy(hb).to(dev)
        for s0 in range(0, n_streams, unique):
            k = min(unique, n_streams - s0)
            d_b[s0:s0 + k].copy_(d_u[:k])
        del d_u
        d_batches.append(d_b)
    torch.cuda.synchronize(dev)
    seq = [0]  # batches this context has been given so far: the next one is number seq[0] of the rotation

    def next_batch():
        b = d_batches[seq[0] % n_distinct]
        seq[0] += 1
        return b

    r = api.Receiver(n_streams, a.types, a.thresh, 0, device=dev_index, max_blocks=n_blocks, timing=True,
                     max_events=max(4096, n_streams * 256), input_10x=a.input_10x, experiments=a.experiments)

    # ---- parity gate (fresh context state): GPU events of the first batch == oracle events, stream by stream.  A plain run
    # submits and drains the same batch without the comparison: the warm-up and the timed steps start from the same state
    parity_ok = None
    parity_n = 0
    if a.parity_streams != 0:
        r.submit(next_batch())  # batch 0 of the rotation = hosts[0]
        first = r.drain()
    if a.parity_streams != 0 and a.full:
        from oracle import oracle as O
        want_n = a.parity_streams if a.parity_streams > 0 else (n_streams if world == 1 else 128)
        want_n = min(want_n, n_streams)
        # spread over the batch: first, middle, last (stream s of the batch is distinct stream s % unique)
        pick = np.unique(np.linspace(0, n_streams - 1, want_n).round().astype(np.int64))
        parity_n = len(pick)
        src = np.unique(pick % unique)
        if rate == 1:
            orc = dict(zip(src.tolist(), O.process_many(host[src], a.types, a.thresh, 0)))
        else:
            orc = {}
            for u in src.tolist():
                o = O.Oracle(a.types, a.thresh, 0)
                o.process_s16(O.decim10(host[u]))
                orc[u] = np.array([(e[0], e[7], e[2], e[3], e[4], e[1], e[6], np.frombuffer(e[5], np.uint8))
                                   for e in o.events_full()], dtype=O.ORC_EVENT_DTYPE)
        minb = np.array([10, 7, 7, 7, 11])
        gs, gm = api.events_canon(first)
        bounds = np.searchsorted(gs, np.arange(n_streams + 1))  # the drain orders by (stream, slot, seq)
        parity_ok = True
        for sidx in pick.tolist():
            e = orc[sidx % unique]
            # default mode reports the flushes that can print (include/tfrec_amd.h TFREC_AMD_F_ALL_FLUSHES)
            keep = (e["byte_cnt"] >= minb[e["slot"]]) & ~((e["slot"] == 3) & (e["byte_cnt"] >= 64)) & ~((e["slot"] == 4) & (e["byte_cnt"] > 60))
            wm = O.canon(e[keep])
            wm = wm[np.lexsort((wm[:, 1], wm[:, 0]))]
            g = gm[bounds[sidx]:bounds[sidx + 1]]
            g = g[np.lexsort((g[:, 1], g[:, 0]))]
            if g.shape != wm.shape or not np.array_equal(g, wm):
                parity_ok = False
                print("PARITY FAILURE on rank %d stream %d" % (rank, sidx), file=sys.stderr)
                break
        if shard.sum_over_ranks(0 if parity_ok else 1, red_dev) != 0:
            sys.exit(3)

    # Submits and drains form a FIFO (include/tfrec_amd.h, TFREC_AMD_FIFO_DEPTH): up to `depth` batches are queued before
    # the oldest one's events are drained, so the GPU never waits for the host's copy + sort of a batch and the stages
    # of consecutive batches overlap.  Exactly n_steps batches are submitted and drained inside run().
    depth = max(1, min(a.depth, api.FIFO_DEPTH))

    bg = None
    if a.bg_traffic_gb > 0:
        n_bg = int(a.bg_traffic_gb * 1e9 / 2)
        bg = (torch.empty(n_bg, dtype=torch.uint8, device=dev), torch.empty(n_bg, dtype=torch.uint8, device=dev), torch.cuda.Stream(device=dev))

    # host side of a step (ms): every submit's duration, the longest time from a drain's return to the next drain's call, and every
    # pause of Python's garbage collector inside run() -- a stalled host shows up here, not in the kernels' intervals (round 6:
    # hipMemcpyAsync of the drain's copy blocked submits 6 and 7 after every synchronize, profiles/r06_host_stalls.txt)
    host_ms = {"submit_max": 0.0, "between_drains_max": 0.0, "gc_pauses": []}
    gc_t = [0.0]

    def gc_cb(phase, info):
        if phase == "start":
            gc_t[0] = time.perf_counter()
        else:
            host_ms["gc_pauses"].append([info.get("generation"), round((time.perf_counter() - gc_t[0]) * 1e3, 3)])

    last_ev = [None]  # the events the most recent drain returned: what a caller of the path receives for its last step

    def run(n_steps, collect, src=None, stamps=None):
        n_ev = 0
        queued = 0
        t_ret = None
        for k in range(n_steps):
            while queued < n_steps and queued - k < depth:
                ts = time.perf_counter()
                r.submit(next_batch() if src is None else src)
                if stamps is not None:
                    host_ms["submit_max"] = max(host_ms["submit_max"], (time.perf_counter() - ts) * 1e3)
                    host_ms.setdefault("submit_ms", []).append(round((time.perf_counter() - ts) * 1e3, 3))
                queued += 1
                if bg is not None:
                    with torch.cuda.stream(bg[2]):
                        bg[1].copy_(bg[0], non_blocking=True)
            if stamps is not None and t_ret is not None:
                host_ms["between_drains_max"] = max(host_ms["between_drains_max"], (time.perf_counter() - t_ret) * 1e3)
            last_ev[0] = r.drain()
            n_ev += len(last_ev[0])
            t_ret = time.perf_counter()
            if stamps is not None:
                stamps.append(time.perf_counter())
            if collect is not None:
                t = r.timings()  # HIP events recorded on the streams the kernels of the drained batch ran on
                for kk, v in t.items():
                    collect.setdefault(kk, []).append(v)
        return n_ev

    import gc
    run(a.warmup, None)
    kt = {}
    torch.cuda.synchronize(dev)
    if world > 1:
        dist.barrier()
    gc.callbacks.append(gc_cb)
    t0 = time.perf_counter()
    stamps = [t0]
    n_events = run(a.steps, kt, stamps=stamps)
    torch.cuda.synchronize(dev)
    gc.callbacks.remove(gc_cb)
    if world > 1:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    elapsed = shard.max_over_ranks(elapsed, red_dev)
    dumped = dump_outputs(a.dump_outputs, last_ev[0]) if a.dump_outputs and rank == 0 else None

    # ---- parity of the state the timed region ran in (carried decoder / biquad / slicer / FIR state, FIFO `depth` deep): one
    # more batch through the same context, a spread of its streams against the oracle CONTINUED over every repetition of
    # the input this context has seen (gate + warm-up + timed steps + this one): decoder.cpp:118-122, tfa2.cpp:325-334,
    # whb.cpp:616-623 carry state from block to block exactly like this
    parity_after = None
    parity_after_n = 0
    if a.full and a.parity_streams != 0 and rate == 1:
        from oracle import oracle as O
        reps_before = seq[0]  # gate + warm-up + timed steps
        assert reps_before == (1 if parity_ok is not None else 0) + a.warmup + a.steps
        r.submit(next_batch())
        last = r.drain()
        # (the oracle has to run every checked stream over ALL repetitions: 256 streams on the driver's short line, fewer on long ones)
        after_n = a.parity_after_streams if a.parity_after_streams > 0 else max(64, min(256, 256 * 32 // max(1, reps_before)))
        want_n = min(n_streams, after_n if world == 1 else max(8, after_n // 4))
        pick = np.unique(np.linspace(0, n_streams - 1, want_n).round().astype(np.int64))
        src = np.unique(pick % unique)
        t_or = time.perf_counter()
        # the TRUE concatenation: batch q of the rotation is hosts[q % n_distinct], every one of the reps_before + 1 in order
        parts_ = [hb[src] for hb in hosts]
        orc = dict(zip(src.tolist(), O.process_parts([parts_[q % n_distinct] for q in range(reps_before + 1)], a.types, a.thresh, 0,
                                                     keep_from=reps_before)))
        t_or = time.perf_counter() - t_or
        minb = np.array([10, 7, 7, 7, 11])
        gs, gm = api.events_canon(last)
        bounds = np.searchsorted(gs, np.arange(n_streams + 1))
        parity_after = True
        for sidx in pick.tolist():
            e = orc[sidx % unique]
            keep = (e["byte_cnt"] >= minb[e["slot"]]) & ~((e["slot"] == 3) & (e["byte_cnt"] >= 64)) & ~((e["slot"] == 4) & (e["byte_cnt"] > 60))
            wm = O.canon(e[keep])
            wm = wm[np.lexsort((wm[:, 1], wm[:, 0]))]
            g = gm[bounds[sidx]:bounds[sidx + 1]]
            g = g[np.lexsort((g[:, 1], g[:, 0]))]
            if g.shape != wm.shape or not np.array_equal(g, wm):
                parity_after = False
                print("PARITY FAILURE after the timed region on rank %d stream %d" % (rank, sidx), file=sys.stderr)
                break
        parity_after_n = len(pick)
        if shard.sum_over_ranks(0 if parity_after else 1, red_dev) != 0:
            sys.exit(5)
    step_ms = np.diff(np.array(stamps)) * 1e3  # time between consecutive drains of this rank
    events_all = shard.sum_over_ranks(n_events, red_dev)

    # ---- the discriminator's self check over everything this context processed: samples decided by the
    # exact slow path, and how many of the logged decisions differ from this host's libm (the reference's arithmetic)
    fm = r.fm_stats()
    fm_bad = shard.sum_over_ranks(fm["host_mismatch"], red_dev)

    mem_tables = r.memory()  # before the PCIe leg: tfrec_amd_submit_host grows one input staging buffer per FIFO set on demand
    # ---- PCIe-inclusive leg: the same batch from page-locked host memory through the FIFO (never `value`)
    h2d = None
    if a.full and a.h2d_steps > 0 and world == 1:
        try:
            import ctypes as C
            L = r.L
            L.tfrec_amd_host_alloc.restype = C.c_void_p
            L.tfrec_amd_host_alloc.argtypes = [C.c_size_t]
            L.tfrec_amd_host_free.argtypes = [C.c_void_p]
            pin = L.tfrec_amd_host_alloc(n_streams * row)
            if pin:
                hbuf = np.ctypeslib.as_array(C.cast(pin, C.POINTER(C.c_uint8)), shape=(n_streams, row))
                for s0 in range(0, n_streams, unique):
                    k = min(unique, n_streams - s0)
                    hbuf[s0:s0 + k] = host[:k]
                run(2, None, src=hbuf)  # (every submit reads the same pinned batch: nothing writes to it)
                th = time.perf_counter()
                run(a.h2d_steps, None, src=hbuf)
                dt = time.perf_counter() - th
                h2d = dict(value=round(n_streams * n_blocks * SAMPLES_PER_BLOCK * rate * a.h2d_steps / dt / 1e6, 3),
                           unit="MSamples/s", ms_per_step=round(dt / a.h2d_steps * 1e3, 3), steps=a.h2d_steps,
                           pcie_gbs=round(n_streams * row * a.h2d_steps / dt / 1e9, 2),
                           how="tfrec_amd_submit_host from one page-locked batch, FIFO depth %d" % depth)
                del hbuf
                L.tfrec_amd_host_free(pin)
        except Exception as e:  # the leg is informative: never fail the line for it
            h2d = dict(error=str(e)[:200])

    # ---- secondary, short measurements of the other single-GPU configurations of BASELINE.json (never `value`): same
    # method (input resident in HBM, FIFO of depth 4, parity gate on fresh state against the oracle)
    extra = {}
    if a.full and world == 1 and not a.no_extra_configs and not a.input_10x and (n_streams, n_blocks, a.types) == (1024, 48, 0x2F):
        from oracle import oracle as O

        def side(name, xs, xb, xt, x10, steps, xthresh=None, gen=None, cpu_ref=False, want_kernels=()):
            """One secondary leg: its own context, parity gate on fresh state (every distinct stream against the oracle),
            then `steps` timed batches through the FIFO.  gen(xu, xb) -> the leg's distinct streams (default: the recipe of the
            main line, seed 2000); xthresh: -t of the leg; cpu_ref: time the real reference's CPU path on the same stream."""
            xr = 10 if x10 else 1
            xth = a.thresh if xthresh is None else xthresh
            xu = min(xs, 16)
            if gen is not None:
                xh = gen(xu, xb)
            elif x10:
                xh = np.stack([synth.gen_stream(2000, k, xb, 0x1F, 256, rate_mult=10) for k in range(xu)])
            else:
                xh = synth.gen_batch(2000, 0, xu, xb)
            xd = torch.empty((xs, xb * api.BLOCK_BYTES * xr), dtype=torch.uint8, device=dev)
            xdu = torch.from_numpy(xh).to(dev)
            for s0 in range(0, xs, xu):
                xd[s0:s0 + min(xu, xs - s0)].copy_(xdu[:min(xu, xs - s0)])
            # the leg's second batch: the same recordings given to the NEXT stream each (stream s gets stream s - 1's), so that no
            # stream sees the same block twice in a row; the steps alternate between the two
            xrot = (xd, torch.roll(xd, 1, 0))
            xq = [0]

            def xnext():
                xq[0] += 1
                return xrot[(xq[0] - 1) & 1]

            with api.Receiver(xs, xt, xth, 0, device=dev_index, max_blocks=xb, max_events=max(4096, xs * 256),
                              input_10x=x10, timing=bool(want_kernels), experiments=a.experiments) as xr_:
                xr_.submit(xnext())
                first = xr_.drain()
                ok = True
                minb = {0: 10, 1: 7, 2: 7, 3: 7, 4: 11}
                n_want = 0
                for k in range(xu):  # every distinct stream of the leg's batch
                    o = O.Oracle(xt, xth, 0)
                    if x10:
                        o.process_s16(O.decim10(xh[k]))
                    else:
                        o.process(xh[k])
                    want = sorted(e for e in o.events_full() if e[2] >= minb[e[0]] and not (e[0] == 3 and e[2] >= 64)
                                  and not (e[0] == 4 and e[2] > 60))
                    n_want += len(want)
                    ok = ok and sorted(api.event_tuples_full(first, k)) == want
                    if xth == 0:  # auto threshold (fm_demod.cpp:58-73): where it ended is part of the result
                        ok = ok and xr_.thresh(k) == o.thresh()
                q = 0
                for k in range(3):  # warm-up
                    xr_.submit(xnext())
                    xr_.drain()
                torch.cuda.synchronize(dev)
                tx = time.perf_counter()
                kk = {}
                for k in range(steps):
                    while q < steps and q - k < depth:
                        xr_.submit(xnext())
                        q += 1
                    xr_.drain()
                    if want_kernels:
                        tm = xr_.timings()
                        for nm in want_kernels:
                            kk.setdefault(nm, []).append(tm[nm])
                torch.cuda.synchronize(dev)
                dt = time.perf_counter() - tx
            xalg = algorithmic_floor_ms(xs, xb, xt) if not x10 else None
            del xrot
            extra[name] = dict(streams=xs, blocks=xb, types_mask=xt, thresh=xth, input_10x=x10, steps=steps, parity_ok=ok, distinct_batches=2,
                               parity_streams_checked=xu, parity_events_checked=n_want,
                               ms_per_step=round(dt / steps * 1e3, 4),
                               hbm_frac=round(2.0 * xs * xb * SAMPLES_PER_BLOCK * xr / (dt / steps) / 1e9 / HBM_PEAK_GBS, 4),
                               algorithmic_valu_floor_ms=(xalg["ms"] if xalg else None),
                               value=round(xs * xb * SAMPLES_PER_BLOCK * xr * steps / dt / 1e6, 1), unit="MSamples/s")
            for nm, v in kk.items():
                extra[name][nm] = round(float(np.mean(v)), 4)
            if cpu_ref and a.cpu_budget > 0:  # (64 streams of the leg's recipe back to back: seconds, not milliseconds, of CPU work)
                extra[name]["cpu_baseline"] = cpu_baseline(synth.gen_batch(2000, 0, 64, xb), xt, xth, a.cpu_budget, all_cores=False)
            return extra[name]

        def noisy_tail(xu, xb):
            """the main recipe with the LAST distinct stream at noise sigma 16 LSB: |I| + |Q| of the decimated samples stays
            above -t 500, the stream's trigger windows never close (duty 1.0): the worst case of every per-stream serial chain"""
            xh = synth.gen_batch(2000, 0, xu, xb)
            xh[xu - 1] = synth.gen_stream(2000, xu - 1, xb, 0x1F, 16 * 256)
            return xh

        try:
            # the reference's own operating points ...
            side("configs[0]: one 1.536 MS/s stream, TFA_1 only (-T 1), auto threshold (the reference's default flags)", 1, 48, 0x01,
                 False, 30, xthresh=0, cpu_ref=True)
            side("configs[1]: one 1.536 MS/s stream, TFA_1/2/3 (-T 7)", 1, 48, 0x07, False, 30)
            # (512 streams: 16 GB of input per batch -- with 256 the 10:1 stage hides behind the demodulator chains, whose length
            # does not shrink with the batch; BASELINE.json names no stream count for this configuration)
            side("configs[4]: 512 streams at 15.36 MS/s through the 10:1 front end, all five protocols", 512, 48, 0x2F, True, 8)
            # the streaming kernels without the WHB chain's serial floor: configs[2]'s batch with the demodulators of configs[1]
            side("1024 streams x TFA_1/2/3 (-T 7): no WHB chain", 1024, 48, 0x07, False, 12)
            # ... the two ends of the trigger duty cycle: never triggered (the front end and the
            # window scan are all that runs -- the streaming kernel's own HBM fraction inside the whole path) ...
            side("1024 streams x 5 protocols, -t 30000: never triggered (front end only)", 1024, 48, 0x2F, False, 12, xthresh=30000,
                 want_kernels=("frontend_ms",))
            # ... and the tail case: one stream in 16 (64 of 1024) with its windows open all the time (duty 1.0): every
            # per-stream serial chain of the batch is as long as its longest stream
            t_ = side("1024 streams x 5 protocols, 64 of them at trigger duty 1.0 (noise above -t 500)", 1024, 48, 0x2F, False, 12,
                      gen=noisy_tail, want_kernels=("whb_verify_ms", "whb_demod_ms", "coop_slicer_ms", "tfa1_coop_slicer_ms"))
            t_["whb_verify_over_period"] = round(t_["whb_verify_ms"] / t_["ms_per_step"], 3)
        except Exception as e:  # informative legs: never fail the line for them
            extra["error"] = str(e)[:200]

    samples_per_step_gpu = n_streams * n_blocks * SAMPLES_PER_BLOCK * rate  # complex INPUT samples
    total_samples = samples_per_step_gpu * a.steps * world
    value = total_samples / elapsed / 1e6

    if rank == 0:
        # (whb_decode / whb_commit: since they run in the tail of whb_demod_kernel those two timing fields are empty)
        kms = {k[:-3] + "_kernel": float(np.mean(v)) for k, v in kt.items()
               if k not in ("chains_ms", "total_ms", "whb_decode_ms", "whb_commit_ms")}
        dom_name = max(kms, key=kms.get)  # (replaced below by the kernel that is longest ALONE on the chip, where profiled)
        dom_ms = kms[dom_name]
        alg_bytes = 2.0 * samples_per_step_gpu  # 2 B per complex input sample, one launch = one batch
        achieved = alg_bytes / (dom_ms * 1e-3) / 1e9 if dom_ms > 0 else 0.0
        # What this run cannot measure itself comes from the builder's committed rocprofv3 runs of the SAME command
        # (profiles/run_round3.sh; named in `profiles` / `traffic_source`): the kernel's average duration in the kernel
        # trace, HBM bytes per launch (separate FETCH_SIZE / WRITE_SIZE passes, corrected as MI355X_MICROARCH.md prescribes
        # and calibrated per access pattern), and the batch's VALU instruction mix for the VALU-issue roof.
        traffic = traffic_total = prof_ms = traffic_source = None
        valu = None
        same_workload = (n_streams, n_blocks, a.types, rate) == (1024, 48, 0x2F, 1)
        ptag = next((t for t in ("r06_final", "r06_mid", "r05_final", "r05_mid", "r04_final", "r04_mid", "r03_final", "r03_mid")
                     if os.path.exists(os.path.join(ROOT, "profiles", t + "_traffic.json"))), None)
        chain_floor = fe_alone = chain_kernel = None
        utilisation = None
        if ptag and same_workload:
            try:  # the dominant kernel = the one with the longest duration ALONE on the chip (committed profile), timed live
                vj0 = json.load(open(os.path.join(ROOT, "profiles", ptag + "_valu.json")))["kernels"]
                alone = {}
                # (the timing field `whb_verify_ms` covers the WHB check, since round 6 whb_chain_kernel + whb_check_kernel)
                alias = {"whb_chain_kernel": "whb_verify_kernel", "whb_check_kernel": "whb_verify_kernel"}
                for kn, kv in vj0.items():
                    base = kn.split("<")[0]
                    base = alias.get(base, base)
                    alone[base] = max(alone.get(base, 0.0), kv.get("kernel_ms_alone") or 0.0)  # (template instances: the longest)
                cand_ = [kn for kn in sorted(alone, key=alone.get, reverse=True) if kn in kms and kms[kn] > 0]
                if cand_:
                    dom_name = cand_[0]
                    dom_ms = kms[dom_name]
                    achieved = alg_bytes / (dom_ms * 1e-3) / 1e9
            except Exception:
                pass
            try:
                tj = json.load(open(os.path.join(ROOT, "profiles", ptag + "_traffic.json")))
                traffic = tj["kernels"].get("whb_chain_kernel" if dom_name == "whb_verify_kernel" else dom_name, {}).get("hbm_bytes")
                traffic_total = tj.get("total_hbm_bytes_per_batch")
                traffic_source = "profiles/%s_traffic.json (builder's rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this command)" % ptag
            except Exception:
                pass
            try:  # "tfrec::frontend_kernel<false> ... calls total avg pct": the trace's average for the dominant kernel
                short = dom_name.replace("_kernel", "")
                cand = []
                for ln in open(os.path.join(ROOT, "profiles", ptag + "_kernel_stats.txt")):
                    f = ln.split()
                    # (the live interval `whb_verify` brackets whb_chain_kernel, whb_check_kernel and the redo launch: the same three here)
                    if len(f) >= 5 and (("tfrec::%s_kernel" % short) in ln or (short == "whb_verify" and (
                            "tfrec::whb_chain_kernel" in ln or "tfrec::whb_check_kernel" in ln or "whb_demod_kernel<true, true>" in ln))) and f[-4].isdigit():
                        cand.append((float(f[-3]), float(f[-2])))
                if cand:  # (several template instances of one kernel: all launches of a batch together)
                    calls = max(1, sum(1 for _ in cand))
                    prof_ms = round(sum(t for t, _ in cand) / 1e3 / (a_steps_in_profile(ROOT, ptag) or 1), 4)
            except Exception:
                pass
            try:
                vj = json.load(open(os.path.join(ROOT, "profiles", ptag + "_valu.json")))
                valu = {
                    "insts_per_batch": {k: int(v) for k, v in vj["per_batch"].items()},
                    "ns_per_instruction_per_simd": vj["ns_per_instruction_per_simd"],
                    "roof_ms": vj["valu_roof_ms"], "busy_ms_counters": vj["valu_busy_ms_counters"],
                    "salu_roof_ms": vj["salu_roof_ms"], "salu_busy_ms_counters": vj["salu_busy_ms_counters"],
                    "frac": round(vj["valu_roof_ms"] / (elapsed / a.steps * 1e3), 4),
                    "sum_of_kernel_ms_alone": vj["sum_of_kernel_ms_alone"],
                    "source": "profiles/%s_valu.json (builder's rocprofv3 --pmc passes of this command; NOT measured in this run)" % ptag,
                    "how": "VALU wave-instructions of one batch by class (rocprofv3 --pmc, profiles/%s_pmc_mix.txt) x the measured "
                           "time per instruction and SIMD (profiles/ubench/valu_issue.hip -> profiles/%s_valu_issue.jsonl: kernel time / "
                           "(instructions per wave x waves per SIMD), 1.6-2.1 ns = 4 cycles) / 1024 SIMDs; busy_ms_counters = "
                           "SQ_ACTIVE_INST_VALU x 4 cycles / (1024 SIMDs x 2.4 GHz), the same roof from the counters alone; frac = "
                           "roof_ms / ms_per_step; per kernel: profiles/%s_valu.json" % (ptag, ptag, ptag),
                }
                if vj.get("issue_roof_ms"):
                    utilisation = {
                        "issue_busy_ms": vj["issue_roof_ms"],
                        "issue_busy_over_period": round(vj["issue_roof_ms"] / (elapsed / a.steps * 1e3), 4),
                        "note": ("NOT a roofline: the sum over the batch's kernels (each measured alone) of SQ_ACTIVE_INST_ANY x 4 cycles / (1024 SIMDs "
                                 "x 2.36 GHz) = wave-quad-cycles with an instruction of any kind in flight = ~1.1 x (VALU + SALU wave instructions).  "
                                 "Rounds 1-4: the batch period equalled this sum within 1-5 percent.  Rounds 5 and 6 took a quarter of the instructions "
                                 "out (lane-per-step slicers; the WHB check a stream per lane: 312 -> 82 M; the WHB candidate walk) and the period "
                                 "followed by a third of that: the sum describes how full the SIMDs are, it is not a bound.  The period sits on the "
                                 "two serial per-stream WHB stages, each busy for the whole period on its stream (whb_demod_kernel<false>: one wave "
                                 "per stream, 2.2 ms alone, ~4.3 ms inside the batch; whb_chain_kernel: 3.2 ms alone, ~5 ms inside) and follows what "
                                 "makes their waves WAIT rather than what they issue (DESIGN.md section 3, 'What binds': 180 k same-address atomics per "
                                 "batch cost 25 percent, two more loads per step of whb_demod_kernel 20 percent).  No single resource is saturated.  "
                                 "What bounds the path nominally is in `roofline` (hbm_floor_ms, algorithmic_valu_floor_ms, chain_floor_ms); "
                                 "source profile: profiles/" + ptag + "_valu.json"),
                        "source": "profiles/%s_valu.json (builder's rocprofv3 --pmc passes; NOT measured in this run)" % ptag,
                    }
                # the serial floor: the dominant chain kernel ALONE on the chip (serial per stream; consecutive batches'
                # launches of it run one after the other) and the only kernel that streams the input, alone
                kj = vj.get("kernels", {})
                # (the longest single kernel alone: the serial per-stream chains -- the WHB check, the WHB demodulator -- are
                # launched once per batch and consecutive batches' launches run one after the other on their stream)
                chain_floor = max((v.get("kernel_ms_alone") or 0.0) for v in kj.values()) or None
                chain_kernel = max(kj, key=lambda k: kj[k].get("kernel_ms_alone") or 0.0) if kj else None
                fe_alone = next((v.get("kernel_ms_alone") for k, v in kj.items() if k.startswith("frontend_kernel")), None)
            except Exception:
                pass
        alg = algorithmic_floor_ms(n_streams, n_blocks, a.types) if rate == 1 else None
        period_ms = elapsed / a.steps * 1e3
        floors = [f for f in (chain_floor, alg["ms"] if alg else None, alg_bytes_ms(n_streams, n_blocks, rate)) if f]
        out = {
            "metric": "IQ MSamples/s through demod+decode (batched streams)",
            "value": round(value, 3),
            "unit": "MSamples/s",
            "n_gpus": world,
            "steps": a.steps,
            "warmup": a.warmup,
            "ms_per_step": round(elapsed / a.steps * 1e3, 4),
            "ms_min": round(float(step_ms.min()), 4), "ms_median": round(float(np.median(step_ms)), 4),
            "ms_max": round(float(step_ms.max()), 4),
            # without the steps in which the FIFO of `depth` batches fills and drains (the timed region starts and ends empty)
            "ms_per_step_steady": (round(float(step_ms[depth:-depth].mean()), 4) if len(step_ms) > 2 * depth + 2 else None),
            # (every step of a short run: where the FIFO's filling, a late host or a slow tail went)
            "step_ms": ([round(float(x), 3) for x in step_ms] if len(step_ms) <= 64 else None),
            "host_ms": {"submit_max": round(host_ms["submit_max"], 3), "between_drains_max": round(host_ms["between_drains_max"], 3),
                        "submit_ms": host_ms.get("submit_ms", [])[:64] if a.steps <= 64 else None, "gc_pauses": host_ms["gc_pauses"][:16], "gc_pause_total": round(sum(p for _, p in host_ms["gc_pauses"]), 3)},
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "int32+f32+f64",  # integer FIR (evaluated exactly in fp32 FMAs) and slicers, fp64 biquads + discriminator
            "data": "synthetic (tfrec_amd.synth, SURVEY App. C recipe; %d distinct streams per GPU%s)" % (
                unique, "" if unique == n_streams else " tiled over %d" % n_streams),
            "config": {
                "workload": ("configs[4]: %d batched 15.36 MS/s streams (10:1 front end) x %d blocks x protocols mask 0x%x, -t %d, per GPU"
                             if a.input_10x else
                             "configs[2]: %d batched 1.536 MS/s streams x %d blocks x protocols mask 0x%x, -t %d, per GPU")
                            % (n_streams, n_blocks, a.types, a.thresh),
                "streams_per_gpu": n_streams, "blocks_per_stream": n_blocks, "types_mask": a.types,
                "thresh": a.thresh, "parallelism": "streams sharded by index, no collective",
                # the steps rotate through this many distinct batches (own seeds); the gate behind the timed region runs the
                # oracle over their true concatenation
                "distinct_batches": n_distinct,
                "library": "experiments (csrc/knobs.h: NOT a result)" if a.experiments else "product (no environment knobs)",
                "events_per_step": n_events // max(1, a.steps), "parity_gate_streams": parity_n,
                "parity_ok": parity_ok, "gen_seconds": round(t_gen, 2),
                # the batch after the timed region (state carried over gate + warm-up + timed steps, FIFO `depth` deep)
                # against the oracle continued over the same repetitions of the input
                "parity_after_timed": parity_after, "parity_after_timed_streams": parity_after_n,
                "parity_after_timed_batches_carried": (reps_before if parity_after is not None else None),
                "atan_resolved": fm["resolved"], "atan_host_verified": fm["host_verified"],
                "atan_host_mismatch": fm_bad, "atan_undecidable": fm["undecidable"],
                # slow-path decisions beyond the per-submit log (62): exact by construction, but not compared with this host's libm
                "atan_unverified": fm["resolved"] - fm["host_verified"],
                "bg_traffic_gb": a.bg_traffic_gb if a.bg_traffic_gb > 0 else None,
                "dist_backend": a.dist_backend if world > 1 else None,
                "rank_input_crc32": input_crc, "events_all_ranks": events_all,
            },
            "roofline": {
                # (the timing interval `whb_verify` brackets the WHB check: whb_chain_kernel -- all but 0.1-0.3 ms of it -- then
                # whb_check_kernel and the redo launch, which normally returns at once)
                "bound": "hbm", "kernel": "whb_chain_kernel" if dom_name == "whb_verify_kernel" else dom_name,
                "achieved": round(achieved, 3), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "frac": round(achieved / HBM_PEAK_GBS, 5), "traffic": traffic, "traffic_source": traffic_source,
                # `kernel` is the kernel with the longest duration ALONE on the chip (a serial per-stream chain that does not
                # stream the input: its `frac` prices the batch's algorithmic bytes against ITS duration, as the contract asks);
                # the honest figure for the path is whole_path_frac = algorithmic bytes / batch period / peak
                "headline_frac": "whole_path_frac",
                # the dominant kernel's duration: live HIP events on its stream (includes its wait for the chip beside the
                # other streams' kernels) | average of the same kernel in the committed kernel trace, per batch
                "kernel_ms_hip_events": round(dom_ms, 4), "kernel_ms_profiles": prof_ms,
                "kernel_ms_covers": (["whb_chain_kernel", "whb_check_kernel", "whb_demod_kernel<true, true>"]
                                     if dom_name == "whb_verify_kernel" else [dom_name]),
                "profiles": ("profiles/%s_kernel_stats.txt" % ptag) if ptag and same_workload else None,
                "valu_profiled": valu,
                # ---- what binds (period / max(floors) = how far from the roof):
                #  hbm_floor_ms             2 B per input sample at 8 TB/s
                #  algorithmic_valu_floor_ms the reference's arithmetic, 64 lanes wide at one instruction per SIMD and quad-cycle
                #  chain_floor_ms           the dominant serial kernel alone on the chip (profiles)
                "hbm_floor_ms": alg_bytes_ms(n_streams, n_blocks, rate),
                "algorithmic_valu_floor_ms": alg["ms"] if alg else None,
                "algorithmic_valu_floor": alg,
                "chain_floor_ms": chain_floor, "chain_floor_kernel": chain_kernel,
                "period_over_max_floor": (round(period_ms / max(floors), 3) if floors else None),
                "frontend": ({"ms_alone": fe_alone, "frac": round(alg_bytes / (fe_alone * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                              "source": "profiles/%s_valu.json" % ptag} if fe_alone else None),
                "algorithmic_bytes_per_launch": alg_bytes,
                "whole_path_frac": round(alg_bytes / (elapsed / a.steps) / 1e9 / HBM_PEAK_GBS, 5),
                "traffic_total": traffic_total,
                "traffic_ratio": round(traffic_total / alg_bytes, 3) if traffic_total else None,
                "kernels_ms": {k: round(v, 4) for k, v in sorted(kms.items())},
                "gpu_ms_per_step": round(float(np.mean(kt.get("total_ms", [0.0]))), 4),
                "speculation_stats": r.stats(),
                "pipeline_streams": r.layout(),
                # device_bytes: what a context fed from device memory holds; with_host_staging: after the
                # PCIe leg, + FIFO-depth staging copies of the batch (tfrec_amd_submit_host) -- round 4's line reported only this
                "context_memory": dict(mem_tables, device_bytes_with_host_staging=r.memory()["device_bytes"]),
            },
        }
        if a.full and a.cpu_budget > 0 and world == 1 and rate == 1:
            out["cpu_baseline"] = cpu_baseline(host[: min(unique, 256)], a.types, a.thresh, a.cpu_budget)
        if h2d is not None:
            out["h2d_included"] = h2d
        if utilisation:
            out["utilisation"] = utilisation
        if extra:
            out["other_configs"] = extra
        if dumped is not None:
            out["dump_outputs"] = dumped
        print(json.dumps(out), flush=True)
    r.close()
    if rank == 0 and fm["undecidable"]:
        print("fm_dev: %d sample(s) within 0.06 ulp of an atan2 rounding midpoint: glibc's own result there is host-dependent"
              % fm["undecidable"], file=sys.stderr)
    if fm_bad:
        print("fm_dev: %d slow-path decisions differ from this host's libm" % fm_bad, file=sys.stderr)
        if world > 1:
            dist.destroy_process_group()
        sys.exit(4)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
