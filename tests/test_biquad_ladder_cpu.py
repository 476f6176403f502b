"""The biquad passes' speculate-and-repair ladder (tfrec_amd/csrc/biquad.h) executed on the CPU: tests/ladder_model.py restates
the four rungs as the kernels decide them, and these tests check on the frozen inputs that (1) whatever the rungs do, the stored
outputs and the carried state are the true trajectory bit for bit -- the header's "exactness never depends on convergence" --,
(2) the model's windows are the oracle's, and (3) at 16-slot segments the inputs send every chain through every rung, so that
tests/test_biquad_ladder_gpu.py, which runs the same inputs through the kernels, reaches the second repair and the serial
repair.  No GPU."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import ladder_model as LM
from oracle import oracle as O
from oracle import scenes as S

M = LM.N_BLOCKS * S.BLOCK_DEC
RUNG_ENTRIES = ("segments", "k3b_unconverged", "k3b2_run", "k3b2_unconverged", "serial", "serial_joined", "serial_to_end", "k3b_slots")


def _chain_total(models, slot):
    return LM.total_census(r for m in models for r in m[slot])


@pytest.mark.parametrize("seg_slots", [16, 256])
def test_ladder_outputs_are_the_true_trajectory(seg_slots):
    """Every in-window output the ladder leaves stored, and the state it carries to the next submit, equal the true trajectory's
    bit for bit, at the short and at the product segment length."""
    n = 0
    for s, m in enumerate(LM.frozen_models(seg_slots)):
        for slot, chain in m.items():
            for r in chain:
                assert r.first_difference(r.row) is None, "stream %d: %s" % (s, r.first_difference(r.row))
                assert r.ladder_end.bits() == r.true_end.bits(), "stream %d %s submit %d: carried state" % (s, LM.NAMES[slot], r.k)
                assert np.all(r.rung[r.index // 32] > 0)
                n += len(r.index)
    assert n > 4 * 10 * M  # (the always-triggered rows alone)


def test_true_trajectory_is_one_filter_run_over_the_in_window_samples():
    """The model's true rows, submit after submit, against ONE run of the oracle's iir2 (orc_iir_run) over the chain's in-window
    samples of the whole stream: the windows' cut at the submits, the slot layout and the carried state drop out."""
    _, decs, xs = LM.frozen_oracles()
    for s, m in enumerate(LM.frozen_models(16)):
        trig = S.trigger_samples(decs[s], LM.THRESH)
        for slot, chain in m.items():
            inw = np.zeros(M, dtype=bool)
            for a, b in S.windows(trig, S.WINDOW[slot]):
                inw[a:b + 1] = True
            x = np.ascontiguousarray(xs[s][slot][inw], dtype=np.float64)
            y = np.empty_like(x)
            O.lib().orc_iir_run(LM.cutoff(slot), x.ctypes.data, y.ctypes.data, len(x))
            want = np.trunc(y).astype(np.int64)
            if slot != 4:
                want = want.astype(np.int16).astype(np.int64)
            got = np.concatenate([r.true_row[r.index] for r in chain])
            assert np.array_equal(got, want), "stream %d %s" % (s, LM.NAMES[slot])


def test_model_windows_are_the_oracles():
    """The windows the model cuts give the oracle's flush counts per slot (an empty WHB window ends without a flush), and per
    submit what oracle.scenes.table_demand says of them."""
    orcs, decs, _ = LM.frozen_oracles()
    bounds = np.cumsum((0,) + LM.CUTS) * S.BLOCK_DEC
    for s, m in enumerate(LM.frozen_models(16)):
        trig = S.trigger_samples(decs[s], LM.THRESH)
        ev = orcs[s].events_full()
        for slot, chain in m.items():
            wins = S.windows(trig, S.WINDOW[slot])
            if slot < 4:
                assert sum(1 for w in wins if w[1] < M) == sum(1 for e in ev if e[0] == slot), (s, slot)
            for r, lo, hi in zip(chain, bounds, bounds[1:]):
                need = S.table_demand([(a - lo, b - lo) for a, b in wins], int(hi - lo), 1)
                assert need["windows"] == len(r.windows), (s, slot, r.k)
                used = max(((og >> 5) + j + (n + 31) // 32 for j, (og, n) in enumerate(r.windows)), default=0)
                assert need["slots"] == used <= len(r.rung), (s, slot, r.k)
                assert r.census["segments"] == (sum((n + 31) // 32 for _, n in r.windows) + 15) // 16
    for s in LM.ALWAYS_TRIGGERED:  # one window from the first trigger on, continued at sample 0 of every later submit
        for chain in LM.frozen_models(16)[s].values():
            for r, c in zip(chain, LM.CUTS):
                (og, n), = r.windows
                end = c * S.BLOCK_DEC - (LM.TAIL_BYTES // 8 - S.WINDOW[r.slot] if r.k == len(LM.CUTS) - 1 else 0)
                assert end - 16 <= og + n <= end + 16 * (r.k == len(LM.CUTS) - 1) and (og == 0 if r.k else og < 64), (s, r.k, og, n)


def test_short_segments_send_every_chain_through_every_rung():
    """The conditions the frozen inputs are chosen for (not measurements: if an input set misses one, the inputs change): at 16
    slots every chain has at least 3 of everything -- segments, first repairs that do not converge, second repairs, second
    repairs that do not converge, serial repairs, serial repairs that join a checkpoint and that run to the segment's end --, serial
    repairs that hop a window boundary occur 3 times in the TFA_2 family and once for WHB."""
    models = LM.frozen_models(16)
    for slot in LM.BIQUAD_SLOTS:
        tot = _chain_total(models, slot)
        print(LM.NAMES[slot], tot)
        for key in RUNG_ENTRIES:
            assert tot[key] >= 3, (LM.NAMES[slot], key, tot)
        assert tot["serial"] == tot["serial_joined"] + tot["serial_to_end"]
    assert sum(_chain_total(models, slot)["serial_hops"] for slot in (1, 2, 3)) >= 3
    whb = _chain_total(models, 4)
    assert whb["serial_hops"] >= 1 and whb["serial_joined"] >= 1 and whb["serial_to_end"] >= 1
    # the single-chain cases of the GPU module run the always-triggered rows alone: they reach the serial repair too
    for slot in (2, 4):
        tot = LM.total_census(r for s in LM.ALWAYS_TRIGGERED for r in models[s][slot])
        assert tot["serial"] >= 2 and tot["k3b2_run"] >= 3, (slot, tot)


# WHB's chain input is integer arithmetic (fm_dev_nrzs), so its census is the same on every machine: recorded here
WHB_CENSUS = {16: dict(segments=1555, k3b_unconverged=268, k3b2_run=245, k3b2_unconverged=32, serial=8, serial_joined=3,
                       serial_to_end=5, serial_hops=3, k3b_slots=19553),
              256: dict(segments=99, k3b_unconverged=0, k3b2_run=0, k3b2_unconverged=0, serial=0, serial_joined=0, serial_to_end=0,
                        serial_hops=0, k3b_slots=1191)}


def test_product_length_census():
    """At the product's 256 slots no segment of these inputs gets past the first repair, which always converges (the TFA_2
    family's figures depend on the host's atan2 in the last place and are printed; DESIGN.md section 4 has them)."""
    for seg_slots in (16, 256):
        assert _chain_total(LM.frozen_models(seg_slots), 4) == WHB_CENSUS[seg_slots]
    models = LM.frozen_models(256)
    for slot in LM.BIQUAD_SLOTS:
        tot = _chain_total(models, slot)
        print(LM.NAMES[slot], tot)
        assert tot["segments"] == 99 and tot["k3b_slots"] >= tot["segments"]
        for key in ("k3b_unconverged", "k3b2_run", "k3b2_unconverged", "serial", "serial_joined", "serial_to_end", "serial_hops"):
            assert tot[key] == 0, (LM.NAMES[slot], key)


def test_core_under_sanitizers(tmp_path):
    """tests/ladder_core.c as a stand-alone program under ASan and UBSan, on a WHB chain submit with serial repairs of both
    outcomes across windows: clean, exact, and the census of the library build."""
    _, decs, xs = LM.frozen_oracles()
    s, slot, k = 13, 4, 1
    r = LM.frozen_models(16)[s][slot][k]
    lo = LM.CUTS[0] * S.BLOCK_DEC
    x = xs[s][slot][lo:lo + LM.CUTS[k] * S.BLOCK_DEC]
    dump, exe = str(tmp_path / "chain.bin"), str(tmp_path / "ladder_core_main")
    LM.dump_chain(dump, x, r.windows, slot, 16, len(r.rung), r.start)
    subprocess.check_call(["gcc", "-O1", "-g", "-ffp-contract=off", "-std=c11", "-Wall", "-Werror", "-DLADDER_MAIN",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, LM.CORE_C])
    out = subprocess.run([exe, dump], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stderr == "", out.stdout + out.stderr
    words = out.stdout.split()
    assert words[:4] == ["rc", "0", "exact", "1"]
    assert [int(v) for v in words[5:5 + len(LM.CENSUS)]] == [r.census[key] for key in LM.CENSUS]
    assert len(r.windows) > 1 and r.census["segments"] > 3
