// Test and instrumentation knobs of the library.
//
// THREE builds of the same sources (tfrec_amd/_build.py):
//   libtfrec_amd.so      the product -- what bench.py, the adapter and the parity tests load.  Built WITHOUT
//                        TFREC_AMD_EXPERIMENTS: every knob below is its default as a compile-time constant, the test hooks
//                        fold away, and neither a getenv call nor a knob's name is in the binary
//                        (`strings libtfrec_amd.so | grep -c TFREC_AMD_DEEP` = 0; tests/test_cabi_cpu.py checks it).
//   libtfrec_amd_exp.so  -DTFREC_AMD_EXPERIMENTS: the knobs are read from the environment.  Loaded only by the tests that
//                        drive a hook (tests/: api.Receiver(..., experiments=True)) and by sessions under profiles/.
//   libtfrec_amd_seg.so  the experiments build with -DTFREC_AMD_SEG_SLOTS=16 (tfrec_dev.h: kSegSlots and its lower bound): biquad
//                        segments short enough that the second repair pass and the serial repair of biquad.h run on ordinary
//                        input.  Loaded only by tests/test_biquad_ladder_gpu.py (api.Receiver(..., short_segments=True)).
// What the knobs are still for (every other A/B variant of rounds 1-6 is retired: profiles/NOTES.md, "retired knobs"):
//   test hooks        WHB_FORCE_FAIL, WHB_TEST_PERTURB (WHB check failures and redos), FM_FLAG_EPS (the discriminator's exact
//                     slow path), COPY_GUESS_MIN (the drain's fetch-the-rest path);
//   stream layout     DEEP=0: the shallow layout (tests and tests/stress_gpu.py run it);
//   vectorised walks  TFA1_VEC, TFA2_VEC: =0 selects the cooperative slicers' scalar walk (read by the kernels from WinTables);
//   instrumentation   HOST_PROF (host time per submit / drain), DEBUG_WINHIST, DEBUG_CONVHIST (distributions of one submit).
// The macros take the knob's name WITHOUT its TFREC_AMD_ prefix; in the product build the name is not expanded at all.
#pragma once

#include <stdlib.h>

#ifdef TFREC_AMD_EXPERIMENTS
namespace tfrec {
// integer from the environment, `dflt` when unset or outside [lo, hi]
static inline int knob_int(const char *name, int dflt, int lo = 0, int hi = 1 << 30)
{
	const char *v = getenv(name);
	const int x = v ? atoi(v) : dflt;
	return x >= lo && x <= hi ? x : dflt;
}
}  // namespace tfrec
#define TFREC_KNOB_INT(NAME, dflt, lo, hi) (::tfrec::knob_int("TFREC_AMD_" NAME, (dflt), (lo), (hi)))
#define TFREC_KNOB_STR(NAME) (getenv("TFREC_AMD_" NAME))
#define TFREC_KNOBS_BUILT 1
#else
#define TFREC_KNOB_INT(NAME, dflt, lo, hi) (dflt)
#define TFREC_KNOB_STR(NAME) (static_cast<const char *>(nullptr))
#define TFREC_KNOBS_BUILT 0
#endif
