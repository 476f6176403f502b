// tfrec_amd/csrc/capi.hip -- C ABI (include/tfrec_amd.h): context, submit, drain.  No torch types.  One translation unit, cut by
// concern into the capi_*.h headers below (each needs the ones above it); their entry points have C linkage from tfrec_amd.h.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <functional>
#include <new>
#include <vector>

#include "knobs.h"
#include "tfrec_dev.h"

namespace tfrec {
hipError_t launch_decim10(hipStream_t st, const uint8_t *iq, size_t stride, int n_streams, int n_blocks,
			  const uint8_t *tail_in, uint8_t *tail_out, uint32_t *out, size_t out_stride, const uint4 *chan);
hipError_t launch_resample(hipStream_t st, const uint8_t *iq, size_t stride, int n_streams, int n_blocks, int p, int q, int t,
			   const float *taps, const uint8_t *tail_in, uint8_t *tail_out, uint32_t *out, size_t out_stride,
			   const uint4 *chan, bool tuned);
hipError_t launch_resample_fmt(hipStream_t st, int fmt, const uint8_t *iq, size_t stride, int n_streams, int n_blocks, int p, int q, int t,
			       const float *taps, const uint8_t *tail_in, uint8_t *tail_out, uint32_t *out, size_t out_stride,
			       const uint4 *chan, bool tuned);
hipError_t launch_ingest(hipStream_t st, int fmt, const uint8_t *iq, size_t stride, int n_streams, int n_blocks, uint32_t *out,
			 size_t out_stride, const uint4 *chan);
hipError_t launch_frontend(hipStream_t st, const uint8_t *iq, size_t stride, int n_streams, int n_blocks,
			   const uint8_t *tail_in, uint8_t *tail_out, uint32_t *dec, size_t dec_stride,
			   unsigned long long *mask, size_t mask_stride, uint32_t *prevdec, int thresh, const FrontTapsCfg &taps,
			   bool in16, const uint2 *tune, const uint4 *chan);
hipError_t launch_fmdev(hipStream_t st, const uint32_t *dec, size_t dec_stride, const unsigned long long *mask,
			size_t mask_stride, const uint32_t *prevdec, int16_t *fmdev, size_t fmdev_stride, EventBuf *eb,
			int n_streams, int n_blocks, int wmax, double flag_eps);
hipError_t launch_pipeline(const PipeCtl &P, const uint32_t *dec, size_t dec_stride, const unsigned long long *mask,
			   size_t mask_stride, const int16_t *fmdev, size_t fmdev_stride, int n_streams, int n_blocks,
			   long long sample_base, const ChainLaunch &L, const WinTables &T, int16_t *ld16, int32_t *dev32,
			   tfrec_amd_event *events, EventBuf *eb, uint32_t flags);
hipError_t whb_chain_lds_optin();
hipError_t launch_fm_probe(hipStream_t st, const int32_t *quads, size_t n, int32_t *out, EventBuf *eb, int kind);
hipError_t launch_iir_probe(hipStream_t st, const double *in, size_t n, const BiquadCoef &c, double *out, int form);
hipError_t launch_threshold(hipStream_t st, const uint32_t *dec, size_t dec_stride, unsigned long long *mask,
			    size_t mask_stride, int n_streams, int n_blocks, FskState *fsk, int wmax, const StreamCfg *scfg);
hipError_t launch_chains(hipStream_t st, const uint32_t *dec, size_t dec_stride, const unsigned long long *mask,
			 size_t mask_stride, int n_streams, int n_blocks, long long sample_base, const ChainLaunch &L,
			 tfrec_amd_event *events, EventBuf *eb, uint32_t flags);
hipError_t launch_levels(hipStream_t st, const uint32_t *dec, size_t dec_stride, const unsigned long long *mask, size_t mask_stride,
			 int n_streams, int n_blocks, LevelState *lev, const StreamCfg *scfg, tfrec_amd_level *out);
hipError_t launch_capture(hipStream_t st, const uint32_t *dec, size_t dec_stride, const unsigned long long *mask, size_t mask_stride,
			  int n_streams, int n_blocks, long long sample_base, CaptureState *cst, const StreamCfg *scfg, CaptureStage *stage,
			  int stage_cap, uint2 *cnt, uint4 *base, CaptureHeader *hdr, tfrec_amd_run *runs, uint32_t max_runs, uint32_t *pool,
			  unsigned long long max_samples);
hipError_t launch_spectrum(hipStream_t st, int fmt, const uint8_t *iq, size_t stride, int n_rows, long n_in, int n_bins, int g,
			   size_t max_records, unsigned long long *sum, unsigned long long *peak, uint32_t *nfr);
hipError_t launch_occupancy(hipStream_t st, int n_rows, long n_in, int n_bins, int g, size_t max_records, const unsigned long long *sum,
			    const unsigned long long *peak, const uint32_t *nfr, uint32_t ratio, uint32_t rel, tfrec_amd_occupancy *recs,
			    uint32_t *bits);
hipError_t launch_correct(hipStream_t st, int fmt, const uint8_t *iq, size_t stride, int n_rows, long n_in, const CorrectBufs &b);
hipError_t launch_decin(hipStream_t st, const uint8_t *in, size_t stride, int n_streams, int n_blocks, const uint4 *chan, uint32_t *dec,
			size_t dec_stride, unsigned long long *mask, size_t mask_stride, uint32_t *prevdec, uint32_t *last, int thresh,
			const StreamCfg *scfg);
hipError_t launch_decin_runs(hipStream_t st, int n_streams, int n_blocks, const uint4 *tab, const uint32_t *pool, const uint32_t *pre,
			     const int32_t *first, const uint2 *ov, uint32_t *dec, size_t dec_stride, unsigned long long *mask,
			     size_t mask_stride, uint32_t *prevdec, uint32_t *last, int thresh, const StreamCfg *scfg);
hipError_t launch_capture_pre(hipStream_t st, const tfrec_amd_run *runs, const CaptureHeader *hdr, uint32_t max_runs, long long sample_base,
			      const uint32_t *dec, size_t dec_stride, const uint32_t *prevdec, uint32_t *pre);
}  // namespace tfrec

using namespace tfrec;

#include "capi_ctx.h"      // constants, errors, tfrec_amd_ctx and what it owns, guards, checks, side lanes
#include "capi_create.h"   // chain parameters, tap tables, the context's buffers, streams and events; constructors, destroy
#include "capi_probe.h"    // the discriminator's host check, debug statistics; probes, read-backs, timings, memory, counters
#include "capi_submit.h"   // the two kernels, a submit's resets and staging, submit_common, the submits, drain, sync, pending
#include "capi_outputs.h"  // the level meter's, the recorder's, the spectrum's and the occupancy detector's entry points
#include "capi_correct.h"  // the DC blocker's and the IQ balancer's constructors, getters, reads and resets
#include "capi_streams.h"  // reset, configure, the three tunes, map, and their getters
#include "capi_decin.h"    // the channel-rate constructor, the recorder's pre samples, sparse submits

extern "C" {

const char *tfrec_amd_version(void) { return "tfrec_amd 0.1 (gfx950)"; }

int tfrec_amd_fifo_depth(void) { return kSets; }

const char *tfrec_amd_strerror(int code)
{
	switch (code) {
	case TFREC_AMD_OK: return "ok";
	case TFREC_AMD_E_INVAL: return "invalid argument or unsupported configuration";
	case TFREC_AMD_E_NOMEM: return "out of memory";
	case TFREC_AMD_E_HIP: return "HIP runtime error";
	case TFREC_AMD_E_OVERFLOW: return "event buffer overflow";
	case TFREC_AMD_E_STATE: return "call sequence error";
	default: return "unknown error";
	}
}

const char *tfrec_amd_last_error(void) { return g_err; }

int tfrec_amd_rssi_db(int slot, int64_t rssi_raw)
{
	if (slot == TFREC_AMD_SLOT_WHB)  // whb.cpp:696 as compiled: 10*log10(rssi*0.00025 + 1)
		return d2i_host(10 * log10((double)rssi_raw * 0.00025 + 1.0));
	// tfa1.cpp:180, tfa2.cpp:434: (int)(10*log10(rssi)) with an int rssi
	return d2i_host(10 * log10((double)(int)rssi_raw));
}

}  // extern "C"
