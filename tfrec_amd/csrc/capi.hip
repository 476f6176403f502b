// tfrec_amd/csrc/capi.hip -- C ABI (include/tfrec_amd.h): context, submit, drain.  No torch types.
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
}  // namespace tfrec

using namespace tfrec;

constexpr int kTuneLimit = 768000;  // |tune_hz| < half the 1.536 MS/s sample rate
constexpr int kTuneWideLimit = 7680000;  // tfrec_amd_tune_streams_wide: half the 15.36 MS/s input rate
constexpr int kRateQMax = 64;  // tfrec_amd_create_rate: the largest Q
constexpr int k10xTail = 112;   // TFREC_AMD_F_INPUT_10X: the 10:1 stage's raw history per stream in bytes (decim10_kernel: kTail10)
constexpr int kRateTail = 128;  // tfrec_amd_create_rate: the resampling stage's raw history per stream in bytes (resample.h: kRsTail)
constexpr int kFmtTail = 256;   // tfrec_amd_create_format: the history per stream in bytes, 64 complex samples of x (formats.h: kFmtTailDw)

// Buffer / table sets = submits that may be in flight (the FIFO depth): front end of submit k+2, biquad stage of
// k+1 and slicer stage of k run beside each other in the deep layout
constexpr int kSets = TFREC_AMD_FIFO_DEPTH;
// header of a set's event block: EventBuf + 16 bytes (the window tables' overflow flag, at kEvOverflowOff on the device and
// in the host copy alike), padded
constexpr size_t kEvOverflowOff = sizeof(EventBuf);
constexpr size_t kEvFreshBytes = kEvOverflowOff + 16;  // what a submit resets from d_eb_fresh: EventBuf + the flag
constexpr size_t kEvHeader = (kEvFreshBytes + 255) & ~(size_t)255;

static thread_local char g_err[256] = "";

static int hip_fail(hipError_t e, const char *what)
{
	snprintf(g_err, sizeof(g_err), "%s: %s", what, hipGetErrorString(e));
	return TFREC_AMD_E_HIP;
}
#define HIPCHK(call)                                   \
	do {                                           \
		hipError_t e_ = (call);                \
		if (e_ != hipSuccess)                  \
			return hip_fail(e_, #call);    \
	} while (0)
// a step that returns a TFREC_AMD_* status
#define TRY(call)                                      \
	do {                                           \
		const int rc_ = (call);                \
		if (rc_ != TFREC_AMD_OK)               \
			return rc_;                    \
	} while (0)

struct FmTotals {
	unsigned long long resolved = 0, verified = 0, mismatch = 0, undecidable = 0;
};

// TFREC_AMD_F_TIMING: a set's marks on the front-end stream (every layout) and the end of the serial chains
enum HostMark {
	kEvSubmit,      // the submit starts (fs)
	kEvFmdevDone,   // the discriminator pass behind the front end is done (fs): the chains start
	kEvSerialDone,  // the serial chains are done (cs)
	kEvFrontDone,   // the front end and the threshold pass are done (fs)
	kHostMarks
};

struct tfrec_amd_ctx {
	tfrec_amd_config cfg;
	ChainLaunch launch;
	// stage-2 taps of the front end: the context's (f2, scfg == nullptr) until a stream is configured, then narrow (f2) and
	// wide (w) with scfg = d_scfg
	FrontTapsCfg taps;
	// Every device buffer, page-locked block, stream and event the context owns, in the order tfrec_amd_create made them
	// (own_*): release_all frees them in reverse.  Aliased streams are not recorded (make_streams).
	struct Owned {
		enum Kind { kDevice, kPinned, kStream, kEvent } kind;
		void *h;
	};
	std::vector<Owned> owned;
	size_t dev_bytes = 0, pinned_bytes = 0;  // tfrec_amd_get_memory
	// ---- streams and events (make_streams: the layout and why; make_pipes)
	// per set: what launch_pipeline takes for a submit of that set (the streams, the set's events and buffers); the serial
	// layout uses its fs, cs, ev_front and done
	PipeCtl pipe[kSets] = {};
	hipStream_t cpy = nullptr;  // the drain's device-to-host copies
	bool deep = false;          // deep layout
	bool fmdev_k2 = false;      // the discriminator pass runs in the pipeline (PipeCtl::fmdev_wmax), not behind the front end
	hipEvent_t ev_in[kSets] = {};              // the caller's stream has produced the input
	hipEvent_t ev[kSets][kHostMarks] = {};     // TFREC_AMD_F_TIMING
	hipEvent_t tev[kSets][kTimingMarks] = {};  // TFREC_AMD_F_TIMING, window-parallel pipeline: PipeCtl::tev
	int last_set = 0;
	// ---- front end (make_front_buffers).  Outputs, one set per submit in flight like the event buffers: the front end of
	// submit k+2 (its own stream) runs beside the demodulator chains of submit k
	uint32_t *d_dec[kSets] = {};
	size_t dec_stride = 0;  // uint32 units
	unsigned long long *d_mask[kSets] = {};
	size_t mask_stride = 0;
	int16_t *d_fmdev[kSets] = {};  // [n_streams][m_max] fm_dev of the decimated samples (computed near windows)
	uint32_t *d_prevdec[kSets] = {};  // [n_streams] the decimated sample before the submit's first one
	FskState *d_fsk = nullptr;  // auto threshold (every context has it: a stream can be configured to auto)
	// TFREC_AMD_F_LEVELS (make_levels): the level meter's carried state, one record buffer per set
	// ([n_streams][the submit's n_blocks]), its low-priority stream, the set's "records written" event and the set's block count
	bool levels = false;
	LevelState *d_lev = nullptr;
	tfrec_amd_level *d_levels[kSets] = {};
	hipStream_t lv = nullptr;
	hipEvent_t ev_lev[kSets] = {};
	int set_blocks[kSets] = {};
	// tfrec_amd_enable_capture: the recorder's carried state, the working set its three kernels share (staged runs,
	// counts and bases per stream: one, because the submits' recorder kernels follow each other on one stream), per set the run
	// table, the sample pool and the header with the true totals, its low-priority stream and the set's "captures written" event
	bool capture = false;
	uint32_t cap_max_runs = 0;
	uint64_t cap_max_samples = 0;
	CaptureState *d_capst = nullptr;
	CaptureStage *d_capstage = nullptr;
	int cap_stage_cap = 0;
	uint2 *d_capcnt = nullptr;
	uint4 *d_capbase = nullptr;
	CaptureHeader *d_caphdr[kSets] = {};
	tfrec_amd_run *d_runs[kSets] = {};
	uint32_t *d_pool[kSets] = {};
	hipStream_t cap = nullptr;
	hipEvent_t ev_cap[kSets] = {};
	std::vector<tfrec_amd_run> cap_tmp;
	// tfrec_amd_enable_spectrum: bins, frames per record, rows analysed at most and the records the largest submit
	// can hold; per set the sums and peaks ([spec_rows][spec_max_records][spec_n]), the frame counts ([spec_rows][spec_max_records]),
	// the "records written" event and what the set's submit held (rows analysed, records); the kernel's low-priority stream
	bool spectrum = false;
	int spec_n = 0, spec_g = 0, spec_rows = 0;
	size_t spec_max_records = 0;
	unsigned long long *d_spec_sum[kSets] = {}, *d_spec_peak[kSets] = {};
	uint32_t *d_spec_nf[kSets] = {};
	hipStream_t sp = nullptr;
	hipEvent_t ev_spectrum[kSets] = {};
	int spec_set_rows[kSets] = {}, spec_set_records[kSets] = {};
	int wmax = 0;
	// tfrec_amd_configure_streams: every stream's settings as the next submit uses them (scfg, the host's copy), their device
	// copy as the last submit used them (d_scfg: written only by stream_reset_kernel, in the entries of its list), and the
	// settings that travel with a submit's reset list (d_rcfg / h_rcfg).  per_stream: a stream was configured -- from then on
	// the kernels read d_scfg (launch.scfg, taps.scfg); before, the uniform kernels run.  n_auto: streams of scfg in auto mode.
	std::vector<StreamCfg> scfg;
	std::vector<tfrec_amd_stream_config> scfg_api;
	StreamCfg *d_scfg = nullptr;
	StreamCfg *d_rcfg[kSets] = {}, *h_rcfg[kSets] = {};
	bool per_stream = false;
	int n_auto = 0;
	// tfrec_amd_tune_streams: every stream's tune as the next submit uses it (tune_hz, and its phase increment tune_inc), and per
	// set the {inc, phase of the submit's first sample} the set's front end reads (h_tune -> d_tune, filled by the submit).
	// n_tuned: streams with inc != 0 -- while there is one, the tuned front end runs; before, the kernels of an untuned context.
	std::vector<int32_t> tune_hz;
	std::vector<uint32_t> tune_inc;
	uint2 *d_tune[kSets] = {}, *h_tune[kSets] = {};
	int n_tuned = 0;
	// tfrec_amd_map_streams / tfrec_amd_tune_streams_wide: the input row every stream reads from the next submit
	// on (the identity until a stream is mapped: `mapped`), every stream's wide tune and its phase increment per 15.36 MS/s
	// sample (n_wide: streams with wide_inc != 0), and per set the {inc10, phase10, row, 0} the set's 10:1 stage -- in a context
	// of the default input the front end, for the row -- reads (h_chan -> d_chan, filled by the submit).
	std::vector<int32_t> row;
	bool mapped = false;
	std::vector<int32_t> wide_hz;
	std::vector<uint32_t> wide_inc;
	int n_wide = 0;
	uint4 *d_chan[kSets] = {}, *h_chan[kSets] = {};
	uint8_t *d_tail[kSets] = {};  // FIR history: [tail_sel] is read by the next front end, [tail_sel ^ 1] written
	int tail_sel = 0;
	// in16: a pre-stage (launch_prestage: the 10:1 stage, the resampling stage or the format conversion) writes stage 0, 1.536 MS/s
	// int16 pairs, one buffer per set, and the front end reads int16.  Its history of the input, if it keeps one: pre_bytes per
	// stream, pre_fill after a start or restart, [tail_sel] read and [tail_sel ^ 1] written like d_tail (make_front_buffers).
	uint32_t *d_in16[kSets] = {};
	size_t in16_stride = 0;  // uint32 units
	uint8_t *d_pre[kSets] = {};
	int pre_bytes = 0, pre_fill = 0;
	bool in10x = false;  // TFREC_AMD_F_INPUT_10X
	// tfrec_amd_create_rate: the input rate is 1536000 rate_p / rate_q; the resampling stage writes d_in16 as the
	// 10:1 stage does, from a tap table [rate_q][rate_t] (h / 1024 as floats).
	// rate_abs: max_phi sum_n |h[phi][n]| of that table, for the guard of tfrec_amd_tune_streams_input (6g), whose per-stream
	// tune and increment per input sample live in wide_hz / wide_inc as the 10x context's wide tune does.
	int32_t rate_p = 1, rate_q = 1, rate_t = 0;
	long long rate_abs = 0;
	bool resamp = false, in16 = false;
	float *d_rtaps = nullptr;
	// tfrec_amd_create_format: fmt is the TFREC_AMD_FMT_* of the input rows, 0 (U8) in every context of the older
	// constructors.  A rate context with another format runs resample_fmt_kernel from a history of canonical x instead
	// of the raw one; at the base rate (ingest: rate 1/1, no resampler) ingest_kernel converts the rows into d_in16.
	int32_t fmt = TFREC_AMD_FMT_U8;
	bool ingest = false;
	// ---- window-parallel pipeline (make_window_state).  One set per submit in flight, like the front-end outputs: the window
	// scan and the biquads of submit k+1 fill theirs while the slicers of submit k still read the other
	int16_t *d_ld16[kSets] = {};   // [chains][m_max] tfa2-family biquad outputs
	int32_t *d_dev32[kSets] = {};  // [n_streams][m_max] WHB stage-1 outputs
	WinTables win[kSets] = {};
	void *win_block[kSets] = {};
	int32_t *d_tcarry = nullptr;                 // WinTables::timeout_carry
	WhbExact *d_whbx = nullptr;                  // WinTables::whbx
	int *d_whbcarry = nullptr;                   // PipeCtl::whb_carry
	uint32_t *d_whbgen = nullptr;                // WinTables::whbgen
	ChainState *d_whbX = nullptr;                // WinTables::whbX
	ChainState *d_whbscr = nullptr;              // WinTables::whbscr
	int whb_test_perturb = 0;                    // TFREC_AMD_WHB_TEST_PERTURB (tests)
	int whb_force_fail = 0;                      // TFREC_AMD_WHB_FORCE_FAIL (tests)
	int submit_seq = 0;
	// ---- event buffers (make_event_blocks).  One set per submit in flight (FIFO of depth TFREC_AMD_FIFO_DEPTH): submits may
	// be queued while the host still drains an older one
	tfrec_amd_event *d_events[kSets] = {};
	EventBuf *d_eb[kSets] = {};
	uint8_t *d_evblock[kSets] = {}, *h_evblock[kSets] = {};  // what d_eb / d_events and h_eb / h_events point into
	uint8_t *h_evblock_dev[kSets] = {};                      // the page-locked blocks as the device addresses them (drain_copy_kernel)
	EventBuf *d_eb_fresh = nullptr;       // { 0, max_events, 0 }: copied over a set's EventBuf when a submit starts
	// Pinned staging for the drain, one per set: the device-to-host copies of a submit's event buffer are queued on cpy
	// when the submit is made (behind its three end-of-chain events), so they are done when the host comes to drain it.
	// The number of events is not known then: `copy_guess` of them are copied ahead (twice the last submit's count), the
	// drain fetches the rest if there are more.
	tfrec_amd_event *h_events[kSets] = {};
	EventBuf *h_eb[kSets] = {};
	hipEvent_t copied[kSets] = {};
	uint32_t copied_n[kSets] = {};
	uint32_t copy_guess = 4096, copy_guess_min = 4096;  // TFREC_AMD_COPY_GUESS_MIN (tests: exercise the fetch-the-rest path)
	std::vector<uint32_t> sort_idx, sort_start;
	int head = 0, inflight = 0;           // oldest undrained set, submits not yet drained (0..TFREC_AMD_FIFO_DEPTH)
	int last_drained = -1;
	uint8_t *d_stage[kSets] = {};  // tfrec_amd_submit_host: device staging, one per buffer set, grown on demand
	size_t stage_bytes[kSets] = {};
	long long sample_base = 0;
	int last_blocks = 0;
	// tfrec_amd_reset_streams: streams marked since the last submit (each once), and the per-stream sample origin -- the
	// sample_base at the stream's last reset -- that the drain subtracts from end_sample.  A submit records the origins it
	// ran with (set_origin), so that the drain of an older submit still in the FIFO uses the older ones.
	std::vector<int32_t> reset_pending;
	std::vector<uint8_t> reset_marked;
	std::vector<long long> origin;
	std::vector<long long> set_origin[kSets];  // empty: no submit before the set's one carried a reset
	int32_t *d_reset[kSets] = {};  // the submit's reset list on the device (stream_reset_kernel)
	int32_t *h_reset[kSets] = {};  // ... and its page-locked source
	ChainState *d_chain_init = nullptr;  // the constructor ChainState (chain_init_state), source of every reset
	bool submitted = false;              // pipe[last_set].done has been recorded
	bool any_reset = false;              // a submit has carried a reset: set_origin is kept from then on
	bool timed = false;
	// fm_dev samples decided by the exact slow path: all / checked against this host's libm at drain / differing from
	// it / closer to a rounding midpoint than glibc's error bound
	FmTotals fm;
	// fm_dev samples closer than this to a truncation boundary take the exact slow path.  1e-9 = 250x the fast path's
	// error bound; TFREC_AMD_FM_FLAG_EPS (tests) widens it to drive the slow path -- exact for any value -- through the
	// pipeline with ordinary input: 1e-3 fills the deferred list, 0.6 overflows it (every sample: the rescan path)
	double fm_flag_eps = 1e-9;
	// A HIP call failed in the middle of a submit: kernels of it may already have run on carried state (FIR history, chain
	// state, the FIFO's bookkeeping), so the context cannot continue exactly.  Every later submit / drain returns
	// TFREC_AMD_E_STATE; destroy and recreate.
	bool poisoned = false;
	// TFREC_AMD_HOST_PROF=1: host-side time of the submit / drain calls, printed when the context is destroyed
	double hp_submit = 0, hp_wait = 0, hp_copy = 0, hp_sort = 0, hp_gap = 0, hp_lat = 0, hp_s2s = 0;
	long hp_n = 0, hp_gap_n = 0;
};

namespace tfrec {
// The drain's device-to-host copy as a kernel of our own (16 bytes per lane into the page-locked block, which the device addresses
// directly).  hipMemcpyAsync did the same with the runtime's copy kernel -- but two or three times after every synchronize (the 6th and
// 7th submit of the driver's 20-step line) the CALL blocked the host for a whole batch period, now and then for two (13 ms: the pipeline
// ran dry, 6.2 instead of 5.75 ms per step): profiles/r06_host_stalls.txt.
__global__ __launch_bounds__(256) void drain_copy_kernel(const uint4 *__restrict__ src, uint4 *__restrict__ dst, size_t n16)
{
	for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (size_t)gridDim.x * 256)
		dst[i] = src[i];
}

// tfrec_amd_reset_streams: every piece of state a submit carries to the next one, back to what tfrec_amd_create made of it,
// for the streams list[0 .. n_list) (distinct, < n_streams).  A workgroup per listed stream.  See DESIGN.md, "Stream reset".
struct StreamReset {
	const int32_t *list;
	int32_t n_list, n_streams;
	uint8_t *tail;      // front-end FIR history the NEXT front end reads: tail_bytes per stream, filled with tail_fill
	int32_t tail_bytes, tail_fill;
	uint8_t *pre;       // the pre-stage's history the NEXT one reads (pre_bytes per stream, filled with pre_fill), or nullptr
	int32_t pre_bytes, pre_fill;
	FskState *fsk;      // auto threshold
	LevelState *lev;    // TFREC_AMD_F_LEVELS: the level meter's carried state, or nullptr
	CaptureState *cap;  // tfrec_amd_enable_capture: the recorder's carried state, or nullptr
	const StreamCfg *cfgs;  // [n_list] the listed streams' settings from this submit on ...
	StreamCfg *scfg;        // ... written over their entries here
	int32_t n_active;
	ChainState *states[kNSlots];
	const ChainState *chain_init;
	int32_t *tcarry;    // [n_active * n_streams] window scan's timeout carry (window-parallel pipeline), or nullptr
	WhbExact *whbx;     // WHB check's exact filter state, its carry and the redo's chain state (WHB registered), or nullptr
	int *whbcarry;
	ChainState *whbX;
};

__global__ __launch_bounds__(64) void stream_reset_kernel(StreamReset R)
{
	if ((int)blockIdx.x >= R.n_list)
		return;
	const int s = R.list[blockIdx.x];
	if (s < 0 || s >= R.n_streams)
		return;
	const int ln = threadIdx.x;
	for (int i = ln; i < R.tail_bytes; i += 64)
		R.tail[(size_t)s * R.tail_bytes + i] = (uint8_t)R.tail_fill;
	for (int i = ln; i < R.pre_bytes; i += 64)  // (0 without a history)
		R.pre[(size_t)s * R.pre_bytes + i] = (uint8_t)R.pre_fill;
	constexpr int kChunks = (int)(sizeof(ChainState) / 16);
	const uint4 *init = reinterpret_cast<const uint4 *>(R.chain_init);
	for (int a = 0; a < R.n_active; a++)
		for (int i = ln; i < kChunks; i += 64)
			reinterpret_cast<uint4 *>(&R.states[a][s])[i] = init[i];
	if (R.whbX)
		for (int i = ln; i < kChunks; i += 64)
			reinterpret_cast<uint4 *>(&R.whbX[s])[i] = init[i];
	if (ln == 0) {
		// In place: every kernel of the submits before this one that reads scfg has ended (launch_resets)
		const StreamCfg sc = R.cfgs[blockIdx.x];
		R.scfg[s] = sc;
		R.fsk[s] = FskState{ sc.thresh, 0, 0, -(1 << 28) };  // auto: 500, fm_demod.cpp:23-27, as tfrec_amd_create
		if (R.lev)
			R.lev[s] = LevelState{ sc.thresh, 0, 0, -(1 << 28) };
		if (R.cap)
			R.cap[s] = CaptureState{ sc.thresh, 0, 0, -(1 << 28) };
		if (R.tcarry)
			for (int a = 0; a < R.n_active; a++)
				R.tcarry[(size_t)a * R.n_streams + s] = 0;
		if (R.whbx) {
			R.whbx[s] = WhbExact{ 0.0, 0.0, 0, 0, 0, 0 };
			R.whbcarry[s] = 0;
		}
	}
}
}  // namespace tfrec

namespace {
struct PoisonGuard {
	tfrec_amd_ctx *c;
	bool ok = false;
	explicit PoisonGuard(tfrec_amd_ctx *c_) : c(c_) {}
	~PoisonGuard()
	{
		if (!ok)
			c->poisoned = true;
	}
};
}  // namespace

// ---- biquad coefficients (iir2::set, dsp_stuff.cpp:36-45) in the arithmetic of the reference's normative
// build (oracle/tfrec_oracle.c header).  The five cut-offs the reference ever instantiates
// (main.cpp:186-217, tfa2.cpp:321, whb.cpp:610-611) come from a table of the exact values that build
// produces, so they do not depend on this host's libm tan(); other cut-offs use the formula.
static BiquadCoef biquad_coef(double cutoff)
{
	static const struct {
		double cutoff, b0, a1, a2;
	} known[] = {
		{ 0.5 / (384000.0 / 17240), 0x1.27f98b1037a14p-8, 0x1.cd1527f4a26e2p+0, -0x1.a36a1c41c6995p-1 },
		{ 0.5 / (384000.0 / 9600), 0x1.7ed02b18a270dp-10, 0x1.e397ac010fc89p+0, -0x1.ca2cf85850d62p-1 },
		{ 0.5 / (384000.0 / 8842), 0x1.461fa1a309718p-10, 0x1.e5d4f47377e30p+0, -0x1.ce36282a35d90p-1 },
		{ 2.0 / 64.0, 0x1.14a67102a1ffdp-7, 0x1.b949652fa3970p+0, -0x1.83dd316f714e0p-1 },
		{ 0.0025 / 64.0, 0x1.02ae4cfc8910ap-26, 0x1.ffe9409fe171bp+0, -0x1.ffd283451f7d3p-1 },
	};
	BiquadCoef c;
	for (const auto &k : known)
		if (k.cutoff == cutoff) {
			c.b0 = k.b0;
			c.b1 = k.b0 + k.b0;
			c.b2 = k.b0;
			c.a1 = k.a1;
			c.a2 = k.a2;
			return c;
		}
	const double i = 1.0 / tan(cutoff * M_PI);
	const double s = sqrt(2.0);
	const double b0 = 1.0 / ((i + s) * i + 1.0);
	const double t = i * i - 1.0;
	c.b0 = b0;
	c.b1 = b0 + b0;
	c.b2 = b0;
	c.a1 = (t + t) * b0;
	c.a2 = ((s - i) * i - 1.0) * b0;
	return c;
}

static int d2i_host(double v)
{
	if (!(v > -2147483649.0 && v < 2147483648.0))
		return (int)0x80000000;
	return (int)v;
}

// The discriminator samples the device decided with its exact slow path (fm_resolve.h), checked against the libm of
// THIS host -- the arithmetic the reference binary would use here (dsp_stuff.cpp:284-292 as compiled: DESIGN.md 1).
static void account_fm_log(FmTotals *t, const EventBuf &eb)
{
	t->resolved += eb.uncertain;
	t->undecidable += eb.fm_undecidable;
	const uint32_t n = std::min<uint32_t>(eb.fm_logged, (uint32_t)kFmLogCap);
	const double scale = 16384.0 * (1.0 / M_PI);
	for (uint32_t k = 0; k < n; k++) {
		const int want = d2i_host(atan2(eb.fm_log[k].cj, eb.fm_log[k].cr) * scale);
		t->verified++;
		if (want != eb.fm_log[k].result)
			t->mismatch++;
	}
}

// ---- checks shared by the entry points
static int check_live(const tfrec_amd_ctx *c)
{
	if (!c->poisoned)
		return TFREC_AMD_OK;
	snprintf(g_err, sizeof(g_err), "an earlier submit failed half way: the context must be recreated");
	return TFREC_AMD_E_STATE;
}

static int check_stream(const tfrec_amd_ctx *c, int32_t s)
{
	if (s >= 0 && s < c->cfg.n_streams)
		return TFREC_AMD_OK;
	snprintf(g_err, sizeof(g_err), "stream index %d outside [0, %d)", (int)s, c->cfg.n_streams);
	return TFREC_AMD_E_INVAL;
}

static int check_fifo(const tfrec_amd_ctx *c)
{
	if (c->inflight < kSets)
		return TFREC_AMD_OK;
	snprintf(g_err, sizeof(g_err), "%d submits are waiting to be drained: call tfrec_amd_drain_events first", kSets);
	return TFREC_AMD_E_STATE;
}

// ---- what a context owns: every buffer, stream and event of tfrec_amd_create is made by one of these, which record it
template <class T>
static int own_device(tfrec_amd_ctx *c, T *&p, size_t bytes)
{
	void *h = nullptr;
	if (hipMalloc(&h, bytes) != hipSuccess) {
		snprintf(g_err, sizeof(g_err), "hipMalloc(%zu) failed", bytes);
		return TFREC_AMD_E_NOMEM;
	}
	c->owned.push_back({ tfrec_amd_ctx::Owned::kDevice, h });
	c->dev_bytes += bytes;
	p = static_cast<T *>(h);
	return TFREC_AMD_OK;
}

template <class T>
static int own_pinned(tfrec_amd_ctx *c, T *&p, size_t bytes)
{
	void *h = nullptr;
	if (hipHostMalloc(&h, bytes, hipHostMallocDefault) != hipSuccess) {
		snprintf(g_err, sizeof(g_err), "hipHostMalloc(%zu) failed", bytes);
		return TFREC_AMD_E_NOMEM;
	}
	c->owned.push_back({ tfrec_amd_ctx::Owned::kPinned, h });
	c->pinned_bytes += bytes;
	p = static_cast<T *>(h);
	return TFREC_AMD_OK;
}

static int own_stream(tfrec_amd_ctx *c, hipStream_t &st, int prio)
{
	HIPCHK(hipStreamCreateWithPriority(&st, hipStreamNonBlocking, prio));
	c->owned.push_back({ tfrec_amd_ctx::Owned::kStream, st });
	return TFREC_AMD_OK;
}

static int own_event(tfrec_amd_ctx *c, hipEvent_t &e, unsigned flags)
{
	HIPCHK(hipEventCreateWithFlags(&e, flags));
	c->owned.push_back({ tfrec_amd_ctx::Owned::kEvent, e });
	return TFREC_AMD_OK;
}

// everything recorded, newest first, and tfrec_amd_submit_host's staging
static void release_all(tfrec_amd_ctx *c)
{
	for (auto it = c->owned.rbegin(); it != c->owned.rend(); ++it)
		switch (it->kind) {
		case tfrec_amd_ctx::Owned::kDevice: (void)hipFree(it->h); break;
		case tfrec_amd_ctx::Owned::kPinned: (void)hipHostFree(it->h); break;
		case tfrec_amd_ctx::Owned::kStream: (void)hipStreamDestroy(static_cast<hipStream_t>(it->h)); break;
		case tfrec_amd_ctx::Owned::kEvent: (void)hipEventDestroy(static_cast<hipEvent_t>(it->h)); break;
		}
	c->owned.clear();
	for (uint8_t *&p : c->d_stage) {
		(void)hipFree(p);
		p = nullptr;
	}
}

// constructor state of a chain: tfa1.cpp:136-141, tfa2.cpp:316-334, whb.cpp:605-623, decoders :36-45/:54-62/:77-107
static ChainState chain_init_state()
{
	ChainState st;
	memset(&st, 0, sizeof(st));
	st.sr_cnt = -1;
	st.dmin = 32767;
	st.dmax = -32767;
	return st;
}

// A stream's settings as the kernels read them: the active slots (launch order) of its types, its threshold (auto: 500, where
// its FskState starts), its longest window, its taps
// second-stage taps: dsp_stuff.cpp:61-88 (narrow) / :91-117 (wide, -W)
static const int16_t kNarrowTaps[20] = { -1087, -1082, -1065, -451, 912, 2997, 5556, 8157, 10285, 11484,
					 11484, 10285, 8157, 5556, 2997, 912, -451, -1065, -1082, -1087 };
static const int16_t kWideTaps[20] = { 546, 451, -317, -1844, -3198, -2817, 494, 6469, 13074, 17421,
				       17421, 13074, 6469, 494, -2817, -3198, -1844, -317, 451, 546 };

// The resampling stage's tap table (tfrec_amd/resample.py restates it): h[phi][n], phi < q, n < t = 2 ceil(3 p / q).
// With dn = (n - t/2 + 1) q - phi the tap offset is d = dn / q and d / r = dn / p:
//   g = sinc(dn / p) (0.54 + 0.46 cos(2 pi dn / (q t))),  v = g 65536 / sum g,  h = round(v), and the residual 65536 - sum h goes to
//   the tap with the largest v (the lowest n among equals).
// false: the rate is outside 1 < p/q < 10, q <= 64, gcd = 1, or refused -- a v within 1e-9 of a rounding tie (the table must not
// depend on the host's libm), or max_phi sum |h| * 8192 >> 16 >= 32768 (the int16 store could wrap).
static bool resample_table(int32_t p, int32_t q, std::vector<int32_t> &h, int &t)
{
	if (p <= 0 || q <= 0 || q > kRateQMax || p <= q || (long long)p >= 10LL * q)
		return false;
	for (int a = p, b = q; b;) {  // gcd
		const int r = a % b;
		a = b;
		b = r;
		if (!b && a != 1)
			return false;
	}
	t = 2 * ((3 * p + q - 1) / q);
	h.assign((size_t)q * t, 0);
	std::vector<double> v((size_t)t);
	for (int phi = 0; phi < q; phi++) {
		double total = 0.0;
		for (int n = 0; n < t; n++) {
			const double dn = (double)((n - t / 2 + 1) * q - phi);
			const double u = M_PI * dn / p;
			v[n] = (dn == 0.0 ? 1.0 : sin(u) / u) * (0.54 + 0.46 * cos(2.0 * M_PI * dn / ((double)q * t)));
			total += v[n];
		}
		long long sum = 0, sum_abs = 0;
		int best = 0;
		for (int n = 0; n < t; n++) {
			v[n] = v[n] * 65536.0 / total;
			if (fabs(fabs(v[n] - floor(v[n])) - 0.5) < 1e-9)
				return false;
			const int32_t r = (int32_t)floor(v[n] + 0.5);
			h[(size_t)phi * t + n] = r;
			sum += r;
			if (v[n] > v[best])
				best = n;
		}
		h[(size_t)phi * t + best] += (int32_t)(65536 - sum);
		for (int n = 0; n < t; n++)
			sum_abs += llabs((long long)h[(size_t)phi * t + n]);
		if (((sum_abs * 8192) >> 16) >= 32768)
			return false;
	}
	return true;
}

static StreamCfg device_cfg(const tfrec_amd_ctx *c, const tfrec_amd_stream_config &sc)
{
	StreamCfg d;
	memset(&d, 0, sizeof(d));
	for (int a = 0; a < c->launch.n_active; a++)
		if (sc.types_mask & (1 << c->launch.params[a].sensor_type)) {
			d.amask |= 1u << a;
			d.wmax = std::max(d.wmax, (int32_t)c->launch.params[a].window);
		}
	d.thresh = sc.thresh ? sc.thresh : 500;
	d.autoth = sc.thresh == 0;
	d.wide = (uint16_t)sc.filter_type;
	return d;
}

// ================================================================================ tfrec_amd_create, step by step
static int validate(const tfrec_amd_config *cfg)
{
	if (cfg->n_streams < 1 || cfg->n_streams > 65535 || cfg->max_blocks < 1 || cfg->max_blocks > 4096 ||
	    cfg->max_events < 1 || (cfg->types_mask & 0x2f) == 0 || (cfg->types_mask & ~0x2f) != 0 ||
	    cfg->filter_type < 0 || cfg->filter_type > 1) {
		snprintf(g_err, sizeof(g_err), "bad config");
		return TFREC_AMD_E_INVAL;
	}
	if (cfg->thresh < 0) {
		snprintf(g_err, sizeof(g_err), "thresh must be >= 0 (0 = the reference's auto mode)");
		return TFREC_AMD_E_INVAL;
	}
	int ndev = 0;
	if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
		snprintf(g_err, sizeof(g_err), "no HIP device available");
		return TFREC_AMD_E_HIP;
	}
	if (cfg->device < 0 || cfg->device >= ndev)
		return TFREC_AMD_E_INVAL;
	return TFREC_AMD_OK;
}

// the parameters of a chain of protocol kind `kind` (0 TFA_1, 1 TFA_2 family, 2 WHB) at `baud`
static int chain_params(ChainParams &p, int kind, double baud)
{
	if (kind == 0) {
		p.window = 400;  // 40*BITPERIOD, tfa1.cpp:34, 148
		p.spb = 10;
		return TFREC_AMD_OK;
	}
	p.spb = (1536000 / 4.0) / baud;
	if (kind == 1) {
		p.window = d2i_host(16 * p.spb);  // tfa2.cpp:355
		// multiplier form of numbits (ChainParams::nb_mul), accepted only if it reproduces the fp64 expression
		// for every argument the slicer can form
		const int hmax = (int)(16 * p.spb) + 2;
		const uint64_t a0 = (uint64_t)((double)(1ull << 40) / p.spb);
		for (uint64_t a_try : { a0, a0 + 1, a0 - 1 }) {
			bool ok = true;
			for (int h = 0; h <= hmax && ok; h++)
				ok = tfa2_numbits_mul(2 * h, a_try) == (int)(((double)h + p.spb / 2) / p.spb);
			if (ok) {
				p.nb_mul = a_try;
				break;
			}
		}
		p.td_lo = (int)floor(p.spb / 4) + 1;
		p.td_hi = (int)ceil(32 * p.spb) - 1;
		p.iir = biquad_coef(0.5 / p.spb);  // tfa2.cpp:321
		return TFREC_AMD_OK;
	}
	// whb_demod_kernel's candidate walk has the reference's 64 samples per bit (main.cpp:217) built in (chains2.hip: kWhbSpb)
	if (p.spb != 64.0) {
		snprintf(g_err, sizeof(g_err), "WHB chain with %.3f samples per bit: only 64 is built", p.spb);
		return TFREC_AMD_E_INVAL;
	}
	p.window = d2i_host(8 * p.spb);         // whb.cpp:641
	p.iir = biquad_coef(2.0 / p.spb);       // whb.cpp:610
	p.iir_avg = biquad_coef(0.0025 / p.spb); // whb.cpp:611
	return TFREC_AMD_OK;
}

// the chains of cfg->types_mask in registration order (types and samples-per-bit of main.cpp:173-218), their state arrays
static int register_chains(tfrec_amd_ctx *c)
{
	static const struct {
		int sensor_type, kind, min_bytes;
		double baud;
	} reg[kNSlots] = { { 0, 0, 10, 0 }, { 1, 1, 7, 17240 }, { 2, 1, 7, 9600 }, { 3, 1, 7, 8842 }, { 5, 2, 11, 6000 } };
	const size_t n = (size_t)c->cfg.n_streams;
	const std::vector<ChainState> init(n, chain_init_state());
	for (int s = 0; s < kNSlots; s++) {
		if (!(c->cfg.types_mask & (1 << reg[s].sensor_type)))
			continue;
		const int a = c->launch.n_active++;
		c->launch.slot[a] = s;
		ChainParams &p = c->launch.params[a];
		memset(&p, 0, sizeof(p));
		p.kind = reg[s].kind;
		p.sensor_type = reg[s].sensor_type;
		p.min_bytes = reg[s].min_bytes;
		TRY(chain_params(p, p.kind, reg[s].baud));
		TRY(own_device(c, c->launch.states[a], n * sizeof(ChainState)));
		HIPCHK(hipMemcpy(c->launch.states[a], init.data(), n * sizeof(ChainState), hipMemcpyHostToDevice));
		c->wmax = std::max(c->wmax, (int)p.window);
	}
	return TFREC_AMD_OK;
}

// the front end: its taps, outputs (one set per submit in flight), FIR history, the auto threshold and every stream's settings
static int make_front_buffers(tfrec_amd_ctx *c)
{
	const tfrec_amd_config &cfg = c->cfg;
	const size_t m_max = (size_t)cfg.max_blocks * kBlockDec;
	const size_t n = (size_t)cfg.n_streams;
	// second-stage taps (kNarrowTaps / kWideTaps), as h / 65536
	for (int k = 0; k < 20; k++) {
		c->taps.f2[k][0] = c->taps.f2[k][1] = (float)(cfg.filter_type ? kWideTaps[k] : kNarrowTaps[k]) / 65536.0f;
		c->taps.w[k][0] = c->taps.w[k][1] = (float)kWideTaps[k] / 65536.0f;
	}
	c->taps.scfg = nullptr;
	c->dec_stride = m_max;
	c->mask_stride = m_max / 64;
	for (int k = 0; k < kSets; k++) {
		TRY(own_device(c, c->d_dec[k], n * c->dec_stride * sizeof(uint32_t) + 256));  // + slack: K3 loads whole 32-sample chunks at window tails
		TRY(own_device(c, c->d_mask[k], n * c->mask_stride * sizeof(unsigned long long)));
	}
	// fm_demod.cpp:23-27: thresh 0 selects the adaptive mode starting at 500.  Every stream starts with the context's settings.
	TRY(own_device(c, c->d_fsk, n * sizeof(FskState)));
	TRY(own_device(c, c->d_scfg, n * sizeof(StreamCfg)));
	const tfrec_amd_stream_config sc0 = { cfg.types_mask, cfg.thresh, cfg.filter_type, 0 };
	c->scfg_api.assign(n, sc0);
	c->scfg.assign(n, device_cfg(c, sc0));
	c->n_auto = cfg.thresh == 0 ? (int)n : 0;
	const std::vector<FskState> fsk(n, FskState{ c->scfg[0].thresh, 0, 0, -(1 << 28) });
	HIPCHK(hipMemcpy(c->d_fsk, fsk.data(), n * sizeof(FskState), hipMemcpyHostToDevice));
	HIPCHK(hipMemcpy(c->d_scfg, c->scfg.data(), n * sizeof(StreamCfg), hipMemcpyHostToDevice));
	for (int k = 0; k < kSets; k++) {
		TRY(own_device(c, c->d_fmdev[k], n * m_max * sizeof(int16_t) + 256));  // + slack: K3 reads whole dwords past an odd tail
		TRY(own_device(c, c->d_prevdec[k], n * sizeof(uint32_t)));
	}
	c->in10x = (cfg.flags & TFREC_AMD_F_INPUT_10X) != 0;
	c->in16 = c->in10x || c->resamp || c->ingest;
	const size_t tail_bytes = c->in16 ? 2 * (size_t)kTailBytes : (size_t)kTailBytes;  // int16 history is twice as wide
	// zero FIR history == u8 value 128 (decimate::decimate zeroes hist0, dsp_stuff.cpp:145-152); int16 history of the 10x
	// path: zero, raw u8 history of its 10:1 stage (or of the resampling stage): 128
	for (int k = 0; k < 2; k++) {
		TRY(own_device(c, c->d_tail[k], n * tail_bytes));
		HIPCHK(hipMemset(c->d_tail[k], c->in16 ? 0 : 0x80, n * tail_bytes));
	}
	if (c->in16) {  // stage 0 and the pre-stage's history: raw u8 (silence is 128) or, a rate context in another format, x
		c->in16_stride = 4 * m_max;  // complex samples at 1.536 MS/s per stream and submit
		for (int k = 0; k < kSets; k++)
			TRY(own_device(c, c->d_in16[k], n * c->in16_stride * sizeof(uint32_t)));
		const bool raw = c->fmt == TFREC_AMD_FMT_U8;
		c->pre_bytes = c->in10x ? k10xTail : c->ingest ? 0 : raw ? kRateTail : kFmtTail;
		c->pre_fill = raw ? 0x80 : 0;
		for (int k = 0; c->pre_bytes && k < (c->in10x ? kSets : 2); k++) {  // (the 10x context has always owned one per set)
			TRY(own_device(c, c->d_pre[k], n * c->pre_bytes));
			HIPCHK(hipMemset(c->d_pre[k], c->pre_fill, n * c->pre_bytes));
		}
	}
	if (c->resamp) {
		std::vector<int32_t> h;
		int t = 0;
		if (!resample_table(c->rate_p, c->rate_q, h, t))  // (tfrec_amd_create_rate checked it already)
			return TFREC_AMD_E_INVAL;
		c->rate_t = t;
		for (int phi = 0; phi < c->rate_q; phi++) {
			long long a = 0;
			for (int k = 0; k < t; k++)
				a += llabs((long long)h[(size_t)phi * t + k]);
			c->rate_abs = std::max(c->rate_abs, a);
		}
		std::vector<float> hf(h.size());
		for (size_t i = 0; i < h.size(); i++)
			hf[i] = (float)h[i] * (1.0f / 1024.0f);  // exact: |h| < 2^17
		TRY(own_device(c, c->d_rtaps, hf.size() * sizeof(float)));
		HIPCHK(hipMemcpy(c->d_rtaps, hf.data(), hf.size() * sizeof(float), hipMemcpyHostToDevice));
	}
	return TFREC_AMD_OK;
}

// One set's window tables (chains2.hip): the rows and counters of every chain carved out of one block
static int make_win_tables(tfrec_amd_ctx *c, int set)
{
	const size_t m_max = (size_t)c->cfg.max_blocks * kBlockDec;
	const size_t n = (size_t)c->cfg.n_streams;
	const size_t chains = (size_t)c->launch.n_active * n;
	const bool whb = has_kind(c->launch, 2);
	WinTables &T = c->win[set];
	T.cap = (int32_t)(m_max / 356 + 2);  // windows of one chain are > W-1 >= 355 samples apart
	T.slots = (int32_t)(m_max / 32 + (size_t)T.cap + 2);  // window-relative 32-sample slots per chain row
	if ((size_t)T.slots > (size_t)kWhbRecOffMask) {  // WhbStepRec::meta packs a slot index into kWhbRecOffMask's bits
		snprintf(g_err, sizeof(g_err), "max_blocks too large for the WHB step records");
		return TFREC_AMD_E_INVAL;
	}
	// rows only for the chains that use them: ld16 for the TFA_2 family (its slots are adjacent in registration order),
	// checkpoints for the chains with a biquad stage (all but TFA_1, which is registered first)
	int a_ld0 = -1, n_ld = 0, a_ck0 = -1;
	for (int a = 0; a < c->launch.n_active; a++) {
		if (c->launch.params[a].kind == 1) {
			if (a_ld0 < 0)
				a_ld0 = a;
			n_ld = a - a_ld0 + 1;
		}
		if (c->launch.params[a].kind != 0 && a_ck0 < 0)
			a_ck0 = a;
	}
	T.ld_c0 = (int32_t)((a_ld0 < 0 ? 0 : a_ld0) * n);
	T.ck_c0 = (int32_t)((a_ck0 < 0 ? 0 : a_ck0) * n);
	const size_t ck_chains = a_ck0 < 0 ? 0 : chains - (size_t)a_ck0 * n;
	TRY(own_device(c, c->d_ld16[set], std::max<size_t>(1, (size_t)n_ld * n) * (size_t)T.slots * 32 * sizeof(int16_t)));
	if (whb)  // + slack: whb_demod_kernel keeps three 64-sample steps in flight past a row's last window (whb_demod.h)
		TRY(own_device(c, c->d_dev32[set], n * (size_t)T.slots * 32 * sizeof(int32_t) + 4096));
	T.bit_words = (int32_t)(m_max / 64 + 3 * (size_t)T.cap + 8);
	const size_t wins = chains * (size_t)T.cap;
	size_t off = 0;
	auto carve = [&](size_t bytes) {
		const size_t o = off;
		off += (bytes + 255) & ~(size_t)255;
		return o;
	};
	const size_t o_count = carve(chains * 4), o_cont = carve(chains * 4), o_tnext = carve(chains * 4);
	const size_t o_open = carve(wins * 4), o_close = carve(wins * 4), o_res = carve(wins * sizeof(WinResult));
	const size_t o_dcd = carve(wins * sizeof(WinDecode)), o_wst = carve(whb ? n * (size_t)T.cap * sizeof(WhbStart) : 0);
	const size_t o_bits = carve(chains * (size_t)T.bit_words * 4), o_items = carve((kNQueues * wins + chains) * sizeof(uint2));
	const size_t o_queue = carve((kNQueues + 1) * sizeof(WorkQueue)), o_stats = carve(128);
	T.segcap = (int32_t)((m_max / 32 + (size_t)T.cap) / kSegSlots + 2);
	const size_t segs = chains * (size_t)T.segcap;
	const size_t o_ckpt = carve(ck_chains * (size_t)T.slots * sizeof(double2));
	const size_t o_sstart = carve(segs * sizeof(uint2)), o_vtotal = carve(chains * 4);
	const size_t o_se1 = carve(segs * sizeof(BiquadEnd)), o_se2 = carve(segs * sizeof(BiquadEnd)), o_sfix = carve(segs * 4);
	const size_t o_se3 = carve(segs * sizeof(BiquadEnd)), o_sfix2 = carve(segs * 4);
	const size_t o_cand = carve(n * (size_t)T.slots * 4), o_mark = carve(n * (size_t)T.slots * sizeof(MarkPiece));
	T.whbrec_stride = (int32_t)(m_max / 64 + 2 * (size_t)T.cap + 2 + kWhbRecSlack);
	const size_t o_wrec = carve(whb ? n * (size_t)T.whbrec_stride * sizeof(WhbStepRec) : 0), o_wfail = carve(whb ? n * 4 : 0);
	const size_t o_wsnap = carve(whb ? n * sizeof(ChainState) : 0), o_wx0 = carve(whb ? n * sizeof(WhbExact) : 0);
	const size_t o_wseen = carve(whb ? n * 4 : 0);
	T.whbdense_stride = (int32_t)(m_max + 64);
	T.whbx_stride = (int32_t)(m_max / 64 + 2);
	const size_t o_wdn = carve(whb ? n * 4 : 0), o_wxb = carve(whb ? n * (size_t)T.whbx_stride * 8 : 0);
	const size_t o_wxs = carve(whb ? n * (size_t)T.whbx_stride * sizeof(double2) : 0);
	const size_t o_wdense = carve(whb ? n * (size_t)T.whbdense_stride * 4 : 0);
	TRY(own_device(c, c->win_block[set], off));
	uint8_t *b = (uint8_t *)c->win_block[set];
	T.count = (int32_t *)(b + o_count);
	T.cont = (int32_t *)(b + o_cont);
	T.timeout_next = (int32_t *)(b + o_tnext);
	T.open = (int32_t *)(b + o_open);
	T.close = (int32_t *)(b + o_close);
	T.result = (WinResult *)(b + o_res);
	T.decode = (WinDecode *)(b + o_dcd);
	T.whbstart = (WhbStart *)(b + o_wst);
	T.bits = (uint32_t *)(b + o_bits);
	T.items = (uint2 *)(b + o_items);
	T.queue = (WorkQueue *)(b + o_queue);
	T.overflow = nullptr;  // lives in the set's event block (kEvOverflowOff): make_event_blocks, reset by every submit
	T.stats = (unsigned long long *)(b + o_stats);
	T.ckpt = (double2 *)(b + o_ckpt);
	T.segstart = (uint2 *)(b + o_sstart);
	T.vtotal = (int32_t *)(b + o_vtotal);
	T.segend1 = (BiquadEnd *)(b + o_se1);
	T.segend2 = (BiquadEnd *)(b + o_se2);
	T.segfix = (int32_t *)(b + o_sfix);
	T.segend3 = (BiquadEnd *)(b + o_se3);
	T.segfix2 = (int32_t *)(b + o_sfix2);
	T.cand = (uint32_t *)(b + o_cand);
	T.mark = (MarkPiece *)(b + o_mark);
	T.whbrec = (WhbStepRec *)(b + o_wrec);
	T.whbfail = (int32_t *)(b + o_wfail);
	T.whbsnap = (ChainState *)(b + o_wsnap);
	T.whbx0 = (WhbExact *)(b + o_wx0);
	T.whbseen = (uint32_t *)(b + o_wseen);
	T.whbdense = (int32_t *)(b + o_wdense);
	T.whbdense_n = (int32_t *)(b + o_wdn);
	T.whbxbits = (unsigned long long *)(b + o_wxb);
	T.whbxsnap = (double2 *)(b + o_wxs);
	T.whbgen = c->d_whbgen;
	T.whbX = c->d_whbX;
	T.whbscr = c->d_whbscr;
	T.whbpub = nullptr;
	T.whb_test_perturb = c->whb_test_perturb;
	T.tfa1_vec = TFREC_KNOB_INT("TFA1_VEC", 1, 0, 1) != 0;
	T.tfa2_vec = TFREC_KNOB_INT("TFA2_VEC", 1, 0, 1) != 0;
	T.whb_force_fail = c->whb_force_fail;
	T.whbx = c->d_whbx;
	T.timeout_carry = c->d_tcarry;
	T.prevdec = c->d_prevdec[set];
	HIPCHK(hipMemset(T.queue, 0, (kNQueues + 1) * sizeof(WorkQueue)));
	HIPCHK(hipMemset(T.stats, 0, 128));
	return TFREC_AMD_OK;
}

// the window-parallel pipeline's carried state (the window scan's timeout carry, the WHB check's) and every set's window tables
static int make_window_state(tfrec_amd_ctx *c)
{
	const size_t n = (size_t)c->cfg.n_streams;
	const size_t chains = (size_t)c->launch.n_active * n;
	TRY(own_device(c, c->d_tcarry, chains * 4));
	HIPCHK(hipMemset(c->d_tcarry, 0, chains * 4));
	if (has_kind(c->launch, 2)) {  // iir_avg starts from zero like every iir2 (dsp_stuff.cpp:28-34)
		TRY(own_device(c, c->d_whbx, n * sizeof(WhbExact)));
		TRY(own_device(c, c->d_whbcarry, n * sizeof(int)));
		TRY(own_device(c, c->d_whbgen, n * sizeof(uint32_t)));
		TRY(own_device(c, c->d_whbX, n * sizeof(ChainState)));
		TRY(own_device(c, c->d_whbscr, n * sizeof(ChainState)));
		HIPCHK(hipMemset(c->d_whbgen, 0, n * sizeof(uint32_t)));
		HIPCHK(hipMemset(c->d_whbx, 0, n * sizeof(WhbExact)));
		HIPCHK(hipMemset(c->d_whbcarry, 0, n * sizeof(int)));
		// TEST hooks (results stay exact under both: the check's tolerance and the ambiguity rule widen with D, and a forced
		// failure is only a redo) -- clamped, and never silent: a stray variable changes the redo rate, i.e. the speed
		if (const char *tp = TFREC_KNOB_STR("WHB_TEST_PERTURB"))
			c->whb_test_perturb = std::max(-1000000, std::min(1000000, atoi(tp)));
		if (const char *ff = TFREC_KNOB_STR("WHB_FORCE_FAIL"))
			c->whb_force_fail = std::max(0, atoi(ff));
#if TFREC_KNOBS_BUILT
		if (c->whb_test_perturb || c->whb_force_fail)
			fprintf(stderr, "tfrec_amd: TEST hook active (TFREC_AMD_WHB_TEST_PERTURB=%d, TFREC_AMD_WHB_FORCE_FAIL=%d): WHB streams are "
					"redone on purpose, results unchanged, throughput lower\n", c->whb_test_perturb, c->whb_force_fail);
#endif
		HIPCHK(whb_chain_lds_optin());  // (a per-device attribute: this context's device is the current one)
	}
	for (int set = 0; set < kSets; set++)
		TRY(make_win_tables(c, set));
	return TFREC_AMD_OK;
}

// One event block per set: [EventBuf | the window tables' overflow flag, 16 B | pad to 256 | events] on the device and a
// page-locked copy (the drain's device-to-host copy of a submit is ONE copy on the stream that sets the batch period: three
// copies were 0.45 ms of it with their gaps); the fresh header every submit starts from; the reset lists
static int make_event_blocks(tfrec_amd_ctx *c)
{
	const size_t n = (size_t)c->cfg.n_streams;
	const size_t block = kEvHeader + (size_t)c->cfg.max_events * sizeof(tfrec_amd_event);
	EventBuf eb;
	memset(&eb, 0, sizeof(eb));
	eb.capacity = (uint32_t)c->cfg.max_events;
	for (int k = 0; k < kSets; k++) {
		TRY(own_device(c, c->d_evblock[k], block));
		c->d_eb[k] = (EventBuf *)c->d_evblock[k];
		c->d_events[k] = (tfrec_amd_event *)(c->d_evblock[k] + kEvHeader);
		if (c->win[k].count)  // (window-parallel pipeline: its overflow flag lives behind the EventBuf)
			c->win[k].overflow = (int32_t *)(c->d_evblock[k] + kEvOverflowOff);
		HIPCHK(hipMemset(c->d_evblock[k], 0, kEvHeader));
		HIPCHK(hipMemcpy(c->d_eb[k], &eb, sizeof(eb), hipMemcpyHostToDevice));
	}
	TRY(own_device(c, c->d_eb_fresh, kEvFreshBytes));
	HIPCHK(hipMemset(c->d_eb_fresh, 0, kEvFreshBytes));
	HIPCHK(hipMemcpy(c->d_eb_fresh, &eb, sizeof(eb), hipMemcpyHostToDevice));
	// tfrec_amd_reset_streams: a list of at most n_streams indices per set, and the constructor state it restores
	TRY(own_device(c, c->d_chain_init, sizeof(ChainState)));
	const ChainState init = chain_init_state();
	HIPCHK(hipMemcpy(c->d_chain_init, &init, sizeof(init), hipMemcpyHostToDevice));
	for (int k = 0; k < kSets; k++) {
		TRY(own_device(c, c->d_reset[k], n * sizeof(int32_t)));
		TRY(own_device(c, c->d_rcfg[k], n * sizeof(StreamCfg)));
		TRY(own_device(c, c->d_tune[k], n * sizeof(uint2)));
		TRY(own_device(c, c->d_chan[k], n * sizeof(uint4)));
	}
	for (int k = 0; k < kSets; k++) {
		TRY(own_pinned(c, c->h_evblock[k], block));
		HIPCHK(hipHostGetDevicePointer((void **)&c->h_evblock_dev[k], c->h_evblock[k], 0));
		c->h_eb[k] = (EventBuf *)c->h_evblock[k];
		c->h_events[k] = (tfrec_amd_event *)(c->h_evblock[k] + kEvHeader);
		TRY(own_pinned(c, c->h_reset[k], n * sizeof(int32_t)));
		TRY(own_pinned(c, c->h_rcfg[k], n * sizeof(StreamCfg)));
		TRY(own_pinned(c, c->h_tune[k], n * sizeof(uint2)));
		TRY(own_pinned(c, c->h_chan[k], n * sizeof(uint4)));
	}
	c->tune_hz.assign(n, 0);
	c->tune_inc.assign(n, 0u);
	c->wide_hz.assign(n, 0);
	c->wide_inc.assign(n, 0u);
	c->row.resize(n);
	for (size_t s = 0; s < n; s++)
		c->row[s] = (int32_t)s;
	c->reset_marked.assign(n, 0);
	c->origin.assign(n, 0);
	return TFREC_AMD_OK;
}

// TFREC_AMD_F_LEVELS: the level meter's state (every stream starts like its FskState), records, stream and events
static int make_levels(tfrec_amd_ctx *c)
{
	c->levels = (c->cfg.flags & TFREC_AMD_F_LEVELS) != 0;
	if (!c->levels)
		return TFREC_AMD_OK;
	const size_t n = (size_t)c->cfg.n_streams;
	TRY(own_device(c, c->d_lev, n * sizeof(LevelState)));
	const std::vector<LevelState> lev(n, LevelState{ c->scfg[0].thresh, 0, 0, -(1 << 28) });
	HIPCHK(hipMemcpy(c->d_lev, lev.data(), n * sizeof(LevelState), hipMemcpyHostToDevice));
	for (int k = 0; k < kSets; k++) {
		TRY(own_device(c, c->d_levels[k], n * (size_t)c->cfg.max_blocks * sizeof(tfrec_amd_level)));
		TRY(own_event(c, c->ev_lev[k], hipEventDisableTiming));
	}
	int prio_lo = 0, prio_hi = 0;
	(void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
	TRY(own_stream(c, c->lv, prio_lo));
	return TFREC_AMD_OK;
}

// The stream layout: which streams exist, at which priority, and which are aliases -- into S (every set's PipeCtl starts
// from it) and c->cpy.
//   serial (TFREC_AMD_F_SERIAL_CHAINS): fs, cs, and cp for the drain's copies.
//   shallow (TFREC_AMD_DEEP=0): + t1, aux; the biquad stages and the WHB check are aliases (k2 = cs, kw = aux, vx = aux).
//   deep (the default): + k2, kw of their own, fq and ks (discriminator and speculative pass) when a WHB and a TFA_2-family
//     chain are registered, cq for the drain's copies; the window scan runs at the head of kw (ws) and the WHB check on cp
//     (vx).  Stage A of submit k+1 runs beside stage B of submit k.
// Why (measured):
// - HIP multiplexes the streams of one priority onto GPU_MAX_HW_QUEUES hardware queues (default 4), and two streams that
//   share a queue serialise (profiles/ubench/queues.hip).  The runtime keeps one pool of hardware queues PER PRIORITY:
//   fs / cs / aux / t1 are the high-priority streams, and cp (with k2 / kw in the deep layout) has normal priority -- no pool
//   holds more than four streams, whatever GPU_MAX_HW_QUEUES is.
// - Every pipeline stream except the biquad stages runs at high priority.  With the front end at low priority ("fill what
//   the latency-bound chains leave free") its kernel stretched from 3 to 11 ms beside the chains and, with three submits in
//   flight, became the longest stage of all: 13.4 ms per batch instead of 11.7.  (The biquad stages and cp run at normal
//   priority, 0; the discriminator pass, the TFA_2 family's speculative pass and the drain's copies, when they have streams
//   of their own, at low priority.)
// - The window scan at the head of kw, not behind the front end: the front-end stream is the busiest of all (0.3-1.1 ms less
//   on it per batch).
// - The discriminator pass moves from the front-end stream into the pipeline (the head of the TFA_2-family biquad stage, or
//   fq) when a WHB demodulator is registered: then the WHB chain is the longest and the front-end stream the busiest
//   (measured 12.2 -> 11.8 ms per batch; without WHB the TFA_2 chain is the longest and the move costs 7.7 -> 8.5 ms).
// - fq: the discriminator pass on a LOW-priority stream of its own.  It needs the front end only, not the window scan; at the
//   head of k2 it made that stream (discriminator + five biquad kernels) the one that set the batch period: 6.98 -> 6.60 ms
//   per batch over 100 steps (profiles/r04_ab_fmdev_stream.txt).  The low-priority pool's hardware queues are otherwise
//   unused, so the stream shares none (a fifth normal-priority stream would).
// - ks: the speculative biquad pass of the TFA_2 family on a low-priority stream of its own (when the discriminator pass has
//   its stream): it needs nothing of the submit before (chains2.hip K3a), so it runs beside that submit's repair passes and
//   chain walk on k2.  The third stream of the low-priority pool (with fq and cq): no shared hardware queue.
// - cq: the drain's copies must not queue behind the work of younger submits, so they need a hardware queue of their own.
//   On cp they sat between the WHB checks of consecutive submits and waited for ALL chains of their submit: the check of
//   submit k + 1 could not start before the TFA chains of submit k had ended.  6.32 -> 6.21 ms per batch over
//   100 steps (profiles/r04_ab_copy_stream.txt); the low pool's hardware queues hold only this stream and the
//   discriminator's.
// - vx = cp: the WHB check (whb_chain_kernel, whb_check_kernel, the redo) runs where the drain's copies were until they
//   moved to cq.  A stream of its own would be the FIFTH of normal priority in the process (k2, kw, cp and the caller's): it
//   shared a hardware queue with kw, and the 6 ms verification of submit k held up the WHB biquads of submit k + 2.
static int make_streams(tfrec_amd_ctx *c, PipeCtl &S)
{
	int prio_lo = 0, prio_hi = 0;
	(void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
	hipStream_t cp = nullptr;
	TRY(own_stream(c, S.fs, prio_hi));
	TRY(own_stream(c, cp, 0));
	TRY(own_stream(c, S.cs, prio_hi));
	S.ws = S.fs;
	c->cpy = cp;
	if (c->cfg.flags & TFREC_AMD_F_SERIAL_CHAINS)
		return TFREC_AMD_OK;
	TRY(own_stream(c, S.t1, prio_hi));
	TRY(own_stream(c, S.aux, prio_hi));
	const char *dp = TFREC_KNOB_STR("DEEP");
	c->deep = dp ? atoi(dp) != 0 : true;
	c->fmdev_k2 = has_kind(c->launch, 1) && has_kind(c->launch, 2);
	S.k2 = S.cs;
	S.kw = S.aux;
	S.vx = S.aux;
	if (!c->deep)
		return TFREC_AMD_OK;
	TRY(own_stream(c, S.k2, 0));
	TRY(own_stream(c, S.kw, 0));
	S.ws = S.kw;
	if (c->fmdev_k2) {
		TRY(own_stream(c, S.fq, prio_lo));
		TRY(own_stream(c, S.ks, prio_lo));
	}
	TRY(own_stream(c, c->cpy, prio_lo));
	S.vx = cp;
	return TFREC_AMD_OK;
}

// every set's PipeCtl (the layout's streams, the set's events and buffers) and the set's other events
static int make_pipes(tfrec_amd_ctx *c, const PipeCtl &S)
{
	const bool serial = (c->cfg.flags & TFREC_AMD_F_SERIAL_CHAINS) != 0;
	const bool timing = (c->cfg.flags & TFREC_AMD_F_TIMING) != 0;
	for (int k = 0; k < kSets; k++) {
		PipeCtl &P = c->pipe[k];
		P = S;
		for (hipEvent_t *e : { &P.done[0], &P.done[1], &P.done[2], &P.ev_win, &P.ev_fork, &P.ev_k2, &P.ev_kw, &P.ev_fm,
				       &P.ev_spec, &c->ev_in[k], &P.ev_front, &c->copied[k] })
			TRY(own_event(c, *e, hipEventDisableTiming));
		if (!serial)
			TRY(own_event(c, P.ev_aux, hipEventDisableTiming));
		if (timing) {
			for (hipEvent_t &e : c->ev[k])
				TRY(own_event(c, e, hipEventDefault));
			if (!serial) {
				for (hipEvent_t &e : c->tev[k])
					TRY(own_event(c, e, hipEventDefault));
				P.tev = c->tev[k];
			}
		}
		P.whb_carry = c->d_whbcarry;
		P.fmdev_wmax = c->fmdev_k2 ? c->wmax : 0;
		P.fm_flag_eps = c->fm_flag_eps;
		P.fmdev_out = c->d_fmdev[k];
		P.prevdec = c->d_prevdec[k];
	}
	return TFREC_AMD_OK;
}

static int init_context(tfrec_amd_ctx *c)
{
	if (const char *fe = TFREC_KNOB_STR("FM_FLAG_EPS"))
		c->fm_flag_eps = std::max(1e-9, atof(fe));
	if (const char *cg = TFREC_KNOB_STR("COPY_GUESS_MIN"))
		c->copy_guess = c->copy_guess_min = (uint32_t)std::max(1, atoi(cg));
	TRY(register_chains(c));
	TRY(make_front_buffers(c));
	if (!(c->cfg.flags & TFREC_AMD_F_SERIAL_CHAINS))
		TRY(make_window_state(c));
	TRY(make_event_blocks(c));
	PipeCtl streams = {};
	TRY(make_streams(c, streams));
	TRY(make_pipes(c, streams));
	TRY(make_levels(c));
	return TFREC_AMD_OK;
}

static void print_host_prof(const tfrec_amd_ctx *c)
{
	if (TFREC_KNOB_STR("HOST_PROF") && c->hp_n)
		fprintf(stderr, "tfrec_amd host time per batch: submit %.0f us, drain: wait %.0f + copy %.0f + sort %.0f us (%ld batches)\n",
			1e6 * c->hp_submit / c->hp_n, 1e6 * c->hp_wait / c->hp_n, 1e6 * c->hp_copy / c->hp_n, 1e6 * c->hp_sort / c->hp_n,
			c->hp_n);
	if (TFREC_KNOB_STR("HOST_PROF") && c->hp_gap_n)
		fprintf(stderr, "tfrec_amd front-end stream: %.3f ms between one submit's front end and the next one's; front-end start -> TFA_1 chain end %.2f ms; front-end start to start %.3f ms (%ld batches)\n",
			c->hp_gap / c->hp_gap_n, c->hp_lat / c->hp_gap_n, c->hp_s2s / c->hp_gap_n, c->hp_gap_n);
}

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

int tfrec_amd_destroy(tfrec_amd_ctx *c)
{
	if (!c)
		return TFREC_AMD_OK;
	(void)hipSetDevice(c->cfg.device);
	(void)hipDeviceSynchronize();
	print_host_prof(c);
	release_all(c);
	delete c;
	return TFREC_AMD_OK;
}

int tfrec_amd_create(const tfrec_amd_config *cfg, tfrec_amd_ctx **out)
{
	if (!cfg || !out)
		return TFREC_AMD_E_INVAL;
	*out = nullptr;
	TRY(validate(cfg));
	HIPCHK(hipSetDevice(cfg->device));
	tfrec_amd_ctx *c = new (std::nothrow) tfrec_amd_ctx();
	if (!c)
		return TFREC_AMD_E_NOMEM;
	c->cfg = *cfg;
	const int rc = init_context(c);
	if (rc != TFREC_AMD_OK) {
		tfrec_amd_destroy(c);
		return rc;
	}
	*out = c;
	return TFREC_AMD_OK;
}

int tfrec_amd_resample_taps(int32_t rate_p, int32_t rate_q, int32_t *taps, int cap, int *n_taps_per_phase)
{
	std::vector<int32_t> h;
	int t = 0;
	if (cap < 0 || (cap > 0 && !taps) || !resample_table(rate_p, rate_q, h, t)) {
		snprintf(g_err, sizeof(g_err), "input rate %d/%d: unsupported or refused", (int)rate_p, (int)rate_q);
		return TFREC_AMD_E_INVAL;
	}
	if (n_taps_per_phase)
		*n_taps_per_phase = t;
	if (taps) {
		if ((size_t)cap < h.size())
			return TFREC_AMD_E_INVAL;
		memcpy(taps, h.data(), h.size() * sizeof(int32_t));
	}
	return TFREC_AMD_OK;
}

int tfrec_amd_create_rate(const tfrec_amd_config *cfg, int32_t rate_p, int32_t rate_q, tfrec_amd_ctx **out)
{
	if (!cfg || !out)
		return TFREC_AMD_E_INVAL;
	*out = nullptr;
	if (cfg->flags & TFREC_AMD_F_INPUT_10X) {
		snprintf(g_err, sizeof(g_err), "an input rate and the 15.36 MS/s input flag exclude each other");
		return TFREC_AMD_E_INVAL;
	}
	TRY(tfrec_amd_resample_taps(rate_p, rate_q, nullptr, 0, nullptr));
	TRY(validate(cfg));
	HIPCHK(hipSetDevice(cfg->device));
	tfrec_amd_ctx *c = new (std::nothrow) tfrec_amd_ctx();
	if (!c)
		return TFREC_AMD_E_NOMEM;
	c->cfg = *cfg;
	c->rate_p = rate_p;
	c->rate_q = rate_q;
	c->resamp = true;
	const int rc = init_context(c);
	if (rc != TFREC_AMD_OK) {
		tfrec_amd_destroy(c);
		return rc;
	}
	*out = c;
	return TFREC_AMD_OK;
}

int tfrec_amd_create_format(const tfrec_amd_config *cfg, int32_t format, int32_t rate_p, int32_t rate_q, tfrec_amd_ctx **out)
{
	if (!cfg || !out)
		return TFREC_AMD_E_INVAL;
	*out = nullptr;
	const bool base = rate_p == 1 && rate_q == 1;
	if (format < TFREC_AMD_FMT_U8 || format > TFREC_AMD_FMT_F32) {
		snprintf(g_err, sizeof(g_err), "unknown input format %d", (int)format);
		return TFREC_AMD_E_INVAL;
	}
	if (format == TFREC_AMD_FMT_U8)  // exactly the older constructors
		return base ? tfrec_amd_create(cfg, out) : tfrec_amd_create_rate(cfg, rate_p, rate_q, out);
	if (cfg->flags & TFREC_AMD_F_INPUT_10X) {
		snprintf(g_err, sizeof(g_err), "the 15.36 MS/s input flag takes u8 input only");
		return TFREC_AMD_E_INVAL;
	}
	if (!base)
		TRY(tfrec_amd_resample_taps(rate_p, rate_q, nullptr, 0, nullptr));
	TRY(validate(cfg));
	HIPCHK(hipSetDevice(cfg->device));
	tfrec_amd_ctx *c = new (std::nothrow) tfrec_amd_ctx();
	if (!c)
		return TFREC_AMD_E_NOMEM;
	c->cfg = *cfg;
	c->fmt = format;
	c->rate_p = rate_p;
	c->rate_q = rate_q;
	c->resamp = !base;
	c->ingest = base;
	const int rc = init_context(c);
	if (rc != TFREC_AMD_OK) {
		tfrec_amd_destroy(c);
		return rc;
	}
	*out = c;
	return TFREC_AMD_OK;
}

int tfrec_amd_get_input_format(tfrec_amd_ctx *c, int32_t *format)
{
	if (!c || !format)
		return TFREC_AMD_E_INVAL;
	*format = c->fmt;
	return TFREC_AMD_OK;
}

int tfrec_amd_get_input_rate(tfrec_amd_ctx *c, int32_t *p, int32_t *q)
{
	if (!c || !p || !q)
		return TFREC_AMD_E_INVAL;
	*p = c->in10x ? 10 : c->rate_p;
	*q = c->in10x ? 1 : c->rate_q;
	return TFREC_AMD_OK;
}

// The resets marked since the last submit, at the head of this submit's front end (fs).  Carried state is written by several
// stages on several streams (a ChainState by the biquad stage, the slicers, the decoders' commit and the WHB check's redo), and
// in the deep layout those of the submit before may still run while this one's front end does: the front-end stream first
// waits for the end of every chain of the last submit (its set's done: every stage of it and of all earlier submits is behind
// one of them), then one kernel restores the state of the listed streams.  Every stage of this submit is ordered after its
// front end, so it reads the restored state.  A submit without a pending reset launches nothing of this.
static int launch_resets(tfrec_amd_ctx *c, int set)
{
	hipStream_t fs = c->pipe[set].fs;
	if (c->submitted)
		for (hipEvent_t e : c->pipe[c->last_set].done)
			HIPCHK(hipStreamWaitEvent(fs, e, 0));
	if (c->submitted && c->levels)  // (the level meter of the last submit reads d_scfg and owns d_lev)
		HIPCHK(hipStreamWaitEvent(fs, c->ev_lev[c->last_set], 0));
	if (c->submitted && c->capture)  // (so does the recorder: d_scfg and d_capst)
		HIPCHK(hipStreamWaitEvent(fs, c->ev_cap[c->last_set], 0));
	const int nl = (int)c->reset_pending.size();
	memcpy(c->h_reset[set], c->reset_pending.data(), (size_t)nl * sizeof(int32_t));  // (the set's last copy was drained)
	for (int i = 0; i < nl; i++)  // a reset stream restarts with its own current settings
		c->h_rcfg[set][i] = c->scfg[c->reset_pending[i]];
	HIPCHK(hipMemcpyAsync(c->d_reset[set], c->h_reset[set], (size_t)nl * sizeof(int32_t), hipMemcpyHostToDevice, fs));
	HIPCHK(hipMemcpyAsync(c->d_rcfg[set], c->h_rcfg[set], (size_t)nl * sizeof(StreamCfg), hipMemcpyHostToDevice, fs));
	StreamReset R;
	memset(&R, 0, sizeof(R));
	R.list = c->d_reset[set];
	R.n_list = nl;
	R.n_streams = c->cfg.n_streams;
	R.tail = c->d_tail[c->tail_sel];  // the buffer this submit's front end reads (the history flips per submit)
	R.tail_bytes = c->in16 ? 2 * kTailBytes : kTailBytes;
	R.tail_fill = c->in16 ? 0 : 0x80;  // as make_front_buffers: int16 zero, or u8 128
	R.pre = c->d_pre[c->tail_sel];
	R.pre_bytes = c->pre_bytes;
	R.pre_fill = c->pre_fill;
	R.fsk = c->d_fsk;
	R.lev = c->d_lev;
	R.cap = c->d_capst;
	R.cfgs = c->d_rcfg[set];
	R.scfg = c->d_scfg;
	R.n_active = c->launch.n_active;
	for (int a = 0; a < c->launch.n_active; a++)
		R.states[a] = c->launch.states[a];
	R.chain_init = c->d_chain_init;
	R.tcarry = c->d_tcarry;
	R.whbx = c->d_whbx;
	R.whbcarry = c->d_whbcarry;
	R.whbX = c->d_whbX;
	hipLaunchKernelGGL(tfrec::stream_reset_kernel, dim3(nl), dim3(64), 0, fs, R);
	HIPCHK(hipGetLastError());
	return TFREC_AMD_OK;
}

// Instrumentation builds and knobs: statistics of the third submit, printed to stderr (the host waits for the device first)
static void report_debug_stats(tfrec_amd_ctx *c, int set, int n_blocks)
{
#ifdef TFREC_AMD_VECSTAT
	if (c->submit_seq == 3) {
		(void)hipDeviceSynchronize();
		unsigned long long st[16] = { 0 };
		(void)hipMemcpy(st, c->win[set].stats, sizeof(st), hipMemcpyDeviceToHost);
		fprintf(stderr, "VECSTAT (one submit) TFA_1: groups %llu, stale piece %llu, entered-with-none hazard %llu, > 64 bits in a lane %llu, lanes with 32 ones or more %llu; TFA_2 family: groups %llu, entered with relative 0 %llu, > 16 rounds %llu, > 64 bits in a lane %llu, walks of the groups that converged %llu\n", st[8], st[9], st[10], st[11], st[5], st[12], st[13], st[14], st[15], st[6]);
	}
#endif
#ifdef TFREC_AMD_COOPSTAT
	if (c->submit_seq == 3) {
		(void)hipDeviceSynchronize();
		unsigned long long st[16] = { 0 };
		(void)hipMemcpy(st, c->win[set].stats, sizeof(st), hipMemcpyDeviceToHost);
		fprintf(stderr, "COOPSTAT (one submit) TFA_2 family: frozen one-block steps %llu, accepted %llu, rejected %llu, other frozen steps %llu; TFA_1: steps %llu, candidate runs %llu; TFA_2 walked steps with a full mask %llu, candidates in walked steps %llu, walked steps that begin inside a run %llu\n", st[7], st[8], st[9], st[10], st[11], st[12], st[13], st[14], st[15]);
	}
#endif
	if (TFREC_KNOB_STR("DEBUG_WINHIST") && c->submit_seq == 3) {  // (debug: the window length distribution of one submit)
		(void)hipDeviceSynchronize();
		const WinTables &T = c->win[set];
		const size_t chains = (size_t)c->launch.n_active * c->cfg.n_streams;
		std::vector<int32_t> cnt(chains), op(chains * T.cap), cl(chains * T.cap);
		(void)hipMemcpy(cnt.data(), T.count, chains * 4, hipMemcpyDeviceToHost);
		(void)hipMemcpy(op.data(), T.open, chains * T.cap * 4, hipMemcpyDeviceToHost);
		(void)hipMemcpy(cl.data(), T.close, chains * T.cap * 4, hipMemcpyDeviceToHost);
		const int M = n_blocks * kBlockDec;
		for (int a = 0; a < c->launch.n_active; a++) {
			long hist[16] = { 0 }, nwin = 0, tot = 0;
			for (int s = 0; s < c->cfg.n_streams; s++) {
				const size_t ch = (size_t)a * c->cfg.n_streams + s;
				for (int j = 0; j < cnt[ch]; j++) {
					const int last = cl[ch * T.cap + j] < M ? cl[ch * T.cap + j] : M - 1;
					const int n = last - op[ch * T.cap + j] + 1;
					int b = 0;
					while ((256 << b) <= n && b < 15)
						b++;
					hist[b]++;
					nwin++;
					tot += n;
				}
			}
			fprintf(stderr, "WINHIST slot %d kind %d window %d: %ld windows, %ld samples (%.1f %% of the submit);", a, c->launch.params[a].kind,
				c->launch.params[a].window, nwin, tot, 100.0 * tot / ((double)M * c->cfg.n_streams));
			for (int b = 0; b < 16; b++)
				if (hist[b])
					fprintf(stderr, " <%d:%ld", 256 << b, hist[b]);
			fprintf(stderr, "\n");
		}
	}
	if (TFREC_KNOB_STR("DEBUG_CONVHIST") && c->submit_seq == 3 && !(c->cfg.flags & TFREC_AMD_F_SERIAL_CHAINS)) {
		// (debug: after how many 32-sample slots the first repair run of a biquad segment -- started from the end state of the
		// segment before -- became bit-identical to the segment's own run from a zero state: the convergence-time distribution
		// of the speculation, per chain; a build with -DTFREC_AMD_CK_EVERY=1 resolves it to one slot)
		(void)hipDeviceSynchronize();
		const WinTables &T = c->win[set];
		const size_t chains = (size_t)c->launch.n_active * c->cfg.n_streams;
		std::vector<int32_t> fx(chains * T.segcap), vt(chains);
		(void)hipMemcpy(fx.data(), T.segfix, fx.size() * 4, hipMemcpyDeviceToHost);
		(void)hipMemcpy(vt.data(), T.vtotal, chains * 4, hipMemcpyDeviceToHost);
		for (int a = 0; a < c->launch.n_active; a++) {
			if (c->launch.params[a].kind == 0)
				continue;
			std::vector<long> hist(kSegSlots + 1, 0);
			long nseg = 0, never = 0;
			for (int s = 0; s < c->cfg.n_streams; s++) {
				const size_t ch = (size_t)a * c->cfg.n_streams + s;
				const int ns = (vt[ch] + kSegSlots - 1) / kSegSlots;
				for (int k = 1; k < ns; k++) {
					if (vt[ch] - k * kSegSlots < kSegSlots)
						continue;  // (a chain's short last segment says nothing)
					const int v = fx[ch * T.segcap + k];
					nseg++;
					if (v & kSegConverged)
						hist[std::min(kSegSlots, v & ~(kSegConverged | kSegRan))]++;
					else
						never++;
				}
			}
			fprintf(stderr, "CONVHIST slot %d (window %d, segments of %d slots): %ld full segments, %ld not converged at their end; converged within n slots:",
				c->launch.slot[a], c->launch.params[a].window, kSegSlots, nseg, never);
			long cum = 0;
			for (int n = 1; n <= kSegSlots; n++) {
				cum += hist[n];
				if (n == 4 || n == 8 || n == 12 || n == 16 || n == 20 || n == 24 || n == 32 || n == 40 || n == 48 || n == 64 || n == 96 ||
				    n == 128 || n == 192 || n == 256 || n == 384 || n == 512 || n == 1024)
					fprintf(stderr, " %d:%.4f", n, nseg ? (double)cum / nseg : 0.0);
			}
			fprintf(stderr, "\n");
		}
	}
}

// The tuned front end's per-stream {inc, phase} of this submit, queued on the front-end stream ahead of it.  The
// phase of the submit's first 1.536 MS/s sample n0 (4 per decimated sample, counted from the stream's start or restart --
// 0 for a stream that restarts with this submit) is (n0 * inc) mod 2^32, in 64-bit integers.  h_tune[set] is free: the
// set's previous submit, whose copy read it, has been drained.
static int stage_tune(tfrec_amd_ctx *c, int set)
{
	for (int s = 0; s < c->cfg.n_streams; s++) {
		const uint32_t inc = c->tune_inc[s];
		const long long n0 = c->reset_marked[s] ? 0 : 4 * (c->sample_base - c->origin[s]);
		c->h_tune[set][s] = make_uint2(inc, (uint32_t)((uint64_t)n0 * inc));
	}
	HIPCHK(hipMemcpyAsync(c->d_tune[set], c->h_tune[set], (size_t)c->cfg.n_streams * sizeof(uint2), hipMemcpyHostToDevice,
			      c->pipe[set].fs));
	return TFREC_AMD_OK;
}

// The per-stream {inc10, phase10, input row, 0} of this submit, staged like stage_tune's.  phase10 is the phase of
// the submit's first INPUT sample n0 (40 per decimated sample with TFREC_AMD_F_INPUT_10X): (n0 * inc10) mod 2^32.  A rate
// context (6g): {inc_in, ...} with n0 = 4 P / Q input samples per decimated sample -- whole, because every submit is.
static int stage_chan(tfrec_amd_ctx *c, int set)
{
	for (int s = 0; s < c->cfg.n_streams; s++) {
		const uint32_t inc = c->wide_inc[s];
		const long long rp = c->in10x ? 10 : c->rate_p, rq = c->in10x ? 1 : c->rate_q;
		const long long n0 = c->reset_marked[s] ? 0 : 4 * (c->sample_base - c->origin[s]) * rp / rq;
		c->h_chan[set][s] = make_uint4(inc, (uint32_t)((uint64_t)n0 * inc), (uint32_t)c->row[s], 0u);
	}
	HIPCHK(hipMemcpyAsync(c->d_chan[set], c->h_chan[set], (size_t)c->cfg.n_streams * sizeof(uint4), hipMemcpyHostToDevice,
			      c->pipe[set].fs));
	return TFREC_AMD_OK;
}

// rows of the input batch the streams read: 1 + the highest one mapped
static int rows_in_use(const tfrec_amd_ctx *c)
{
	if (!c->mapped)
		return c->cfg.n_streams;
	return 1 + *std::max_element(c->row.begin(), c->row.end());
}

// Bytes of one input row of a submit of n_blocks blocks: n_blocks * 32768 * P / Q complex samples, which must be a whole
// number (any n_blocks when Q is a power of two, otherwise a multiple of Q's odd part), of 2, 4 or 8 bytes each.
static int input_bytes(const tfrec_amd_ctx *c, int n_blocks, size_t *bytes)
{
	if (n_blocks < 1)
		return TFREC_AMD_E_INVAL;
	const long long p = c->in10x ? 10 : c->rate_p, q = c->in10x ? 1 : c->rate_q;
	const long long num = (long long)n_blocks * (TFREC_AMD_BLOCK_BYTES / 2) * p;
	if (num % q != 0) {
		snprintf(g_err, sizeof(g_err), "%d blocks at the input rate %lld/%lld are not a whole number of input samples", n_blocks, p, q);
		return TFREC_AMD_E_INVAL;
	}
	*bytes = (size_t)(num / q) * fmt_sample_bytes(c->fmt);
	return TFREC_AMD_OK;
}

// The submit's input -> stage 0 (d_in16[set]) on the set's front-end stream.  chan: the set's {inc, phase, row, 0} per stream
// where a stream is mapped or has an input-rate tune (stage_chan), or nullptr.
static int launch_prestage(tfrec_amd_ctx *c, int set, const uint8_t *d_iq, size_t stride, int n_blocks, const uint4 *chan)
{
	hipStream_t fs = c->pipe[set].fs;
	const int n = c->cfg.n_streams;
	const uint8_t *hin = c->d_pre[c->tail_sel];
	uint8_t *hout = c->d_pre[c->tail_sel ^ 1];
	uint32_t *out = c->d_in16[set];
	if (c->in10x)  // 15.36 MS/s u8 -> 1.536 MS/s int16 pairs
		HIPCHK(launch_decim10(fs, d_iq, stride, n, n_blocks, hin, hout, out, c->in16_stride, chan));
	else if (c->ingest)  // 1.536 MS/s in another format -> x as int16 pairs
		HIPCHK(launch_ingest(fs, c->fmt, d_iq, stride, n, n_blocks, out, c->in16_stride, chan));
	else if (c->fmt != TFREC_AMD_FMT_U8)  // 1536000 P / Q S/s in another format: the format-aware resampling stage
		HIPCHK(launch_resample_fmt(fs, c->fmt, d_iq, stride, n, n_blocks, c->rate_p, c->rate_q, c->rate_t, c->d_rtaps, hin, hout, out,
					   c->in16_stride, chan, c->n_wide != 0));
	else  // 1536000 P / Q S/s u8 -> 1.536 MS/s int16 pairs
		HIPCHK(launch_resample(fs, d_iq, stride, n, n_blocks, c->rate_p, c->rate_q, c->rate_t, c->d_rtaps, hin, hout, out, c->in16_stride,
				       chan, c->n_wide != 0));
	return TFREC_AMD_OK;
}

// input_on_fs: the input was produced on the front-end stream itself (staged host input): no event needed
static int submit_common(tfrec_amd_ctx *c, const void *d_iq, size_t stride, int n_blocks, void *hip_stream, bool input_on_fs)
{
	if (!c || !d_iq || n_blocks < 1 || n_blocks > c->cfg.max_blocks)
		return TFREC_AMD_E_INVAL;
	size_t row_bytes = 0;
	TRY(input_bytes(c, n_blocks, &row_bytes));
	if ((stride % 16) != 0 || ((uintptr_t)d_iq % 16) != 0 ||
	    (rows_in_use(c) > 1 && stride < row_bytes)) {  // (one row in use: the stride is never applied)
		snprintf(g_err, sizeof(g_err), "IQ base and stream stride must be 16-byte aligned and >= one stream");
		return TFREC_AMD_E_INVAL;
	}
	TRY(check_fifo(c));
	TRY(check_live(c));
	HIPCHK(hipSetDevice(c->cfg.device));
	PoisonGuard guard(c);  // from here on work is enqueued: a failure leaves the carried state undefined
	const bool timing = (c->cfg.flags & TFREC_AMD_F_TIMING) != 0;
	const int set = (c->head + c->inflight) % kSets;  // this submit's buffer set, events and timing events
	const PipeCtl &P = c->pipe[set];
	hipEvent_t *ev = c->ev[set];
	// Front end on its own stream: it starts when the caller's stream has produced the input, and may overlap the
	// chains of the previous submit (different buffer set; the set's previous user was drained, see the FIFO rule).
	// The chains run on internal streams: nothing of ours is queued on the caller's.
	hipStream_t fs = P.fs;
	if (!input_on_fs) {
		HIPCHK(hipEventRecord(c->ev_in[set], (hipStream_t)hip_stream));
		HIPCHK(hipStreamWaitEvent(fs, c->ev_in[set], 0));
	}
	if (c->spectrum) {
		// the spectrum: it reads the raw rows and nothing else, so it is ordered behind the input's producer alone -- the wait the
		// front end makes, or (staged host input) the copy queued on fs just before -- and runs beside everything, on its own
		// low-priority stream.  The set's records were read or dropped when its previous submit was drained.
		if (input_on_fs)
			HIPCHK(hipEventRecord(c->ev_in[set], fs));
		HIPCHK(hipStreamWaitEvent(c->sp, c->ev_in[set], 0));
		const int rows = std::min(rows_in_use(c), c->spec_rows);
		const long n_in = (long)(row_bytes / fmt_sample_bytes(c->fmt));
		HIPCHK(launch_spectrum(c->sp, c->fmt, (const uint8_t *)d_iq, stride, rows, n_in, c->spec_n, c->spec_g, c->spec_max_records,
				       c->d_spec_sum[set], c->d_spec_peak[set], c->d_spec_nf[set]));
		HIPCHK(hipEventRecord(c->ev_spectrum[set], c->sp));
		c->spec_set_rows[set] = rows;
		c->spec_set_records[set] = (int)((n_in / c->spec_n + c->spec_g - 1) / c->spec_g);
	}
	HIPCHK(hipMemcpyAsync(c->d_eb[set], c->d_eb_fresh, kEvFreshBytes, hipMemcpyDeviceToDevice, fs));  // (+ the overflow flag)
	if (timing)
		HIPCHK(hipEventRecord(ev[kEvSubmit], fs));
	const bool resets = !c->reset_pending.empty();
	if (resets)
		TRY(launch_resets(c, set));
	const uint8_t *fin = (const uint8_t *)d_iq;
	size_t fstride = stride;
	// a mapped or wide-tuned context: the 10:1 stage's tuned kernel, or -- default input -- the front end that looks up the rows
	// (a rate context: the resampling stage looks the row up, as the 10:1 stage does)
	const bool chan10 = c->in16 && (c->mapped || c->n_wide), chan_front = !c->in16 && c->mapped;
	if (chan10 || chan_front)
		TRY(stage_chan(c, set));
	if (c->in16) {  // ... then the standard cascade on int16 input
		TRY(launch_prestage(c, set, (const uint8_t *)d_iq, stride, n_blocks, chan10 ? c->d_chan[set] : nullptr));
		fin = (const uint8_t *)c->d_in16[set];
		fstride = c->in16_stride * sizeof(uint32_t);
	}
	if (c->n_tuned || chan_front)
		TRY(stage_tune(c, set));
	HIPCHK(launch_frontend(fs, fin, fstride, c->cfg.n_streams, n_blocks, c->d_tail[c->tail_sel],
			       c->d_tail[c->tail_sel ^ 1], c->d_dec[set], c->dec_stride, c->d_mask[set], c->mask_stride,
			       c->d_prevdec[set], c->cfg.thresh ? c->cfg.thresh : 500, c->taps, c->in16,
			       (c->n_tuned || chan_front) ? c->d_tune[set] : nullptr, chan_front ? c->d_chan[set] : nullptr));
	if (c->n_auto)  // auto threshold: per-block thresholds rewrite the trigger mask (fm_demod.cpp:58-73)
		HIPCHK(launch_threshold(fs, c->d_dec[set], c->dec_stride, c->d_mask[set], c->mask_stride, c->cfg.n_streams,
					n_blocks, c->d_fsk, c->wmax, c->per_stream ? c->d_scfg : nullptr));
	if (timing)
		HIPCHK(hipEventRecord(ev[kEvFrontDone], fs));
	if (has_kind(c->launch, 1) && !c->fmdev_k2)  // FM discriminator of the samples near trigger windows (after the mask is final)
		HIPCHK(launch_fmdev(fs, c->d_dec[set], c->dec_stride, c->d_mask[set], c->mask_stride, c->d_prevdec[set],
				    c->d_fmdev[set], c->dec_stride, c->d_eb[set], c->cfg.n_streams, n_blocks, c->wmax,
				    c->fm_flag_eps));
	if (timing)
		HIPCHK(hipEventRecord(ev[kEvFmdevDone], fs));
	HIPCHK(hipEventRecord(P.ev_front, fs));
	if (c->levels) {  // the level meter: behind the front end (the mask is final), beside the chains, on its own low-priority stream
		HIPCHK(hipStreamWaitEvent(c->lv, P.ev_front, 0));
		HIPCHK(launch_levels(c->lv, c->d_dec[set], c->dec_stride, c->d_mask[set], c->mask_stride, c->cfg.n_streams, n_blocks,
				     c->d_lev, c->d_scfg, c->d_levels[set]));
		HIPCHK(hipEventRecord(c->ev_lev[set], c->lv));
		c->set_blocks[set] = n_blocks;
	}
	if (c->capture) {  // the recorder: placed like the level meter, on a low-priority stream of its own
		HIPCHK(hipStreamWaitEvent(c->cap, P.ev_front, 0));
		HIPCHK(launch_capture(c->cap, c->d_dec[set], c->dec_stride, c->d_mask[set], c->mask_stride, c->cfg.n_streams, n_blocks,
				      c->sample_base, c->d_capst, c->d_scfg, c->d_capstage, c->cap_stage_cap, c->d_capcnt, c->d_capbase,
				      c->d_caphdr[set], c->d_runs[set], c->cap_max_runs, c->d_pool[set], c->cap_max_samples));
		HIPCHK(hipEventRecord(c->ev_cap[set], c->cap));
	}
	if (c->cfg.flags & TFREC_AMD_F_SERIAL_CHAINS) {
		HIPCHK(hipStreamWaitEvent(P.cs, P.ev_front, 0));
		HIPCHK(launch_chains(P.cs, c->d_dec[set], c->dec_stride, c->d_mask[set], c->mask_stride, c->cfg.n_streams, n_blocks,
				     c->sample_base, c->launch, c->d_events[set], c->d_eb[set], c->cfg.flags));
		if (timing)
			HIPCHK(hipEventRecord(ev[kEvSerialDone], P.cs));
		for (hipEvent_t e : P.done)
			HIPCHK(hipEventRecord(e, P.cs));
	} else {
		c->win[set].whb_submit_seq = c->submit_seq++;
		HIPCHK(launch_pipeline(P, c->d_dec[set], c->dec_stride, c->d_mask[set], c->mask_stride, c->d_fmdev[set], c->dec_stride,
				       c->cfg.n_streams, n_blocks, c->sample_base, c->launch, c->win[set], c->d_ld16[set],
				       c->d_dev32[set], c->d_events[set], c->d_eb[set], c->cfg.flags));
	}
	report_debug_stats(c, set, n_blocks);
	// the drain's copies, queued now
	for (hipEvent_t e : P.done)
		HIPCHK(hipStreamWaitEvent(c->cpy, e, 0));
	if (c->levels)  // copied[set] then also says "the records are written" (tfrec_amd_read_levels, and the set's reuse)
		HIPCHK(hipStreamWaitEvent(c->cpy, c->ev_lev[set], 0));
	if (c->capture)  // ... and "the captures are written" (tfrec_amd_read_captures)
		HIPCHK(hipStreamWaitEvent(c->cpy, c->ev_cap[set], 0));
	if (c->spectrum)  // ... and "the spectrum's records are written" (tfrec_amd_read_spectrum; the staged input may be reused)
		HIPCHK(hipStreamWaitEvent(c->cpy, c->ev_spectrum[set], 0));
	c->copied_n[set] = std::min<uint32_t>(c->copy_guess, (uint32_t)c->cfg.max_events);
	{  // header, overflow flag and the first copied_n events in one go
		static_assert(kEvHeader % 16 == 0 && sizeof(tfrec_amd_event) % 16 == 0, "drain_copy_kernel moves 16 bytes per lane");
		const size_t bytes = kEvHeader + (size_t)c->copied_n[set] * sizeof(tfrec_amd_event);
		const size_t n16 = bytes / 16;
		const unsigned blocks = (unsigned)std::min<size_t>(256, (n16 + 255) / 256);
		hipLaunchKernelGGL(tfrec::drain_copy_kernel, dim3(blocks), dim3(256), 0, c->cpy, (const uint4 *)c->d_evblock[set],
				   (uint4 *)c->h_evblock_dev[set], n16);
		HIPCHK(hipGetLastError());
	}
	HIPCHK(hipEventRecord(c->copied[set], c->cpy));
	if (timing)
		c->timed = true;
	if (resets) {
		for (int32_t r : c->reset_pending) {
			c->origin[r] = c->sample_base;
			c->reset_marked[r] = 0;
		}
		c->reset_pending.clear();
	}
	// (until the first reset the origins are all zero: nothing is recorded, and the drain subtracts nothing)
	c->any_reset = c->any_reset || resets;
	if (c->any_reset)
		c->set_origin[set] = c->origin;
	c->submitted = true;
	c->inflight++;
	c->last_set = set;
	c->tail_sel ^= 1;
	c->sample_base += (long long)n_blocks * kBlockDec;
	c->last_blocks = n_blocks;
	guard.ok = true;
	return TFREC_AMD_OK;
}

int tfrec_amd_submit_device(tfrec_amd_ctx *c, const void *d_iq, size_t stride, int n_blocks, void *hip_stream)
{
	const auto t0 = std::chrono::steady_clock::now();
	const int rc = submit_common(c, d_iq, stride, n_blocks, hip_stream, false);
	if (c)
		c->hp_submit += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
	return rc;
}

static int submit_host_impl(tfrec_amd_ctx *c, const uint8_t *h_iq, size_t stride, int n_blocks);

int tfrec_amd_submit_host(tfrec_amd_ctx *c, const uint8_t *h_iq, size_t stride, int n_blocks)
{
	const auto t0 = std::chrono::steady_clock::now();
	const int rc = submit_host_impl(c, h_iq, stride, n_blocks);
	if (c)
		c->hp_submit += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
	return rc;
}

static int submit_host_impl(tfrec_amd_ctx *c, const uint8_t *h_iq, size_t stride, int n_blocks)
{
	if (!c || !h_iq || n_blocks < 1 || n_blocks > c->cfg.max_blocks)
		return TFREC_AMD_E_INVAL;
	size_t row = 0;
	TRY(input_bytes(c, n_blocks, &row));
	if (rows_in_use(c) > 1 && stride < row)
		return TFREC_AMD_E_INVAL;
	TRY(check_fifo(c));
	HIPCHK(hipSetDevice(c->cfg.device));
	const int set = (c->head + c->inflight) % kSets;  // the set's previous user has been drained: its staging buffer is free
	const size_t rows = (size_t)rows_in_use(c);  // (a mapped context: only the rows a stream reads are staged and copied)
	const size_t need = row * rows;
	if (c->stage_bytes[set] < need) {
		(void)hipFree(c->d_stage[set]);
		c->d_stage[set] = nullptr;
		c->stage_bytes[set] = 0;
		if (hipMalloc((void **)&c->d_stage[set], need) != hipSuccess)
			return TFREC_AMD_E_NOMEM;
		c->stage_bytes[set] = need;
	}
	// asynchronous on the front-end stream when h_iq is pinned (tfrec_amd_host_alloc); pageable memory is staged
	// by the runtime before the call returns
	HIPCHK(hipMemcpy2DAsync(c->d_stage[set], row, h_iq, stride, row, rows, hipMemcpyHostToDevice, c->pipe[set].fs));
	return submit_common(c, c->d_stage[set], row, n_blocks, nullptr, true);
}

int tfrec_amd_input_bytes(tfrec_amd_ctx *c, int n_blocks, size_t *bytes_per_stream)
{
	if (!c || !bytes_per_stream)
		return TFREC_AMD_E_INVAL;
	return input_bytes(c, n_blocks, bytes_per_stream);
}

void *tfrec_amd_host_alloc(size_t bytes)
{
	void *p = nullptr;
	if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess)
		return nullptr;
	return p;
}

void tfrec_amd_host_free(void *p)
{
	if (p)
		(void)hipHostFree(p);
}

int tfrec_amd_sync(tfrec_amd_ctx *c)
{
	if (!c)
		return TFREC_AMD_E_INVAL;
	HIPCHK(hipSetDevice(c->cfg.device));
	for (const tfrec_amd_ctx::Owned &o : c->owned)
		if (o.kind == tfrec_amd_ctx::Owned::kStream)
			HIPCHK(hipStreamSynchronize(static_cast<hipStream_t>(o.h)));
	return TFREC_AMD_OK;
}

int tfrec_amd_pending_events(tfrec_amd_ctx *c, int *n)
{
	if (!c || !n)
		return TFREC_AMD_E_INVAL;
	*n = 0;
	TRY(check_live(c));  // (copied[head] may never have been recorded: synchronising on it would succeed at once)
	if (c->inflight == 0)
		return TFREC_AMD_OK;
	HIPCHK(hipSetDevice(c->cfg.device));
	HIPCHK(hipEventSynchronize(c->copied[c->head]));  // the oldest submit not yet drained
	const EventBuf eb = *c->h_eb[c->head];
	*n = (int)(std::min(eb.count, eb.capacity) - std::min(eb.dead, std::min(eb.count, eb.capacity)));  // (retracted events are not reported)
	return eb.count > eb.capacity ? TFREC_AMD_E_OVERFLOW : TFREC_AMD_OK;
}

int tfrec_amd_read_levels(tfrec_amd_ctx *c, tfrec_amd_level *out, size_t cap, int *n_blocks_out)
{
	if (!c || !out || !n_blocks_out)
		return TFREC_AMD_E_INVAL;
	if (!c->levels) {
		snprintf(g_err, sizeof(g_err), "the context was made without the level meter's flag");
		return TFREC_AMD_E_INVAL;
	}
	TRY(check_live(c));
	if (c->inflight == 0) {
		snprintf(g_err, sizeof(g_err), "no undrained submit: the levels are read before tfrec_amd_drain_events");
		return TFREC_AMD_E_STATE;
	}
	const int set = c->head;
	const size_t n = (size_t)c->cfg.n_streams * (size_t)c->set_blocks[set];
	if (cap < n) {
		snprintf(g_err, sizeof(g_err), "room for %zu level records, the submit has %zu", cap, n);
		return TFREC_AMD_E_INVAL;
	}
	HIPCHK(hipSetDevice(c->cfg.device));
	HIPCHK(hipEventSynchronize(c->copied[set]));  // (behind ev_lev[set])
	HIPCHK(hipMemcpy(out, c->d_levels[set], n * sizeof(tfrec_amd_level), hipMemcpyDeviceToHost));
	*n_blocks_out = c->set_blocks[set];
	return TFREC_AMD_OK;
}

int tfrec_amd_enable_capture(tfrec_amd_ctx *c, uint32_t max_runs, uint64_t max_samples)
{
	if (!c)
		return TFREC_AMD_E_INVAL;
	if (max_runs == 0 || max_samples == 0 || c->capture) {
		snprintf(g_err, sizeof(g_err), c->capture ? "the recorder is enabled already" : "max_runs and max_samples must not be 0");
		return TFREC_AMD_E_INVAL;
	}
	TRY(check_live(c));
	if (c->submitted) {
		snprintf(g_err, sizeof(g_err), "the recorder is enabled before the first submit");
		return TFREC_AMD_E_STATE;
	}
	if (max_samples > (uint64_t)SIZE_MAX / sizeof(uint32_t)) {
		snprintf(g_err, sizeof(g_err), "max_samples too large");
		return TFREC_AMD_E_NOMEM;
	}
	HIPCHK(hipSetDevice(c->cfg.device));
	const size_t n = (size_t)c->cfg.n_streams;
	// a stream's runs in one submit: all but the first and the last are at least 356 samples long, with a gap between them
	c->cap_stage_cap = (int)((size_t)c->cfg.max_blocks * kBlockDec / 356 + 3);
	TRY(own_device(c, c->d_capst, n * sizeof(CaptureState)));
	TRY(own_device(c, c->d_capstage, n * (size_t)c->cap_stage_cap * sizeof(CaptureStage)));
	TRY(own_device(c, c->d_capcnt, n * sizeof(uint2)));
	TRY(own_device(c, c->d_capbase, n * sizeof(uint4)));
	std::vector<CaptureState> st(n);
	for (size_t s = 0; s < n; s++)  // every stream starts like its FskState (a configure ahead of the first submit is a restart)
		st[s] = CaptureState{ c->scfg[s].thresh, 0, 0, -(1 << 28) };
	HIPCHK(hipMemcpy(c->d_capst, st.data(), n * sizeof(CaptureState), hipMemcpyHostToDevice));
	for (int k = 0; k < kSets; k++) {
		TRY(own_device(c, c->d_runs[k], (size_t)max_runs * sizeof(tfrec_amd_run)));
		TRY(own_device(c, c->d_pool[k], (size_t)max_samples * sizeof(uint32_t)));
		TRY(own_device(c, c->d_caphdr[k], sizeof(CaptureHeader)));
		TRY(own_event(c, c->ev_cap[k], hipEventDisableTiming));
	}
	int prio_lo = 0, prio_hi = 0;
	(void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
	TRY(own_stream(c, c->cap, prio_lo));
	c->cap_max_runs = max_runs;
	c->cap_max_samples = max_samples;
	c->capture = true;  // (only now: a context whose allocation failed half way runs on without the recorder)
	return TFREC_AMD_OK;
}

int tfrec_amd_read_captures(tfrec_amd_ctx *c, tfrec_amd_run *runs, size_t cap_runs, uint32_t *n_runs, int16_t *samples, size_t cap_pairs,
			    uint64_t *n_pairs)
{
	if (!c || !n_runs || !n_pairs || (cap_runs > 0 && !runs) || (cap_pairs > 0 && !samples))
		return TFREC_AMD_E_INVAL;
	if (!c->capture) {
		snprintf(g_err, sizeof(g_err), "tfrec_amd_enable_capture was not called on this context");
		return TFREC_AMD_E_INVAL;
	}
	TRY(check_live(c));
	if (c->inflight == 0) {
		snprintf(g_err, sizeof(g_err), "no undrained submit: the captures are read before tfrec_amd_drain_events");
		return TFREC_AMD_E_STATE;
	}
	const int set = c->head;
	HIPCHK(hipSetDevice(c->cfg.device));
	HIPCHK(hipEventSynchronize(c->copied[set]));  // (behind ev_cap[set])
	CaptureHeader hdr;
	HIPCHK(hipMemcpy(&hdr, c->d_caphdr[set], sizeof(hdr), hipMemcpyDeviceToHost));
	const bool overflow = hdr.n_runs > c->cap_max_runs || hdr.n_pairs > c->cap_max_samples;
	// the table as far as the device wrote it, then the prefix of whole runs whose pairs it wrote too
	size_t have = (size_t)std::min<unsigned long long>(hdr.n_runs, c->cap_max_runs);
	std::vector<tfrec_amd_run> &tmp = c->cap_tmp;
	tmp.resize(have);
	if (have)
		HIPCHK(hipMemcpy(tmp.data(), c->d_runs[set], have * sizeof(tfrec_amd_run), hipMemcpyDeviceToHost));
	uint64_t pairs = hdr.n_pairs;
	if (overflow) {
		size_t k = 0;
		pairs = 0;
		while (k < have && tmp[k].pool_offset + tmp[k].n_samples <= c->cap_max_samples) {
			pairs = tmp[k].pool_offset + tmp[k].n_samples;
			k++;
		}
		have = k;
	}
	*n_runs = (uint32_t)std::min<unsigned long long>(hdr.n_runs, 0xffffffffull);
	*n_pairs = hdr.n_pairs;
	if (cap_runs < have || (samples && cap_pairs < pairs)) {
		snprintf(g_err, sizeof(g_err), "room for %zu runs and %zu pairs, the submit delivers %zu and %llu", cap_runs, cap_pairs, have,
			 (unsigned long long)pairs);
		return TFREC_AMD_E_INVAL;
	}
	if (!c->set_origin[set].empty()) {  // start_sample counts from the stream's last restart, as end_sample does
		const std::vector<long long> &org = c->set_origin[set];
		for (size_t i = 0; i < have; i++)
			if (tmp[i].stream < org.size())
				tmp[i].start_sample -= org[tmp[i].stream];
	}
	if (samples && pairs)
		HIPCHK(hipMemcpy(samples, c->d_pool[set], (size_t)pairs * sizeof(uint32_t), hipMemcpyDeviceToHost));
	if (have)
		memcpy(runs, tmp.data(), have * sizeof(tfrec_amd_run));
	if (overflow && cap_runs > have)
		memset(&runs[have], 0, sizeof(tfrec_amd_run));
	return overflow ? TFREC_AMD_E_OVERFLOW : TFREC_AMD_OK;
}

// Give back what own_* recorded behind `mark` (an enable call that ran out of memory half way: the context goes on without it)
static void release_from(tfrec_amd_ctx *c, size_t mark, size_t dev_bytes)
{
	while (c->owned.size() > mark) {
		const tfrec_amd_ctx::Owned o = c->owned.back();
		c->owned.pop_back();
		switch (o.kind) {
		case tfrec_amd_ctx::Owned::kDevice: (void)hipFree(o.h); break;
		case tfrec_amd_ctx::Owned::kPinned: (void)hipHostFree(o.h); break;
		case tfrec_amd_ctx::Owned::kStream: (void)hipStreamDestroy(static_cast<hipStream_t>(o.h)); break;
		case tfrec_amd_ctx::Owned::kEvent: (void)hipEventDestroy(static_cast<hipEvent_t>(o.h)); break;
		}
	}
	c->dev_bytes = dev_bytes;
}

static int make_spectrum(tfrec_amd_ctx *c, size_t rows, size_t records, size_t n)
{
	for (int k = 0; k < kSets; k++) {
		TRY(own_device(c, c->d_spec_sum[k], rows * records * n * sizeof(unsigned long long)));
		TRY(own_device(c, c->d_spec_peak[k], rows * records * n * sizeof(unsigned long long)));
		TRY(own_device(c, c->d_spec_nf[k], rows * records * sizeof(uint32_t)));
		TRY(own_event(c, c->ev_spectrum[k], hipEventDisableTiming));
	}
	int prio_lo = 0, prio_hi = 0;
	(void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
	TRY(own_stream(c, c->sp, prio_lo));
	return TFREC_AMD_OK;
}

int tfrec_amd_enable_spectrum(tfrec_amd_ctx *c, int32_t n_bins, int32_t frames_per_record, int32_t max_rows)
{
	if (!c)
		return TFREC_AMD_E_INVAL;
	const bool bins_ok = n_bins == 64 || n_bins == 128 || n_bins == 256 || n_bins == 512 || n_bins == 1024;
	if (!bins_ok || frames_per_record < 1 || frames_per_record > 16384 || max_rows < 1 || max_rows > c->cfg.n_streams || c->spectrum) {
		snprintf(g_err, sizeof(g_err), c->spectrum ? "the spectrum is enabled already"
				: "n_bins is 64, 128, 256, 512 or 1024, frames_per_record within [1, 16384], max_rows within [1, n_streams]");
		return TFREC_AMD_E_INVAL;
	}
	TRY(check_live(c));
	if (c->submitted) {
		snprintf(g_err, sizeof(g_err), "the spectrum is enabled before the first submit");
		return TFREC_AMD_E_STATE;
	}
	HIPCHK(hipSetDevice(c->cfg.device));
	// the largest submit: floor(max_blocks * 32768 * P / Q) complex samples per row
	const long long p = c->in10x ? 10 : c->rate_p, q = c->in10x ? 1 : c->rate_q;
	const long long n_in = (long long)c->cfg.max_blocks * (TFREC_AMD_BLOCK_BYTES / 2) * p / q;
	const long long frames = n_in / n_bins;
	const size_t records = (size_t)((frames + frames_per_record - 1) / frames_per_record);
	const size_t mark = c->owned.size(), bytes = c->dev_bytes;
	const int rc = make_spectrum(c, (size_t)max_rows, records, (size_t)n_bins);
	if (rc != TFREC_AMD_OK) {
		release_from(c, mark, bytes);
		for (int k = 0; k < kSets; k++) {
			c->d_spec_sum[k] = c->d_spec_peak[k] = nullptr;
			c->d_spec_nf[k] = nullptr;
			c->ev_spectrum[k] = nullptr;
		}
		c->sp = nullptr;
		return rc;
	}
	c->spec_n = n_bins;
	c->spec_g = frames_per_record;
	c->spec_rows = max_rows;
	c->spec_max_records = records;
	c->spectrum = true;
	return TFREC_AMD_OK;
}

int tfrec_amd_read_spectrum(tfrec_amd_ctx *c, int32_t row, uint64_t *sum, uint64_t *peak, size_t cap_records, uint32_t *n_frames,
			    int *n_records)
{
	if (!c || !n_records)
		return TFREC_AMD_E_INVAL;
	if (!c->spectrum) {
		snprintf(g_err, sizeof(g_err), "tfrec_amd_enable_spectrum was not called on this context");
		return TFREC_AMD_E_INVAL;
	}
	TRY(check_live(c));
	if (c->inflight == 0) {
		snprintf(g_err, sizeof(g_err), "no undrained submit: the spectrum is read before tfrec_amd_drain_events");
		return TFREC_AMD_E_STATE;
	}
	const int set = c->head;
	if (row < 0 || row >= c->spec_set_rows[set]) {
		snprintf(g_err, sizeof(g_err), "row %d: the submit's spectrum covers rows [0, %d)", (int)row, c->spec_set_rows[set]);
		return TFREC_AMD_E_INVAL;
	}
	const size_t nr = (size_t)c->spec_set_records[set], n = (size_t)c->spec_n;
	*n_records = (int)nr;
	if (cap_records < nr || (nr > 0 && (!sum || !peak || !n_frames))) {
		snprintf(g_err, sizeof(g_err), "room for %zu spectrum records, the submit has %zu", cap_records, nr);
		return TFREC_AMD_E_INVAL;
	}
	if (nr == 0)
		return TFREC_AMD_OK;
	HIPCHK(hipSetDevice(c->cfg.device));
	HIPCHK(hipEventSynchronize(c->copied[set]));  // (behind ev_spectrum[set])
	const size_t r0 = (size_t)row * c->spec_max_records;
	HIPCHK(hipMemcpy(sum, c->d_spec_sum[set] + r0 * n, nr * n * sizeof(uint64_t), hipMemcpyDeviceToHost));
	HIPCHK(hipMemcpy(peak, c->d_spec_peak[set] + r0 * n, nr * n * sizeof(uint64_t), hipMemcpyDeviceToHost));
	HIPCHK(hipMemcpy(n_frames, c->d_spec_nf[set] + r0, nr * sizeof(uint32_t), hipMemcpyDeviceToHost));
	return TFREC_AMD_OK;
}

int tfrec_amd_drain_events(tfrec_amd_ctx *c, tfrec_amd_event *out, int cap, int *n_out)
{
	if (!c || !n_out || cap < 0 || (cap > 0 && !out))
		return TFREC_AMD_E_INVAL;
	*n_out = 0;
	TRY(check_live(c));
	if (c->inflight == 0)
		return TFREC_AMD_OK;
	HIPCHK(hipSetDevice(c->cfg.device));
	const int set = c->head;  // the oldest submit not yet drained; a younger one may still be running
	const auto hp0 = std::chrono::steady_clock::now();
	HIPCHK(hipEventSynchronize(c->copied[set]));  // the chains' ends and the copies queued by the submit
	const auto hp1 = std::chrono::steady_clock::now();
	const EventBuf eb = *c->h_eb[set];
	const uint32_t have = std::min(eb.count, eb.capacity);
	bool overflow = eb.count > eb.capacity;
	tfrec_amd_event *tmp = c->h_events[set];
	if (have > c->copied_n[set])  // more events than the submit guessed (not on cp: the copies of younger submits wait there)
		HIPCHK(hipMemcpy(tmp + c->copied_n[set], c->d_events[set] + c->copied_n[set],
				 (size_t)(have - c->copied_n[set]) * sizeof(tfrec_amd_event), hipMemcpyDeviceToHost));
	c->copy_guess = std::max<uint32_t>(c->copy_guess_min, 2 * have);
	uint32_t live = have;
	if (eb.dead) {  // a WHB stream's speculative events that the exact kernel replaced (rare): never reported
		live = 0;
		for (uint32_t i = 0; i < have; i++)
			if (tmp[i].status != kStatusDead)
				tmp[live++] = tmp[i];
	}
	if (!c->set_origin[set].empty()) {  // end_sample counts from the stream's last reset: flushes and BITS chunks (window opens) alike
		const std::vector<long long> &org = c->set_origin[set];
		for (uint32_t i = 0; i < live; i++)
			if (tmp[i].stream < org.size())
				tmp[i].end_sample -= org[tmp[i].stream];
	}
	c->head = (c->head + 1) % kSets;
	c->inflight--;
	c->last_drained = set;
	account_fm_log(&c->fm, eb);
	{
		int32_t wov = 0;
		memcpy(&wov, c->h_evblock[set] + kEvOverflowOff, 4);
		if (wov) {  // cannot happen (cap is the worst case); reported rather than ignored
			snprintf(g_err, sizeof(g_err), "window table overflow");
			return TFREC_AMD_E_STATE;
		}
	}
	const auto hp2 = std::chrono::steady_clock::now();
	// Order: (stream, slot, seq, BITS chunks before their flush, end_sample, offset).  The events of a stream are few:
	// bucket by stream (counting sort on indices), then order each bucket.
	auto before = [](const tfrec_amd_event &a, const tfrec_amd_event &b) {
		if (a.slot != b.slot)
			return a.slot < b.slot;
		if (a.seq != b.seq)
			return a.seq < b.seq;
		// TFREC_AMD_F_BITS: the bit chunks of a flush come before it, in the order the bits were produced
		const bool ab = a.status == TFREC_AMD_STATUS_BITS, bb = b.status == TFREC_AMD_STATUS_BITS;
		if (ab != bb)
			return ab;
		if (a.end_sample != b.end_sample)
			return a.end_sample < b.end_sample;
		return a.offset < b.offset;
	};
	const uint32_t ns = (uint32_t)c->cfg.n_streams;
	std::vector<uint32_t> &idx = c->sort_idx, &start = c->sort_start;
	idx.resize(live);
	start.assign(ns + 1, 0u);
	for (uint32_t i = 0; i < live; i++)
		start[std::min(tmp[i].stream, ns - 1) + 1]++;
	for (uint32_t s = 0; s < ns; s++)
		start[s + 1] += start[s];
	{
		std::vector<uint32_t> fill(start.begin(), start.end() - 1);
		for (uint32_t i = 0; i < live; i++)
			idx[fill[std::min(tmp[i].stream, ns - 1)]++] = i;
	}
	for (uint32_t s = 0; s < ns; s++)
		std::sort(idx.begin() + start[s], idx.begin() + start[s + 1],
			  [&](uint32_t x, uint32_t y) { return before(tmp[x], tmp[y]); });
	uint32_t ncopy = live;
	if (ncopy > (uint32_t)cap) {
		ncopy = (uint32_t)cap;
		overflow = true;
	}
	for (uint32_t i = 0; i < ncopy; i++)
		out[i] = tmp[idx[i]];
	*n_out = (int)ncopy;
	const auto hp3 = std::chrono::steady_clock::now();
	c->hp_wait += std::chrono::duration<double>(hp1 - hp0).count();
	c->hp_copy += std::chrono::duration<double>(hp2 - hp1).count();
	c->hp_sort += std::chrono::duration<double>(hp3 - hp2).count();
	c->hp_n++;
	return overflow ? TFREC_AMD_E_OVERFLOW : TFREC_AMD_OK;
}

int tfrec_amd_reset_streams(tfrec_amd_ctx *c, const int32_t *streams, int n)
{
	if (!c || n < 0 || (n > 0 && !streams))
		return TFREC_AMD_E_INVAL;
	for (int i = 0; i < n; i++)
		TRY(check_stream(c, streams[i]));
	TRY(check_live(c));
	for (int i = 0; i < n; i++)
		if (!c->reset_marked[streams[i]]) {
			c->reset_marked[streams[i]] = 1;
			c->reset_pending.push_back(streams[i]);
		}
	return TFREC_AMD_OK;
}

// a configure or a tune: from the next submit on the kernels read every stream's own settings
static void use_per_stream(tfrec_amd_ctx *c)
{
	if (c->per_stream)
		return;
	c->per_stream = true;
	c->launch.scfg = c->d_scfg;
	c->taps.scfg = c->d_scfg;
	for (int k = 0; k < 20; k++)  // f2: the narrow taps from now on (w: the wide ones)
		c->taps.f2[k][0] = c->taps.f2[k][1] = (float)kNarrowTaps[k] / 65536.0f;
}

// mark stream s to restart at the next submit (once per submit)
static void mark_restart(tfrec_amd_ctx *c, int32_t s)
{
	if (!c->reset_marked[s]) {
		c->reset_marked[s] = 1;
		c->reset_pending.push_back(s);
	}
}

int tfrec_amd_configure_streams(tfrec_amd_ctx *c, const int32_t *streams, const tfrec_amd_stream_config *cfgs, int n)
{
	if (!c || n < 0 || (n > 0 && (!streams || !cfgs)))
		return TFREC_AMD_E_INVAL;
	for (int i = 0; i < n; i++) {
		const tfrec_amd_stream_config &sc = cfgs[i];
		TRY(check_stream(c, streams[i]));
		if (sc.types_mask == 0 || (sc.types_mask & ~c->cfg.types_mask) != 0 || sc.thresh < 0 || sc.filter_type < 0 ||
		    sc.filter_type > 1 || sc.reserved != 0) {
			snprintf(g_err, sizeof(g_err), "bad stream config (types_mask 0x%x of the context's 0x%x, thresh %d, filter_type %d, "
				 "reserved %d)", (unsigned)sc.types_mask, (unsigned)c->cfg.types_mask, (int)sc.thresh, (int)sc.filter_type,
				 (int)sc.reserved);
			return TFREC_AMD_E_INVAL;
		}
	}
	TRY(check_live(c));
	if (n == 0)
		return TFREC_AMD_OK;
	// a configure is a reset with new settings: the stream restarts at the next submit (before the first one that restores
	// nothing but the settings)
	for (int i = 0; i < n; i++) {
		const int s = streams[i];
		c->scfg_api[s] = cfgs[i];
		c->scfg[s] = device_cfg(c, cfgs[i]);
		mark_restart(c, s);
	}
	c->n_auto = 0;
	for (const StreamCfg &d : c->scfg)
		c->n_auto += d.autoth;
	use_per_stream(c);
	return TFREC_AMD_OK;
}

int tfrec_amd_get_stream_config(tfrec_amd_ctx *c, int stream, tfrec_amd_stream_config *out)
{
	if (!c || !out || stream < 0 || stream >= c->cfg.n_streams)
		return TFREC_AMD_E_INVAL;
	*out = c->scfg_api[stream];
	return TFREC_AMD_OK;
}

// The phase step per sample, in 2^-32 turns, of a tune of tune_hz at 1536000 P / Q samples per second:
//   inc = floor((tune_hz * 2^33 * Q + 1536000 P) / (2 * 1536000 P)) mod 2^32
// (DESIGN.md 6d at 1/1, 6e at 10/1, 6g at the input rate).  |tune_hz| < 7680000 and Q <= 64: the numerator stays below 2^63.
static uint32_t phase_inc(int32_t tune_hz, long long p, long long q)
{
	const long long num = (long long)tune_hz * (1LL << 33) * q + 1536000LL * p, den = 2 * 1536000LL * p;
	long long v = num / den;
	if (num % den != 0 && num < 0)
		v--;  // (floor, not C's truncation)
	return (uint32_t)(uint64_t)v;
}

// What the three tunes share, behind their own preconditions: every stream and tune checked (out_of_range(tune_hz) writes the
// message) before anything changes; then hz / inc of the listed streams, their restart -- a tune is a reset with a new tune,
// exactly as a configure is one with new settings -- and the count of tuned streams.
static int tune_common(tfrec_amd_ctx *c, const int32_t *streams, const int32_t *tune_hz, int n, long long p, long long q,
		       const std::function<bool(int32_t)> &out_of_range, std::vector<int32_t> &hz, std::vector<uint32_t> &inc, int &n_tuned)
{
	for (int i = 0; i < n; i++) {
		TRY(check_stream(c, streams[i]));
		if (out_of_range(tune_hz[i]))
			return TFREC_AMD_E_INVAL;
	}
	TRY(check_live(c));
	for (int i = 0; i < n; i++) {
		const int s = streams[i];
		hz[s] = tune_hz[i];
		inc[s] = phase_inc(tune_hz[i], p, q);
		mark_restart(c, s);
	}
	n_tuned = 0;
	for (const uint32_t v : inc)
		n_tuned += v != 0;
	return TFREC_AMD_OK;
}

// |tune_hz| < limit, the message of the base and the wide tune
static bool outside_limit(int32_t tune_hz, int limit)
{
	if (tune_hz > -limit && tune_hz < limit)
		return false;
	snprintf(g_err, sizeof(g_err), "tune_hz %d outside (-%d, %d)", (int)tune_hz, limit, limit);
	return true;
}

int tfrec_amd_tune_streams(tfrec_amd_ctx *c, const int32_t *streams, const int32_t *tune_hz, int n)
{
	if (!c || n < 0 || (n > 0 && (!streams || !tune_hz)))
		return TFREC_AMD_E_INVAL;
	TRY(tune_common(c, streams, tune_hz, n, 1, 1, [](int32_t hz) { return outside_limit(hz, kTuneLimit); }, c->tune_hz, c->tune_inc,
			c->n_tuned));
	if (n > 0)
		use_per_stream(c);
	return TFREC_AMD_OK;
}

int tfrec_amd_get_stream_tune(tfrec_amd_ctx *c, int stream, int32_t *tune_hz)
{
	if (!c || !tune_hz || stream < 0 || stream >= c->cfg.n_streams)
		return TFREC_AMD_E_INVAL;
	*tune_hz = c->tune_hz[stream];
	return TFREC_AMD_OK;
}

// a map is a restart that changes the row the stream's tiles are loaded from -- also when it names the row the stream reads already
int tfrec_amd_map_streams(tfrec_amd_ctx *c, const int32_t *streams, const int32_t *inputs, int n)
{
	if (!c || n < 0 || (n > 0 && (!streams || !inputs)))
		return TFREC_AMD_E_INVAL;
	for (int i = 0; i < n; i++) {
		TRY(check_stream(c, streams[i]));
		if (inputs[i] < 0 || inputs[i] >= c->cfg.n_streams) {
			snprintf(g_err, sizeof(g_err), "input row %d outside [0, %d)", (int)inputs[i], c->cfg.n_streams);
			return TFREC_AMD_E_INVAL;
		}
	}
	TRY(check_live(c));
	if (n == 0)
		return TFREC_AMD_OK;
	for (int i = 0; i < n; i++) {
		c->row[streams[i]] = inputs[i];
		mark_restart(c, streams[i]);
	}
	c->mapped = true;
	if (!c->in16)  // (the mapped front end is a per-stream variant; with the 10x input or a rate the pre-stage maps)
		use_per_stream(c);
	return TFREC_AMD_OK;
}

int tfrec_amd_get_stream_input(tfrec_amd_ctx *c, int stream, int32_t *input)
{
	if (!c || !input || stream < 0 || stream >= c->cfg.n_streams)
		return TFREC_AMD_E_INVAL;
	*input = c->row[stream];
	return TFREC_AMD_OK;
}

int tfrec_amd_tune_streams_wide(tfrec_amd_ctx *c, const int32_t *streams, const int32_t *tune_hz, int n)
{
	if (!c || n < 0 || (n > 0 && (!streams || !tune_hz)))
		return TFREC_AMD_E_INVAL;
	if (!c->in10x) {
		snprintf(g_err, sizeof(g_err), "the wide tune acts ahead of the 10:1 stage: the context needs the 15.36 MS/s input flag%s",
			 c->resamp ? " (the tune ahead of the resampling stage is tfrec_amd_tune_streams_input)" : "");
		return TFREC_AMD_E_INVAL;
	}
	return tune_common(c, streams, tune_hz, n, 10, 1, [](int32_t hz) { return outside_limit(hz, kTuneWideLimit); }, c->wide_hz,
			   c->wide_inc, c->n_wide);
}

int tfrec_amd_get_stream_tune_wide(tfrec_amd_ctx *c, int stream, int32_t *tune_hz)
{
	if (!c || !tune_hz || stream < 0 || stream >= c->cfg.n_streams)
		return TFREC_AMD_E_INVAL;
	*tune_hz = c->wide_hz[stream];
	return TFREC_AMD_OK;
}

// The tune at the input rate, ahead of the resampling stage (6g); a 10x context's wide tune under another name
int tfrec_amd_tune_streams_input(tfrec_amd_ctx *c, const int32_t *streams, const int32_t *tune_hz, int n)
{
	if (!c || n < 0 || (n > 0 && (!streams || !tune_hz)))
		return TFREC_AMD_E_INVAL;
	if (c->in10x)
		return tfrec_amd_tune_streams_wide(c, streams, tune_hz, n);
	if (!c->resamp) {
		snprintf(g_err, sizeof(g_err), "the input-rate tune acts ahead of a resampling or 10:1 stage, and this context has none: "
					       "tfrec_amd_tune_streams tunes its 1.536 MS/s input");
		return TFREC_AMD_E_INVAL;
	}
	const long long p = c->rate_p, q = c->rate_q;
	if (((c->rate_abs * 11585) >> 16) >= 32768) {  // (no accepted rate comes near: 19111 at most)
		snprintf(g_err, sizeof(g_err), "input rate %lld/%lld: the int16 store of a tuned stream could wrap", p, q);
		return TFREC_AMD_E_INVAL;
	}
	const auto outside = [p, q](int32_t hz) {  // |tune_hz| < fs_in / 2, in integers
		if (2 * llabs((long long)hz) * q < 1536000LL * p)
			return false;
		snprintf(g_err, sizeof(g_err), "tune_hz %d outside half the input rate 1536000 * %lld / %lld (|tune_hz| < %lld)", (int)hz, p, q,
			 (1536000LL * p + 2 * q - 1) / (2 * q));
		return true;
	};
	return tune_common(c, streams, tune_hz, n, p, q, outside, c->wide_hz, c->wide_inc, c->n_wide);
}

int tfrec_amd_get_stream_tune_input(tfrec_amd_ctx *c, int stream, int32_t *tune_hz)
{
	return tfrec_amd_get_stream_tune_wide(c, stream, tune_hz);
}

int tfrec_amd_read_stage0(tfrec_amd_ctx *c, int stream, int16_t *out, size_t n_pairs)
{
	if (!c || !out || !c->in16 || stream < 0 || stream >= c->cfg.n_streams ||
	    n_pairs > (size_t)c->last_blocks * 4 * kBlockDec)
		return TFREC_AMD_E_INVAL;
	int rc = tfrec_amd_sync(c);
	if (rc)
		return rc;
	HIPCHK(hipMemcpy(out, c->d_in16[c->last_set] + (size_t)stream * c->in16_stride, n_pairs * sizeof(uint32_t),
			 hipMemcpyDeviceToHost));
	return TFREC_AMD_OK;
}

int tfrec_amd_read_decimated(tfrec_amd_ctx *c, int stream, int16_t *out, size_t n_pairs)
{
	if (!c || !out || stream < 0 || stream >= c->cfg.n_streams || n_pairs > (size_t)c->last_blocks * kBlockDec)
		return TFREC_AMD_E_INVAL;
	int rc = tfrec_amd_sync(c);
	if (rc)
		return rc;
	HIPCHK(hipMemcpy(out, c->d_dec[c->last_set] + (size_t)stream * c->dec_stride, n_pairs * sizeof(uint32_t),
			 hipMemcpyDeviceToHost));
	return TFREC_AMD_OK;
}

int tfrec_amd_atan_uncertain(tfrec_amd_ctx *c, uint64_t *n)
{
	if (!c || !n)
		return TFREC_AMD_E_INVAL;
	if (c->poisoned)
		return TFREC_AMD_E_STATE;
	int rc = tfrec_amd_sync(c);
	if (rc)
		return rc;
	*n = c->fm.resolved;
	for (int k = 0; k < c->inflight; k++) {  // submits not drained yet
		EventBuf eb;
		HIPCHK(hipMemcpy(&eb, c->d_eb[(c->head + k) % kSets], sizeof(eb), hipMemcpyDeviceToHost));
		*n += eb.uncertain;
	}
	return TFREC_AMD_OK;
}

int tfrec_amd_get_fm_stats(tfrec_amd_ctx *c, tfrec_amd_fm_stats *out)
{
	if (!c || !out)
		return TFREC_AMD_E_INVAL;
	if (c->poisoned)
		return TFREC_AMD_E_STATE;
	memset(out, 0, sizeof(*out));
	out->resolved = c->fm.resolved;
	out->host_verified = c->fm.verified;
	out->host_mismatch = c->fm.mismatch;
	out->undecidable = c->fm.undecidable;
	return TFREC_AMD_OK;
}

int tfrec_amd_fm_dev_probe(int device, int kind, const void *quads_v, size_t n, int32_t *out, tfrec_amd_fm_stats *stats)
{
	const int32_t *quads = (const int32_t *)quads_v;
	if (!quads || !out || n == 0 || n > (1u << 26) || kind < 0 || kind > 2)
		return TFREC_AMD_E_INVAL;
	HIPCHK(hipSetDevice(device));
	int32_t *d_q = nullptr, *d_o = nullptr;
	EventBuf *d_eb = nullptr;
	int rc = TFREC_AMD_OK;
	FmTotals tmp;
	if (hipMalloc((void **)&d_q, n * 16) != hipSuccess || hipMalloc((void **)&d_o, n * 4) != hipSuccess ||
	    hipMalloc((void **)&d_eb, sizeof(EventBuf)) != hipSuccess)
		rc = TFREC_AMD_E_NOMEM;
	// In pieces, so that the log (the first kFmLogCap slow-path decisions of a launch) does not saturate early; a caller
	// that wants EVERY sample checked compares `out` with its own reference.
	const size_t piece = 4096;
	if (rc == TFREC_AMD_OK && hipMemcpy(d_q, quads, n * 16, hipMemcpyHostToDevice) != hipSuccess)
		rc = TFREC_AMD_E_HIP;
	for (size_t o = 0; o < n && rc == TFREC_AMD_OK; o += piece) {
		const size_t m = std::min(piece, n - o);
		EventBuf eb;
		if (hipMemset(d_eb, 0, sizeof(EventBuf)) != hipSuccess || launch_fm_probe(nullptr, d_q + 4 * o, m, d_o + o, d_eb, kind) != hipSuccess ||
		    hipMemcpy(&eb, d_eb, sizeof(eb), hipMemcpyDeviceToHost) != hipSuccess)
			rc = hip_fail(hipGetLastError(), "fm_probe");
		else
			account_fm_log(&tmp, eb);
	}
	if (rc == TFREC_AMD_OK && hipMemcpy(out, d_o, n * 4, hipMemcpyDeviceToHost) != hipSuccess)
		rc = TFREC_AMD_E_HIP;
	(void)hipFree(d_q);
	(void)hipFree(d_o);
	(void)hipFree(d_eb);
	if (stats) {
		memset(stats, 0, sizeof(*stats));
		stats->resolved = tmp.resolved;
		stats->host_verified = tmp.verified;
		stats->host_mismatch = tmp.mismatch;
		stats->undecidable = tmp.undecidable;
	}
	return rc;
}

int tfrec_amd_iir_probe(int device, double cutoff, int form, const double *in, size_t n, double *out)
{
	if (!in || !out || n == 0 || n > (1u << 24) || form < 0 || form > 1 || !(cutoff > 0.0 && cutoff < 0.5))
		return TFREC_AMD_E_INVAL;
	HIPCHK(hipSetDevice(device));
	double *d_in = nullptr, *d_out = nullptr;
	int rc = TFREC_AMD_OK;
	if (hipMalloc((void **)&d_in, n * 8) != hipSuccess || hipMalloc((void **)&d_out, n * 8) != hipSuccess)
		rc = TFREC_AMD_E_NOMEM;
	if (rc == TFREC_AMD_OK && (hipMemcpy(d_in, in, n * 8, hipMemcpyHostToDevice) != hipSuccess ||
				   launch_iir_probe(nullptr, d_in, n, biquad_coef(cutoff), d_out, form) != hipSuccess ||
				   hipMemcpy(out, d_out, n * 8, hipMemcpyDeviceToHost) != hipSuccess))
		rc = hip_fail(hipGetLastError(), "iir_probe");
	(void)hipFree(d_in);
	(void)hipFree(d_out);
	return rc;
}

int tfrec_amd_read_thresh(tfrec_amd_ctx *c, int stream, int *thresh)
{
	if (!c || !thresh || stream < 0 || stream >= c->cfg.n_streams)
		return TFREC_AMD_E_INVAL;
	if (!c->per_stream && c->cfg.thresh) {  // (a configured stream's FskState holds its fixed threshold: stream_reset_kernel)
		*thresh = c->cfg.thresh;
		return TFREC_AMD_OK;
	}
	int rc = tfrec_amd_sync(c);
	if (rc)
		return rc;
	FskState f;
	HIPCHK(hipMemcpy(&f, c->d_fsk + stream, sizeof(f), hipMemcpyDeviceToHost));
	*thresh = f.thresh;
	return TFREC_AMD_OK;
}

int tfrec_amd_get_timings(tfrec_amd_ctx *c, tfrec_amd_timings *out)
{
	if (!c || !out)
		return TFREC_AMD_E_INVAL;
	if (!c->timed)
		return TFREC_AMD_E_STATE;
	// the most recently drained submit; before the first drain: the oldest one in flight
	const int set = c->last_drained >= 0 ? c->last_drained : c->head;
	hipEvent_t *ev = c->ev[set], *tev = c->tev[set];
	for (hipEvent_t e : c->pipe[set].done)
		HIPCHK(hipEventSynchronize(e));
	HIPCHK(hipEventElapsedTime(&out->frontend_ms, ev[kEvSubmit], ev[kEvFrontDone]));
	if (TFREC_KNOB_STR("HOST_PROF") && c->hp_n > 2) {  // idle time of the front-end stream between two submits' front ends
		float gap = 0, total = 0;
		const int next = (set + 1) % kSets;  // (in flight: its front end started long ago)
		if (hipEventElapsedTime(&gap, ev[kEvFrontDone], c->ev[next][kEvSubmit]) == hipSuccess &&
		    hipEventElapsedTime(&total, ev[kEvSubmit], tev[kMarkTfa1End]) == hipSuccess &&
		    gap > -1000 && gap < 1000) {
			float s2s = 0;
			if (hipEventElapsedTime(&s2s, ev[kEvSubmit], c->ev[next][kEvSubmit]) == hipSuccess)
				c->hp_s2s += s2s;
			c->hp_gap += gap;
			c->hp_lat += total;
			c->hp_gap_n++;
		}
		(void)hipGetLastError();
	}
	HIPCHK(hipEventElapsedTime(&out->fmdev_ms, ev[kEvFrontDone], ev[kEvFmdevDone]));
	if (c->fmdev_k2)  // (the discriminator pass ran in the pipeline)
		HIPCHK(hipEventElapsedTime(&out->fmdev_ms, tev[kMarkFmdev], tev[kMarkFmdevEnd]));
	out->windows_ms = out->spec_biquad_ms = out->repair_biquad_ms = out->fix_biquad_ms = out->slicer_ms = 0;
	out->coop_slicer_ms = out->decode_ms = out->commit_ms = 0;
	out->whb_biquad_ms = out->whb_demod_ms = out->whb_decode_ms = out->whb_commit_ms = 0;
	out->tfa1_slicer_ms = out->tfa1_coop_slicer_ms = out->tfa1_decode_commit_ms = 0;
	out->whb_verify_ms = 0;
	if (c->cfg.flags & TFREC_AMD_F_SERIAL_CHAINS) {
		HIPCHK(hipEventElapsedTime(&out->chains_ms, ev[kEvFmdevDone], ev[kEvSerialDone]));
		HIPCHK(hipEventElapsedTime(&out->total_ms, ev[kEvSubmit], ev[kEvSerialDone]));
		return TFREC_AMD_OK;
	}
	// the submit ends when the last of its three chains does
	out->chains_ms = out->total_ms = 0;
	const bool has_tfa2 = has_kind(c->launch, 1), has_whb = has_kind(c->launch, 2), has_tfa1 = has_kind(c->launch, 0);
	const struct {
		bool has;
		int end;
	} chain_end[3] = { { has_tfa2, kMarkTfa2End }, { has_whb, kMarkWhbCommitEnd }, { has_tfa1, kMarkTfa1End } };
	for (const auto &ce : chain_end)
		if (ce.has) {
			float t = 0;
			HIPCHK(hipEventElapsedTime(&t, ev[kEvFmdevDone], tev[ce.end]));
			out->chains_ms = std::max(out->chains_ms, t);
			HIPCHK(hipEventElapsedTime(&t, ev[kEvSubmit], tev[ce.end]));
			out->total_ms = std::max(out->total_ms, t);
		}
	HIPCHK(hipEventElapsedTime(&out->windows_ms, tev[kMarkWindows], tev[kMarkWindowsEnd]));
	if (has_tfa2) {
		HIPCHK(hipEventElapsedTime(&out->spec_biquad_ms, tev[kMarkTfa2Spec], tev[kMarkTfa2Repair]));
		HIPCHK(hipEventElapsedTime(&out->repair_biquad_ms, tev[kMarkTfa2Repair], tev[kMarkTfa2Fix]));
		HIPCHK(hipEventElapsedTime(&out->fix_biquad_ms, tev[kMarkTfa2Fix], tev[kMarkTfa2BiquadEnd]));
		HIPCHK(hipEventElapsedTime(&out->slicer_ms, tev[kMarkTfa2Slicer], tev[kMarkTfa2Coop]));
		HIPCHK(hipEventElapsedTime(&out->coop_slicer_ms, tev[kMarkTfa2Coop], tev[kMarkTfa2Decode]));
		HIPCHK(hipEventElapsedTime(&out->decode_ms, tev[kMarkTfa2Decode], tev[kMarkTfa2Commit]));
		HIPCHK(hipEventElapsedTime(&out->commit_ms, tev[kMarkTfa2Commit], tev[kMarkTfa2End]));
	}
	if (has_tfa1) {
		HIPCHK(hipEventElapsedTime(&out->tfa1_slicer_ms, tev[kMarkTfa1Slicer], tev[kMarkTfa1Coop]));
		HIPCHK(hipEventElapsedTime(&out->tfa1_coop_slicer_ms, tev[kMarkTfa1Coop], tev[kMarkTfa1Decode]));
		HIPCHK(hipEventElapsedTime(&out->tfa1_decode_commit_ms, tev[kMarkTfa1Decode], tev[kMarkTfa1End]));
	}
	if (has_whb) {
		HIPCHK(hipEventElapsedTime(&out->whb_biquad_ms, tev[kMarkWhbSpec], tev[kMarkWhbBiquadEnd]));
		HIPCHK(hipEventElapsedTime(&out->whb_demod_ms, tev[kMarkWhbDemod], tev[kMarkWhbDemodEnd]));
		if (hipEventQuery(tev[kMarkWhbCheckEnd]) == hipSuccess &&
		    hipEventElapsedTime(&out->whb_verify_ms, tev[kMarkWhbCheck], tev[kMarkWhbCheckEnd]) != hipSuccess)
			out->whb_verify_ms = 0;
		(void)hipGetLastError();
		// whb_decode_ms / whb_commit_ms stay 0: those stages run in the tail of whb_demod_kernel
	}
	return TFREC_AMD_OK;
}

int tfrec_amd_get_layout(tfrec_amd_ctx *c, int *n_streams)
{
	if (!c || !n_streams)
		return TFREC_AMD_E_INVAL;
	*n_streams = (c->cfg.flags & TFREC_AMD_F_SERIAL_CHAINS) ? 2 : (c->deep ? 6 : 4);
	return TFREC_AMD_OK;
}

int tfrec_amd_get_memory(tfrec_amd_ctx *c, uint64_t *device_bytes, uint64_t *pinned_host_bytes)
{
	if (!c || !device_bytes || !pinned_host_bytes)
		return TFREC_AMD_E_INVAL;
	*device_bytes = c->dev_bytes;
	for (size_t b : c->stage_bytes)  // staging of tfrec_amd_submit_host, grown on demand
		*device_bytes += b;
	*pinned_host_bytes = c->pinned_bytes;
	return TFREC_AMD_OK;
}

int tfrec_amd_get_stats(tfrec_amd_ctx *c, tfrec_amd_stats *out)
{
	if (!c || !out)
		return TFREC_AMD_E_INVAL;
	memset(out, 0, sizeof(*out));
	if (!c->win[0].stats)
		return TFREC_AMD_OK;
	int rc = tfrec_amd_sync(c);
	if (rc)
		return rc;
	constexpr int kCounters = (int)(sizeof(tfrec_amd_stats) / sizeof(uint64_t));
	static_assert(sizeof(tfrec_amd_stats) == 11 * sizeof(uint64_t) && kCounters <= 16, "the counters are the first slots of WinTables::stats");
	for (int k = 0; k < kSets; k++) {  // the table sets count separately
		tfrec_amd_stats part;
		HIPCHK(hipMemcpy(&part, c->win[k].stats, sizeof(part), hipMemcpyDeviceToHost));
		for (int i = 0; i < kCounters; i++)
			reinterpret_cast<uint64_t *>(out)[i] += reinterpret_cast<const uint64_t *>(&part)[i];
	}
	return TFREC_AMD_OK;
}

}  // extern "C"
