// tfrec_amd/csrc/capi_ctx.h -- the context: included by capi.hip, which lists what is where.
#pragma once

constexpr int kTuneLimit = 768000;  // |tune_hz| < half the 1.536 MS/s sample rate
constexpr int kTuneWideLimit = 7680000;  // tfrec_amd_tune_streams_wide: half the 15.36 MS/s input rate
// tfrec_amd_create_rate's denominators are tfrec_dev.h's: Q <= kRsQMax or Q | kRsQDiv
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

// fm_demod.cpp:23-27: thresh 0 selects the adaptive mode, which starts at 500
static int thresh_or_auto(int thresh) { return thresh ? thresh : 500; }

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

// A side output ("Side outputs"): its low-priority stream and, per set, the event behind the submit's kernels on it.
// The copy stream waits for every enabled lane's event, so copied[set] covers the side outputs: their reads and the set's reuse.
struct SideLane {
	bool on = false;
	hipStream_t st = nullptr;
	hipEvent_t written[kSets] = {};
};
// TFREC_AMD_F_LEVELS: carried state, per set the records ([n_streams][the submit's n_blocks]) and the block count
struct LevelsOut {
	SideLane lane;
	LevelState *d_state = nullptr;
	tfrec_amd_level *d_records[kSets] = {};
	int set_blocks[kSets] = {};
};
// tfrec_amd_enable_capture: carried state, the one working set of its kernels, per set table, pool and totals
struct CaptureOut {
	SideLane lane;
	uint32_t max_runs = 0;
	uint64_t max_samples = 0;
	CaptureState *d_state = nullptr;
	CaptureStage *d_stage = nullptr;
	int stage_cap = 0;
	uint2 *d_cnt = nullptr;
	uint4 *d_base = nullptr;
	CaptureHeader *d_hdr[kSets] = {};
	tfrec_amd_run *d_runs[kSets] = {};
	uint32_t *d_pool[kSets] = {};
	std::vector<tfrec_amd_run> tmp;
};
// tfrec_amd_enable_capture_pre: per set the pair ahead of every run of the set's table
struct CapturePre {
	bool on = false;
	uint32_t *d_pre[kSets] = {};
};
// A burst stage on the recorder's table: per set the record of every run of the set's table.  The whole of the
// meter's (tfrec_amd_enable_burst_meter, 6p), the envelope's (6r) and the clock's (6s) members; the base of the track's and the sync's
template <class Rec>
struct RunRecords {
	bool on = false;
	Rec *d_recs[kSets] = {};
};
// tfrec_amd_enable_burst_track: L; every stream's centre index as the next submit uses it; per set the records
// (RunRecords), the bitmap (ceil(max_samples / 32) words) and the submit's centre indices with their page-locked
// source; per stream the carried last 16 pairs and chain position (track_carry_kernel).  amplitude: the track's other mode
// (tfrec_amd_enable_burst_track_amplitude), in which idx, d_idx and h_idx hold every stream's level instead.  cen.on:
// its third mode (tfrec_amd_enable_burst_track_auto), in which they hold every stream's set centre in Hz, with K, per
// set the centre records and per stream the carried index and centre (centre_carry_kernel).  lag != 0: its fourth mode
// (tfrec_amd_enable_burst_track_phase), the third's buffers with 80 carried pairs per stream in d_carry, and m
struct BurstTrack : RunRecords<tfrec_amd_track> {
	bool amplitude = false;
	RunRecords<tfrec_amd_track_centre> cen;
	int head = 0;
	int lag = 0;
	int2 *d_ccarry = nullptr;
	int smooth = 0;
	size_t n_words = 0;
	std::vector<int32_t> idx;
	uint32_t *d_words[kSets] = {};
	int32_t *d_idx[kSets] = {}, *h_idx[kSets] = {};
	uint32_t *d_carry = nullptr, *d_prior = nullptr;
};
// tfrec_amd_enable_burst_sync: the settings; per set the records (RunRecords) and the match
// bitmap (the track's size); per stream the carried 64 words of track bits and H (sync_carry_kernel)
struct BurstSync : RunRecords<tfrec_amd_burst_sync> {
	int rate = 0, n_bits = 0, max_errors = 0;
	uint32_t flags = 0;
	unsigned long long pattern = 0;
	uint32_t *d_words[kSets] = {};
	uint32_t *d_carry = nullptr, *d_hist = nullptr;
};
// tfrec_amd_enable_burst_code: the settings; per set the records (RunRecords) and the coded bitmap (the track's
// size); per stream the carried 64 words of track bits and H (linecode_carry_kernel)
struct BurstCode : RunRecords<tfrec_amd_track> {
	int rate = 0;
	uint32_t taps = 0, flags = 0;
	uint32_t *d_words[kSets] = {};
	uint32_t *d_carry = nullptr, *d_hist = nullptr;
};
// tfrec_amd_enable_burst_crc: the settings as crc_kernel takes them (D, r0, the width, the terms' number); per set
// the records (RunRecords) and the check bitmap (the track's size); per stream the carried 512 words of input bits and H
// (crc_carry_kernel); once, the term table (8 N pairs)
struct BurstCrc : RunRecords<tfrec_amd_burst_crc> {
	int reach = 0, width = 0, n_terms = 0;
	uint32_t r0 = 0;
	uint32_t *d_words[kSets] = {};
	uint32_t *d_carry = nullptr, *d_hist = nullptr;
	uint2 *d_terms = nullptr;
};
// tfrec_amd_create_decimated (PreStage::kChannel): the carried last pair of every stream
struct DecIn {
	uint32_t *d_last = nullptr;
};
// tfrec_amd_enable_runs_input: the limits and, per set, the sparse submit's table ({ start, end, pool offset low, high } per run),
// pool, pre, first_run[n_streams + 1] and the prevdec overrides ({ use, pair } per stream) on the device, each with its page-locked
// source
struct RunsIn {
	bool on = false;
	uint32_t max_runs = 0;
	uint64_t max_samples = 0;
	uint4 *d_tab[kSets] = {}, *h_tab[kSets] = {};
	uint32_t *d_pool[kSets] = {}, *h_pool[kSets] = {}, *d_pre[kSets] = {}, *h_pre[kSets] = {};
	int32_t *d_first[kSets] = {}, *h_first[kSets] = {};
	uint2 *d_ov[kSets] = {}, *h_ov[kSets] = {};
};
// tfrec_amd_enable_spectrum: bins, frames per record, rows at most, records of the largest submit; per set sums and
// peaks ([rows][max_records][n]), frame counts ([rows][max_records]) and what the set's submit held (rows analysed, records)
struct SpectrumOut {
	SideLane lane;
	int n = 0, g = 0, rows = 0;
	size_t max_records = 0;
	unsigned long long *d_sum[kSets] = {}, *d_peak[kSets] = {};
	uint32_t *d_nf[kSets] = {};
	int set_rows[kSets] = {}, set_records[kSets] = {};
};
// tfrec_amd_enable_occupancy: the detector on the spectrum's records.  It runs on the spectrum's lane, behind its
// kernel (lane: only `on` is used; rows, records and what a set's submit held are the spectrum's); per set the records ([rows]
// [max_records]) and the bitmap words ([rows][max_records][n / 32])
struct OccupancyOut {
	SideLane lane;
	uint32_t ratio = 0, rel = 0;
	tfrec_amd_occupancy *d_recs[kSets] = {};
	uint32_t *d_bits[kSets] = {};
};

// One estimator of the input correction: K (0: the context has no such stage), the ring ([rows][K]) and the rows' {m, head}; per set
// the table of its estimates ([rows][win_stride] int16 pairs: d, or (t, g)).  reset_*: the rows its reset call marked since the last
// submit (each once).
template <class Ring>
struct Estimator {
	int k = 0;
	Ring *d_ring = nullptr;
	int2 *d_state = nullptr;
	uint32_t *d_table[kSets] = {};
	std::vector<int32_t> reset_pending;
	std::vector<uint8_t> reset_marked;
};
// tfrec_amd_create_dc / tfrec_amd_create_iq: the DC blocker, the IQ balancer, or the balancer behind the blocker,
// ahead of the pre-stage.  The rows a submit may use, the largest submit's windows and samples per row (x_stride bytes); per set
// the corrected rows (int16 x' << 2) the pre-stage reads and what the set's submit held; per context a submit's sums ([rows]
// [win_stride]: the blocker's {S_I, S_Q}, the balancer's five) and the balancer's moments.
struct InputCorrection {
	int rows = 0, win_stride = 0;
	size_t x_stride = 0;
	uint8_t *d_x[kSets] = {};
	int set_rows[kSets] = {}, set_windows[kSets] = {};
	Estimator<int2> dc;
	Estimator<IqMoments> iq;
	int2 *d_dc_sums = nullptr;
	IqSums *d_iq_sums = nullptr;
	IqMoments *d_mom = nullptr;
	bool on() const { return dc.k || iq.k; }
};

// What a context's input goes through ahead of the front end, resolved once from the constructor's InputSpec (create_with).
// Exactly these five exist; every question about the input is a test of the kind or one of InputPath's predicates.
enum class PreStage {
	kNone,      // u8 at 1.536 MS/s: the front end reads the rows
	kDecim10,   // TFREC_AMD_F_INPUT_10X: the 10:1 stage (u8 at 15.36 MS/s)
	kResample,  // tfrec_amd_create_rate, or a format at another rate: the resampling stage
	kIngest,    // tfrec_amd_create_format at the base rate (ingest_kernel): the format conversion
	kChannel,   // tfrec_amd_create_decimated (6n): channel-rate input, no front end at all
};
// A carried history of the input: `bytes` per stream, filled with `fill` after a start or a restart (bytes == 0: no such history,
// no buffers).  The buffers flip per submit with InputPath::sel.  make_front_buffers fills the record; history(), history_read(),
// launch_resets and launch_prestage read it, and nothing else computes a size or a fill.
struct Carried {
	uint8_t *buf[kSets] = {};  // [0], [1]; the 10x context's pre-stage has always owned one per set and uses two: kept, its memory totals too
	int bytes = 0, fill = 0;
};
// The context's input path.  fmt is the TFREC_AMD_FMT_* of the input rows, 0 (U8) in every context of the older constructors.  A
// context with an input correction keeps two formats: fmt stays the caller's (input_bytes, submit_host's staging, the spectrum),
// pre_fmt is what the pre-stage reads -- S16, the corrected rows (fix) -- and what its history is kept in; everywhere else pre_fmt
// == fmt.  The input rate is 1536000 rate.p / rate.q: 1/1, 10/1 (kDecim10), 1/4 (kChannel) or the P / Q of kResample, whose stage
// reads rate's tap table (launch.h; t and taps are its alone).  rate_abs: max_phi sum_n |h[phi][n]| of that table, for the guard of
// tfrec_amd_tune_streams_input (6g).
struct InputPath {
	PreStage kind = PreStage::kNone;
	int32_t fmt = TFREC_AMD_FMT_U8, pre_fmt = TFREC_AMD_FMT_U8;
	RateTable rate = { 1, 1, 0, nullptr };
	long long rate_abs = 0;
	// in16(): the pre-stage writes stage 0, 1.536 MS/s int16 pairs, one buffer per set, and the front end reads int16
	uint32_t *d_in16[kSets] = {};
	size_t in16_stride = 0;  // uint32 units
	// the front end's FIR history (every kind owns it; kChannel never reads it) and the pre-stage's history of the raw input or of x
	Carried tail, pre;
	int sel = 0;  // [sel] is what this submit reads -- and what its resets restore --, [sel ^ 1] what it writes for the next one

	bool in16() const { return kind == PreStage::kDecim10 || kind == PreStage::kResample || kind == PreStage::kIngest; }
	bool channel() const { return kind == PreStage::kChannel; }
	// tfrec_amd_tune_streams_wide / _input: a stage that mixes at the input rate
	bool input_tune() const { return kind == PreStage::kDecim10 || kind == PreStage::kResample; }
	// A mapped row (tfrec_amd_map_streams) is looked up by the first kernel on the rows: the pre-stage (in16()), the front end -- in its
	// tuned form, with the set's tune table -- or the channel-rate kernel.  The last two do it as per-stream variants: a map switches to them.
	bool front_maps() const { return kind == PreStage::kNone; }
	bool map_needs_per_stream() const { return !in16(); }
	uint8_t *history_read(const Carried &h) const { return h.buf[sel]; }
	History history(const Carried &h) const { return { h.buf[sel], h.buf[sel ^ 1] }; }
};

// tfrec_amd_configure_streams: every stream's settings as the next submit uses them (scfg, the host's copy; scfg_api as the caller
// gave them), their device copy as the last submit used them (d_scfg: written only by stream_reset_kernel, in the entries of its
// list), and the settings that travel with a submit's reset list (d_rcfg / h_rcfg).  per_stream: a stream was configured -- from
// then on the kernels read d_scfg (launch.scfg, taps.scfg); before, the uniform kernels run.  n_auto: streams of scfg in auto mode.
struct StreamSettings {
	std::vector<StreamCfg> scfg;
	std::vector<tfrec_amd_stream_config> scfg_api;
	StreamCfg *d_scfg = nullptr;
	StreamCfg *d_rcfg[kSets] = {}, *h_rcfg[kSets] = {};
	bool per_stream = false;
	int n_auto = 0;
};
// One tune: every stream's tune as the next submit uses it, its phase increment per sample, and the streams with inc != 0
struct Tune {
	std::vector<int32_t> hz;
	std::vector<uint32_t> inc;
	int n_tuned = 0;
};
// tfrec_amd_tune_streams (narrow: at 1.536 MS/s, DESIGN.md 6d -- while a stream is tuned the tuned front end runs; before, the kernels
// of an untuned context), tfrec_amd_tune_streams_wide / _input (wide: per input sample of the 10:1 or the resampling stage, 6e,
// 6g) and tfrec_amd_map_streams (row: the input row every stream reads from the next submit on, the identity until a stream is
// mapped).  Per set, filled by the submit: the {inc, phase of the submit's first sample} the front end reads (h_tune -> d_tune)
// and the {inc, phase, row, 0} of the kernel that looks the row up (h_chan -> d_chan; InputPath::front_maps).
struct StreamTunes {
	Tune narrow, wide;
	std::vector<int32_t> row;
	bool mapped = false;
	uint2 *d_tune[kSets] = {}, *h_tune[kSets] = {};
	uint4 *d_chan[kSets] = {}, *h_chan[kSets] = {};
};
// tfrec_amd_reset_streams: streams marked since the last submit (each once), and the per-stream sample origin -- the sample_base
// at the stream's last reset -- that the drain subtracts from end_sample.  A submit records the origins it ran with (set_origin),
// so that the drain of an older submit still in the FIFO uses the older ones.
struct Restarts {
	std::vector<int32_t> pending;
	std::vector<uint8_t> marked;
	std::vector<long long> origin;
	std::vector<long long> set_origin[kSets];  // empty: no submit before the set's one carried a reset
	int32_t *d_list[kSets] = {};  // the submit's reset list on the device (stream_reset_kernel)
	int32_t *h_list[kSets] = {};  // ... and its page-locked source
	ChainState *d_chain_init = nullptr;  // the constructor ChainState (chain_init_state), source of every reset
	bool any = false;  // a submit has carried a reset: set_origin is kept from then on
};

// tfrec_amd_save_streams / tfrec_amd_load_streams: the device staging of n_streams blobs and the list of the
// streams a call names, both made by the first call (nullptr before it)
struct StateStage {
	uint8_t *d_blobs = nullptr;
	int32_t *d_list = nullptr;
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
	// per set: what launch_pipeline takes for a submit of that set beside its FrontOut (the streams and the set's events); the
	// serial layout uses its fs, cs, ev_front and done
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
	LevelsOut lev;  // ---- side outputs
	CaptureOut cap;
	CapturePre cap_pre;
	RunRecords<tfrec_amd_burst> burst;
	RunRecords<tfrec_amd_envelope> env;
	RunRecords<tfrec_amd_clock> clk;
	BurstTrack trk;
	BurstSync syn;
	BurstCode code;
	BurstCrc crc;
	DecIn decin;
	RunsIn runs_in;
	SpectrumOut spec;
	OccupancyOut occ;
	int wmax = 0;
	InputPath input;  // ---- the input, resolved once (create_with); its stage-0 buffers, histories and tap table (make_front_buffers)
	StreamSettings settings;  // ---- per-stream tables, by concern (make_stream_settings, make_stream_tunes, make_restarts)
	StreamTunes tunes;
	Restarts restart;
	InputCorrection fix;
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
	bool submitted = false;              // pipe[last_set].done has been recorded
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
	StateStage state;  // ---- save / load (capi_state.h)
	// TFREC_AMD_HOST_PROF=1: host-side time of the submit / drain calls, printed when the context is destroyed
	double hp_submit = 0, hp_wait = 0, hp_copy = 0, hp_sort = 0, hp_gap = 0, hp_lat = 0, hp_s2s = 0;
	long hp_n = 0, hp_gap_n = 0;
};

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
		(void)hipGetLastError();  // reported here: the next submit's launch check must not find it ("Side outputs")
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
		(void)hipGetLastError();
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

static void release_one(const tfrec_amd_ctx::Owned &o)
{
	switch (o.kind) {
	case tfrec_amd_ctx::Owned::kDevice: (void)hipFree(o.h); break;
	case tfrec_amd_ctx::Owned::kPinned: (void)hipHostFree(o.h); break;
	case tfrec_amd_ctx::Owned::kStream: (void)hipStreamDestroy(static_cast<hipStream_t>(o.h)); break;
	case tfrec_amd_ctx::Owned::kEvent: (void)hipEventDestroy(static_cast<hipEvent_t>(o.h)); break;
	}
}

// what own_* recorded behind `mark`, newest first
static void release_behind(tfrec_amd_ctx *c, size_t mark)
{
	for (; c->owned.size() > mark; c->owned.pop_back())
		release_one(c->owned.back());
}

// everything recorded, and tfrec_amd_submit_host's staging
static void release_all(tfrec_amd_ctx *c)
{
	release_behind(c, 0);
	for (uint8_t *&p : c->d_stage) {
		(void)hipFree(p);
		p = nullptr;
	}
}

// An enable call (tfrec_amd_enable_capture, _spectrum, _occupancy) that fails half way leaves the context as it was before the call: what it
// made is given back, the byte counts of tfrec_amd_get_memory are restored and the feature's members are reset as a whole.
template <class Feature>
struct EnableGuard {
	tfrec_amd_ctx *c;
	Feature &f;
	size_t mark, dev_bytes, pinned_bytes;
	bool ok = false;
	EnableGuard(tfrec_amd_ctx *c_, Feature &f_) : c(c_), f(f_), mark(c_->owned.size()), dev_bytes(c_->dev_bytes), pinned_bytes(c_->pinned_bytes) {}
	~EnableGuard()
	{
		if (ok)
			return;
		release_behind(c, mark);
		c->dev_bytes = dev_bytes;
		c->pinned_bytes = pinned_bytes;
		f = Feature{};
	}
};

// ---- side lanes: the low-priority stream and one "written" event per set; a submit's wait ahead of its kernels and event behind
static int make_side_lane(tfrec_amd_ctx *c, SideLane &l)
{
	for (hipEvent_t &e : l.written)
		TRY(own_event(c, e, hipEventDisableTiming));
	int prio_lo = 0, prio_hi = 0;
	(void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
	return own_stream(c, l.st, prio_lo);
}
static hipError_t lane_after(const SideLane &l, hipEvent_t e) { return hipStreamWaitEvent(l.st, e, 0); }
static hipError_t lane_written(const SideLane &l, int set) { return hipEventRecord(l.written[set], l.st); }
