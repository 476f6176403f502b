// tfrec_amd/csrc/capi_submit.h -- submit and drain: included by capi.hip, which lists what is where.
#pragma once

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
	uint32_t *last;     // tfrec_amd_create_decimated: the stream's carried last pair, or nullptr
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
		if (R.last)
			R.last[s] = 0u;
	}
}
}  // namespace tfrec

// The set's front-end output for a submit of n_blocks blocks: what the launchers from the front end to the chains work on
static FrontOut front_out(const tfrec_amd_ctx *c, int set, int n_blocks)
{
	return { .dec = c->d_dec[set], .dec_stride = c->dec_stride, .mask = c->d_mask[set], .mask_stride = c->mask_stride,
		 .prevdec = c->d_prevdec[set], .fmdev = c->d_fmdev[set], .fmdev_stride = c->dec_stride,
		 .n_streams = c->cfg.n_streams, .n_blocks = n_blocks };
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
	if (c->submitted)  // (the level meter and the recorder of the last submit read d_scfg and own their carried state)
		for (const SideLane *l : { &c->lev.lane, &c->cap.lane })
			if (l->on)
				HIPCHK(hipStreamWaitEvent(fs, l->written[c->last_set], 0));
	const InputPath &I = c->input;
	const Restarts &r = c->restart;
	const StreamSettings &S = c->settings;
	const int nl = (int)r.pending.size();
	memcpy(r.h_list[set], r.pending.data(), (size_t)nl * sizeof(int32_t));  // (the set's last copy was drained)
	for (int i = 0; i < nl; i++)  // a reset stream restarts with its own current settings
		S.h_rcfg[set][i] = S.scfg[r.pending[i]];
	HIPCHK(hipMemcpyAsync(r.d_list[set], r.h_list[set], (size_t)nl * sizeof(int32_t), hipMemcpyHostToDevice, fs));
	HIPCHK(hipMemcpyAsync(S.d_rcfg[set], S.h_rcfg[set], (size_t)nl * sizeof(StreamCfg), hipMemcpyHostToDevice, fs));
	StreamReset R = { .list = r.d_list[set], .n_list = nl, .n_streams = c->cfg.n_streams,
			  .tail = I.history_read(I.tail), .tail_bytes = I.tail.bytes, .tail_fill = I.tail.fill,  // what this submit's front end
			  .pre = I.history_read(I.pre), .pre_bytes = I.pre.bytes, .pre_fill = I.pre.fill,        // and pre-stage read
			  .fsk = c->d_fsk, .lev = c->lev.d_state, .cap = c->cap.d_state, .cfgs = S.d_rcfg[set], .scfg = S.d_scfg,
			  .n_active = c->launch.n_active, .states = {}, .chain_init = r.d_chain_init, .tcarry = c->d_tcarry,
			  .whbx = c->d_whbx, .whbcarry = c->d_whbcarry, .whbX = c->d_whbX, .last = c->decin.d_last };
	std::copy_n(c->launch.states, R.n_active, R.states);
	hipLaunchKernelGGL(tfrec::stream_reset_kernel, dim3(nl), dim3(64), 0, fs, R);
	HIPCHK(hipGetLastError());
	return TFREC_AMD_OK;
}

// The tuned front end's per-stream {inc, phase} of this submit, queued on the front-end stream ahead of it.  The
// phase of the submit's first 1.536 MS/s sample n0 (4 per decimated sample, counted from the stream's start or restart --
// 0 for a stream that restarts with this submit) is (n0 * inc) mod 2^32, in 64-bit integers.  h_tune[set] is free: the
// set's previous submit, whose copy read it, has been drained.
static int stage_tune(tfrec_amd_ctx *c, int set)
{
	for (int s = 0; s < c->cfg.n_streams; s++) {
		const uint32_t inc = c->tunes.narrow.inc[s];
		const long long n0 = c->restart.marked[s] ? 0 : 4 * (c->sample_base - c->restart.origin[s]);
		c->tunes.h_tune[set][s] = make_uint2(inc, (uint32_t)((uint64_t)n0 * inc));
	}
	HIPCHK(hipMemcpyAsync(c->tunes.d_tune[set], c->tunes.h_tune[set], (size_t)c->cfg.n_streams * sizeof(uint2), hipMemcpyHostToDevice,
			      c->pipe[set].fs));
	return TFREC_AMD_OK;
}

// The per-stream {inc10, phase10, input row, 0} of this submit, staged like stage_tune's.  phase10 is the phase of
// the submit's first INPUT sample n0 (40 per decimated sample with TFREC_AMD_F_INPUT_10X): (n0 * inc10) mod 2^32.  A rate
// context (6g): {inc_in, ...} with n0 = 4 P / Q input samples per decimated sample -- whole, because every submit is.
static int stage_chan(tfrec_amd_ctx *c, int set)
{
	for (int s = 0; s < c->cfg.n_streams; s++) {
		const uint32_t inc = c->tunes.wide.inc[s];
		const long long n0 = c->restart.marked[s] ? 0 : 4 * (c->sample_base - c->restart.origin[s]) * c->input.rate.p / c->input.rate.q;
		c->tunes.h_chan[set][s] = make_uint4(inc, (uint32_t)((uint64_t)n0 * inc), (uint32_t)c->tunes.row[s], 0u);
	}
	HIPCHK(hipMemcpyAsync(c->tunes.d_chan[set], c->tunes.h_chan[set], (size_t)c->cfg.n_streams * sizeof(uint4), hipMemcpyHostToDevice,
			      c->pipe[set].fs));
	return TFREC_AMD_OK;
}

// rows of the input batch the streams read: 1 + the highest one mapped
static int rows_in_use(const tfrec_amd_ctx *c)
{
	if (!c->tunes.mapped)
		return c->cfg.n_streams;
	return 1 + *std::max_element(c->tunes.row.begin(), c->tunes.row.end());
}

// Bytes of one input row of a submit of n_blocks blocks: n_blocks * 32768 * P / Q complex samples of 2, 4 or 8 bytes each.
// n_blocks must be a multiple of rs_unit(Q) = Q / gcd(Q, 64) -- the odd part of a Q <= 64, so any n_blocks when that Q is a power
// of two --, which makes the samples a whole number and a multiple of 512.
static int input_bytes(const tfrec_amd_ctx *c, int n_blocks, size_t *bytes)
{
	if (n_blocks < 1)
		return TFREC_AMD_E_INVAL;
	const long long p = c->input.rate.p, q = c->input.rate.q;
	const long long num = (long long)n_blocks * (TFREC_AMD_BLOCK_BYTES / 2) * p;
	if (n_blocks % rs_unit(c->input.rate.q) != 0) {
		snprintf(g_err, sizeof(g_err), "%d blocks at the input rate %lld/%lld: a submit holds a multiple of %d blocks", n_blocks, p, q,
			 rs_unit(c->input.rate.q));
		return TFREC_AMD_E_INVAL;
	}
	*bytes = (size_t)(num / q) * fmt_sample_bytes(c->input.fmt);
	return TFREC_AMD_OK;
}

// The submit's input -> stage 0 (d_in16[set]) on the set's front-end stream.  chan: the set's {inc, phase, row, 0} per stream
// where a stream is mapped or has an input-rate tune (stage_chan), or nullptr.
static int launch_prestage(tfrec_amd_ctx *c, int set, const uint8_t *d_iq, size_t stride, int n_blocks, const uint4 *chan)
{
	const InputPath &I = c->input;
	hipStream_t fs = c->pipe[set].fs;
	const int n = c->cfg.n_streams;
	const History hist = I.history(I.pre);
	uint32_t *out = I.d_in16[set];
	switch (I.kind) {  // (no default: a new kind does not compile until it is handled)
	case PreStage::kDecim10:  // 15.36 MS/s u8 -> 1.536 MS/s int16 pairs
		HIPCHK(launch_decim10(fs, d_iq, stride, n, n_blocks, hist, out, I.in16_stride, chan));
		break;
	case PreStage::kIngest:  // 1.536 MS/s in another format -> x as int16 pairs
		HIPCHK(launch_ingest(fs, I.pre_fmt, d_iq, stride, n, n_blocks, out, I.in16_stride, chan));
		break;
	case PreStage::kResample:  // 1536000 P / Q S/s in any format -> 1.536 MS/s int16 pairs
		HIPCHK(launch_resample(fs, I.pre_fmt, d_iq, stride, n, n_blocks, I.rate, hist, out, I.in16_stride, chan, c->tunes.wide.n_tuned != 0));
		break;
	case PreStage::kNone:
	case PreStage::kChannel:  // (no pre-stage: submit_common asks in16() first)
		break;
	}
	return TFREC_AMD_OK;
}

// tfrec_amd_create_dc, tfrec_amd_create_iq: a submit may use at most max_rows input rows (checked before anything is queued)
static int check_correct_rows(const tfrec_amd_ctx *c)
{
	const InputCorrection &o = c->fix;
	if (!o.on() || rows_in_use(c) <= o.rows)
		return TFREC_AMD_OK;
	snprintf(g_err, sizeof(g_err), "the submit uses %d input rows, the %s was made for %d", rows_in_use(c), o.iq.k ? "IQ balancer" : "DC blocker",
		 o.rows);
	return TFREC_AMD_E_INVAL;
}

// the rows an estimator's reset call marked start again: m = head = 0
template <class Ring>
static int start_marked_rows(Estimator<Ring> &e, hipStream_t fs)
{
	for (int32_t r : e.reset_pending) {
		HIPCHK(hipMemsetAsync(e.d_state + r, 0, sizeof(int2), fs));
		e.reset_marked[r] = 0;
	}
	e.reset_pending.clear();
	return TFREC_AMD_OK;
}

// The input correction on the set's front-end stream, ahead of the pre-stage: the rows marked by
// tfrec_amd_reset_dc_rows or tfrec_amd_reset_iq_rows start again in that estimator, then the three kernels correct the submit's
// rows into the set's buffer.  The context's sums, moments, rings and states are ordered from submit to submit by the stream.
static int launch_correct_rows(tfrec_amd_ctx *c, int set, const uint8_t *d_iq, size_t stride, long n_in)
{
	InputCorrection &o = c->fix;
	hipStream_t fs = c->pipe[set].fs;
	TRY(start_marked_rows(o.dc, fs));
	TRY(start_marked_rows(o.iq, fs));
	const int rows = rows_in_use(c);
	const CorrectBufs b = { .dc_k = o.dc.k, .iq_k = o.iq.k, .win_stride = o.win_stride,
				.dc_sums = o.d_dc_sums, .iq_sums = o.d_iq_sums, .mom = o.d_mom,
				.dc_ring = o.dc.d_ring, .dc_state = o.dc.d_state, .iq_ring = o.iq.d_ring, .iq_state = o.iq.d_state,
				.d = o.dc.d_table[set], .tg = o.iq.d_table[set], .out = o.d_x[set], .out_stride = o.x_stride };
	HIPCHK(launch_correct(fs, c->input.fmt, d_iq, stride, rows, n_in, b));
	o.set_rows[set] = rows;
	o.set_windows[set] = (int)(n_in / 512);
	return TFREC_AMD_OK;
}

// The channel-rate front end in the place of the pre-stage and the front end: the dense kernel on the rows, or
// -- runs: tfrec_amd_submit_runs staged this set's table -- the sparse one
static int launch_decin_front(tfrec_amd_ctx *c, int set, const uint8_t *d_iq, size_t stride, const FrontOut &out, bool runs)
{
	hipStream_t fs = c->pipe[set].fs;
	const RunsIn &o = c->runs_in;
	uint32_t *last = c->decin.d_last;
	const int thresh = thresh_or_auto(c->cfg.thresh);
	const StreamCfg *scfg = c->settings.per_stream ? c->settings.d_scfg : nullptr;
	if (runs) {
		const RunsTables r = { .tab = o.d_tab[set], .pool = o.d_pool[set], .pre = o.d_pre[set], .first = o.d_first[set], .ov = o.d_ov[set] };
		HIPCHK(launch_decin_runs(fs, r, out, last, thresh, scfg));
		return TFREC_AMD_OK;
	}
	if (c->tunes.mapped)  // the kernel looks the row up
		TRY(stage_chan(c, set));
	HIPCHK(launch_decin(fs, d_iq, stride, c->tunes.mapped ? c->tunes.d_chan[set] : nullptr, out, last, thresh, scfg));
	return TFREC_AMD_OK;
}

// The burst track on the recorder's lane: the centre indices the submit runs with, staged like stage_tune's
// (h_idx[set] is free: the set's previous submit, whose copy read it, has been drained), then its three kernels.  In amplitude
// mode (6v) the staged values are the levels and the middle kernel is amplitude_kernel; in auto-centre mode (6w) they are the set
// centres in Hz, and the head's kernel and the centre's carry join the sequence; in phase mode (6x) they are too, and all three
// kernels are phase.h's
static int launch_track(tfrec_amd_ctx *c, int set, const FrontOut &out, const CaptureBufs &b)
{
	BurstTrack &o = c->trk;
	std::copy(o.idx.begin(), o.idx.end(), o.h_idx[set]);
	HIPCHK(hipMemcpyAsync(o.d_idx[set], o.h_idx[set], o.idx.size() * sizeof(int32_t), hipMemcpyHostToDevice, c->cap.lane.st));
	const TrackBufs k = { .recs = o.d_recs[set], .words = o.d_words[set], .centre = o.d_idx[set], .carry = o.d_carry, .prior = o.d_prior,
			      .smooth = o.smooth, .cen = o.cen.d_recs[set], .ccarry = o.d_ccarry, .head = o.head, .lag = o.lag };
	HIPCHK(o.lag         ? launch_burst_track_phase(c->cap.lane.st, out, b, k)
	       : o.cen.on    ? launch_burst_track_auto(c->cap.lane.st, out, b, k)
	       : o.amplitude ? launch_burst_track_amplitude(c->cap.lane.st, out, b, k)
			     : launch_burst_track(c->cap.lane.st, out, b, k));
	return TFREC_AMD_OK;
}

// The line code's buffers of a set
static CodeBufs code_bufs(const tfrec_amd_ctx *c, int set)
{
	const BurstCode &o = c->code;
	return { .recs = o.d_recs[set], .words = o.d_words[set], .trecs = c->trk.d_recs[set], .track = c->trk.d_words[set], .carry = o.d_carry,
		 .hist = o.d_hist, .rate = o.rate, .taps = o.taps, .flags = o.flags };
}

// The frame check's buffers of a set: its input is the bitmap the sync reads
static CrcBufs crc_bufs(const tfrec_amd_ctx *c, int set)
{
	const BurstCrc &o = c->crc;
	return { .recs = o.d_recs[set], .words = o.d_words[set], .track = c->code.on ? c->code.d_words[set] : c->trk.d_words[set], .carry = o.d_carry,
		 .hist = o.d_hist, .terms = o.d_terms, .n_terms = o.n_terms, .reach = o.reach, .width = o.width, .r0 = o.r0 };
}

// The burst sync's buffers of a set: with the line code on, the track it reads is the coded one
static SyncBufs sync_bufs(const tfrec_amd_ctx *c, int set)
{
	const BurstSync &o = c->syn;
	return { .recs = o.d_recs[set], .words = o.d_words[set], .track = c->code.on ? c->code.d_words[set] : c->trk.d_words[set], .carry = o.d_carry, .hist = o.d_hist,
		 .rate = o.rate, .n_bits = o.n_bits, .max_errors = o.max_errors, .flags = o.flags, .pattern = o.pattern };
}

// input_on_fs: the input was produced on the front-end stream itself (staged host input): no event needed
// runs: a sparse submit (tfrec_amd_submit_runs, which checked and staged everything on the front-end stream): there are no rows
static int submit_common(tfrec_amd_ctx *c, const void *d_iq, size_t stride, int n_blocks, void *hip_stream, bool input_on_fs,
			 bool runs = false)
{
	if (!c || !d_iq || n_blocks < 1 || n_blocks > c->cfg.max_blocks)
		return TFREC_AMD_E_INVAL;
	size_t row_bytes = 0;
	TRY(input_bytes(c, n_blocks, &row_bytes));
	if (!runs && ((stride % 16) != 0 || ((uintptr_t)d_iq % 16) != 0 ||
		      (rows_in_use(c) > 1 && stride < row_bytes))) {  // (one row in use: the stride is never applied)
		snprintf(g_err, sizeof(g_err), "IQ base and stream stride must be 16-byte aligned and >= one stream");
		return TFREC_AMD_E_INVAL;
	}
	TRY(check_correct_rows(c));
	TRY(check_fifo(c));
	TRY(check_live(c));
	HIPCHK(hipSetDevice(c->cfg.device));
	PoisonGuard guard(c);  // from here on work is enqueued: a failure leaves the carried state undefined
	const bool timing = (c->cfg.flags & TFREC_AMD_F_TIMING) != 0;
	const int set = (c->head + c->inflight) % kSets;  // this submit's buffer set, events and timing events
	const PipeCtl &P = c->pipe[set];
	const FrontOut out = front_out(c, set, n_blocks);
	const InputPath &I = c->input;
	const StreamTunes &T = c->tunes;
	const StreamCfg *scfg = c->settings.per_stream ? c->settings.d_scfg : nullptr;
	hipEvent_t *ev = c->ev[set];
	// Front end on its own stream: it starts when the caller's stream has produced the input, and may overlap the
	// chains of the previous submit (different buffer set; the set's previous user was drained, see the FIFO rule).
	// The chains run on internal streams: nothing of ours is queued on the caller's.
	hipStream_t fs = P.fs;
	if (!input_on_fs) {
		HIPCHK(hipEventRecord(c->ev_in[set], (hipStream_t)hip_stream));
		HIPCHK(hipStreamWaitEvent(fs, c->ev_in[set], 0));
	}
	if (c->spec.lane.on) {
		// the spectrum: it reads the raw rows and nothing else, so it is ordered behind the input's producer alone -- the wait the
		// front end makes, or (staged host input) the copy queued on fs just before -- and runs beside everything, on its own
		// low-priority stream.  The set's records were read or dropped when its previous submit was drained.
		if (input_on_fs)
			HIPCHK(hipEventRecord(c->ev_in[set], fs));
		HIPCHK(lane_after(c->spec.lane, c->ev_in[set]));
		const SpectrumBufs b = { .n_rows = std::min(rows_in_use(c), c->spec.rows), .n_in = (long)(row_bytes / fmt_sample_bytes(I.fmt)),
					 .n_bins = c->spec.n, .g = c->spec.g, .max_records = c->spec.max_records,
					 .sum = c->spec.d_sum[set], .peak = c->spec.d_peak[set], .nfr = c->spec.d_nf[set] };
		HIPCHK(launch_spectrum(c->spec.lane.st, I.fmt, (const uint8_t *)d_iq, stride, b));
		if (c->occ.lane.on)  // the occupancy detector: on the records just queued, in stream order behind their kernel
			HIPCHK(launch_occupancy(c->spec.lane.st, b, c->occ.ratio, c->occ.rel, c->occ.d_recs[set], c->occ.d_bits[set]));
		HIPCHK(lane_written(c->spec.lane, set));
		c->spec.set_rows[set] = b.n_rows;
		c->spec.set_records[set] = (int)((b.n_in / b.n_bins + b.g - 1) / b.g);
	}
	HIPCHK(hipMemcpyAsync(c->d_eb[set], c->d_eb_fresh, kEvFreshBytes, hipMemcpyDeviceToDevice, fs));  // (+ the overflow flag)
	if (timing)
		HIPCHK(hipEventRecord(ev[kEvSubmit], fs));
	const bool resets = !c->restart.pending.empty();
	if (resets)
		TRY(launch_resets(c, set));
	if (I.channel())
		TRY(launch_decin_front(c, set, (const uint8_t *)d_iq, stride, out, runs));
	const uint8_t *fin = (const uint8_t *)d_iq;
	size_t fstride = stride;
	// Who reads the set's {inc, phase, row, 0}: the pre-stage, for a mapped row or an input-rate tune -- or, a mapped context of
	// the default input, the front end, which then runs in its tuned form (the channel-rate kernel: launch_decin_front)
	const bool chan_pre = I.in16() && (T.mapped || T.wide.n_tuned), chan_front = I.front_maps() && T.mapped;
	const bool tuned = T.narrow.n_tuned || chan_front;
	if (chan_pre || chan_front)
		TRY(stage_chan(c, set));
	if (I.in16()) {  // ... then the standard cascade on int16 input
		const uint8_t *pin = (const uint8_t *)d_iq;
		size_t pstride = stride;
		if (c->fix.on()) {  // the input correction first: the pre-stage reads the corrected rows, an S16 input
			TRY(launch_correct_rows(c, set, pin, stride, (long)(row_bytes / fmt_sample_bytes(I.fmt))));
			pin = c->fix.d_x[set];
			pstride = c->fix.x_stride;
		}
		TRY(launch_prestage(c, set, pin, pstride, n_blocks, chan_pre ? T.d_chan[set] : nullptr));
		fin = (const uint8_t *)I.d_in16[set];
		fstride = I.in16_stride * sizeof(uint32_t);
	}
	if (tuned)
		TRY(stage_tune(c, set));
	if (!I.channel())
		HIPCHK(launch_frontend(fs, fin, fstride, I.history(I.tail), out, thresh_or_auto(c->cfg.thresh), c->taps, I.in16(),
				       tuned ? T.d_tune[set] : nullptr, chan_front ? T.d_chan[set] : nullptr));
	if (c->settings.n_auto)  // auto threshold: per-block thresholds rewrite the trigger mask (fm_demod.cpp:58-73)
		HIPCHK(launch_threshold(fs, out, c->d_fsk, c->wmax, scfg));
	if (timing)
		HIPCHK(hipEventRecord(ev[kEvFrontDone], fs));
	if (has_kind(c->launch, 1) && !c->fmdev_k2)  // FM discriminator of the samples near trigger windows (after the mask is final)
		HIPCHK(launch_fmdev(fs, out, c->d_eb[set], c->wmax, c->fm_flag_eps));
	if (timing)
		HIPCHK(hipEventRecord(ev[kEvFmdevDone], fs));
	HIPCHK(hipEventRecord(P.ev_front, fs));
	if (c->lev.lane.on) {  // the level meter: behind the front end (the mask is final), beside the chains, on its own low-priority stream
		HIPCHK(lane_after(c->lev.lane, P.ev_front));
		HIPCHK(launch_levels(c->lev.lane.st, out, c->lev.d_state, c->settings.d_scfg, c->lev.d_records[set]));
		HIPCHK(lane_written(c->lev.lane, set));
		c->lev.set_blocks[set] = n_blocks;
	}
	if (c->cap.lane.on) {  // the recorder: placed like the level meter, on a low-priority stream of its own
		HIPCHK(lane_after(c->cap.lane, P.ev_front));
		const CaptureBufs b = { .state = c->cap.d_state, .stage = c->cap.d_stage, .stage_cap = c->cap.stage_cap, .cnt = c->cap.d_cnt,
					.base = c->cap.d_base, .hdr = c->cap.d_hdr[set], .runs = c->cap.d_runs[set], .pool = c->cap.d_pool[set],
					.max_runs = c->cap.max_runs, .max_samples = c->cap.max_samples };
		HIPCHK(launch_capture(c->cap.lane.st, out, c->sample_base, b, c->settings.d_scfg));
		if (c->cap_pre.on)  // the pair ahead of every run: behind the copy kernel, which wrote the table
			HIPCHK(launch_capture_pre(c->cap.lane.st, out, c->sample_base, b, c->cap_pre.d_pre[set]));
		if (c->burst.on)  // the burst meter: behind the copy kernel too, on the table and the recorder's working set
			HIPCHK(launch_burst_meter(c->cap.lane.st, out, b, c->burst.d_recs[set]));
		if (c->env.on)  // the burst envelope: behind the copy kernel and the meter, on the table, the working set and the final mask
			HIPCHK(launch_burst_envelope(c->cap.lane.st, out, b, c->env.d_recs[set]));
		if (c->clk.on)  // the burst clock: behind the envelope, on the table, the working set and the decimated samples
			HIPCHK(launch_burst_clock(c->cap.lane.st, out, b, c->clk.d_recs[set]));
		if (c->trk.on)  // the burst track: behind the clock, on the table, the working set, the samples, the final mask and its own carry
			TRY(launch_track(c, set, out, b));
		if (c->code.on)  // the line code: behind the track's carry kernel, on the table, the working set, the track's records and bitmap and its own carry
			HIPCHK(launch_burst_code(c->cap.lane.st, out, b, code_bufs(c, set)));
		if (c->syn.on)  // the burst sync: behind the track's carry kernel, on the table, the working set, the track's bitmap and its own carry
			HIPCHK(launch_burst_sync(c->cap.lane.st, out, b, sync_bufs(c, set)));
		if (c->crc.on)  // the frame check: behind the code's (or the track's) carry kernel, on the table, the working set, the sync's input bitmap and its own carry
			HIPCHK(launch_burst_crc(c->cap.lane.st, out, b, crc_bufs(c, set)));
		HIPCHK(lane_written(c->cap.lane, set));
	}
	if (c->cfg.flags & TFREC_AMD_F_SERIAL_CHAINS) {
		HIPCHK(hipStreamWaitEvent(P.cs, P.ev_front, 0));
		HIPCHK(launch_chains(P.cs, out, c->sample_base, c->launch, c->d_events[set], c->d_eb[set], c->cfg.flags));
		if (timing)
			HIPCHK(hipEventRecord(ev[kEvSerialDone], P.cs));
		for (hipEvent_t e : P.done)
			HIPCHK(hipEventRecord(e, P.cs));
	} else {
		c->win[set].whb_submit_seq = c->submit_seq++;
		HIPCHK(launch_pipeline(P, out, c->sample_base, c->launch, c->win[set], c->d_ld16[set], c->d_dev32[set], c->d_events[set],
				       c->d_eb[set], c->cfg.flags));
	}
	report_debug_stats(c, set, n_blocks);
	// the drain's copies, queued now
	for (hipEvent_t e : P.done)
		HIPCHK(hipStreamWaitEvent(c->cpy, e, 0));
	// copied[set] then also says "the set's levels, captures and spectrum records are written" (their reads, and the set's reuse)
	for (const SideLane *l : { &c->lev.lane, &c->cap.lane, &c->spec.lane })
		if (l->on)
			HIPCHK(hipStreamWaitEvent(c->cpy, l->written[set], 0));
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
	Restarts &R = c->restart;
	for (int32_t s : R.pending) {
		R.origin[s] = c->sample_base;
		R.marked[s] = 0;
	}
	R.pending.clear();
	// (until the first reset the origins are all zero: nothing is recorded, and the drain subtracts nothing)
	R.any = R.any || resets;
	if (R.any)
		R.set_origin[set] = R.origin;
	c->submitted = true;
	c->inflight++;
	c->last_set = set;
	c->input.sel ^= 1;
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

static int submit_host_impl(tfrec_amd_ctx *c, const uint8_t *h_iq, size_t stride, int n_blocks)
{
	if (!c || !h_iq || n_blocks < 1 || n_blocks > c->cfg.max_blocks)
		return TFREC_AMD_E_INVAL;
	size_t row = 0;
	TRY(input_bytes(c, n_blocks, &row));
	if (rows_in_use(c) > 1 && stride < row)
		return TFREC_AMD_E_INVAL;
	TRY(check_correct_rows(c));
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

int tfrec_amd_submit_host(tfrec_amd_ctx *c, const uint8_t *h_iq, size_t stride, int n_blocks)
{
	const auto t0 = std::chrono::steady_clock::now();
	const int rc = submit_host_impl(c, h_iq, stride, n_blocks);
	if (c)
		c->hp_submit += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
	return rc;
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
	if (!c->restart.set_origin[set].empty()) {  // end_sample counts from the stream's last reset: flushes and BITS chunks (window opens) alike
		const std::vector<long long> &org = c->restart.set_origin[set];
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
