// tfrec_amd/host/device_worker.h -- one device context of a job and the host thread that drives it (see gpu_engine.h).
// The class and, below it, its steps: a header of gpu_engine.cpp alone, so that gpu_engine.cpp + main.cpp stay the whole adapter
// for whoever builds it (the host Makefile, and oracle/Makefile against the reference's decoders).
//
// engine::run (engine.cpp:63-93) for the dump files [s0, s1) on ONE device, as a three-stage pipeline over batches of
// bps blocks:
//   reader thread : fread batch k+2 of every file into a pinned host buffer (buffers in rotation)
//   GPU           : H2D copy + hot path of batch k+1 (tfrec_amd_submit_host is asynchronous on pinned memory)
//   worker thread : drain batch k's flush events and queue them for the engine's thread
// The C ABI's submit/drain FIFO (depth TFREC_AMD_FIFO_DEPTH = 4) is what lets batches k+1 .. k+3 be queued before batch
// k is drained; the worker keeps the FIFO full (one pinned host buffer per submit in flight + one being read).
#ifndef TFREC_AMD_HOST_DEVICE_WORKER_H
#define TFREC_AMD_HOST_DEVICE_WORKER_H

#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <thread>

#include "job.h"

class device_worker {
public:
	// files, file_blocks (blocks of every file of the job), settings: the whole job's; dflt: the context's thresh and filter (its
	// types are the union of the files' types); abort: set by the engine when any worker failed -- stop instead of running the
	// whole job.  All of them outlive the worker.
	device_worker(const job_settings &job, const std::vector<std::string> &files, const std::vector<size_t> &file_blocks,
		      const std::vector<file_settings> &settings, file_settings dflt, int device, size_t s0, size_t s1, int bps,
		      const std::atomic<bool> &abort);
	void start() { th = std::thread([this]() { run(); }); }
	// next batch's results (false: the worker ended -- rc says why)
	bool pop(batch_result &b);
	std::vector<batch_plan> plan;  // plan_batches
	int rc;
	std::thread th;

private:
	static constexpr int kBufs = TFREC_AMD_FIFO_DEPTH + 1;
	void run();
	int work();
	void push(batch_result &&b);
	void map_rows();
	int open_context();
	void read_batches();
	int submit(size_t k);
	int submit_runs(size_t k);
	int collect(size_t k, batch_result &b);
	int read_captures(size_t k, batch_result &b);
	template <class R>
	int read_run_records(size_t k, int (*reader)(tfrec_amd_ctx *, R *, size_t, uint32_t *), const char *noun, bool cut_opens, std::vector<R> &recs);
	template <class R>
	int read_run_bitmaps(int (*reader)(tfrec_amd_ctx *, R *, size_t, uint32_t *, uint32_t *, size_t, uint64_t *), std::vector<R> &recs,
			     std::vector<uint32_t> &words);
	int read_tracks(size_t k, batch_result &b);
	typedef int (*estimate_reader)(tfrec_amd_ctx *, int32_t, int16_t *, size_t, int *);
	int read_last_estimate(size_t k, estimate_reader reader, std::vector<int> &files, std::vector<int16_t> &last);
	int read_dc(size_t k, batch_result &b) { return read_last_estimate(k, tfrec_amd_read_dc, b.dc_file, b.dc_last); }  // -z -D
	int read_iq(size_t k, batch_result &b) { return read_last_estimate(k, tfrec_amd_read_iq, b.iq_file, b.iq_last); }  // -Z -D
	int close_context(int r);
	int load_kept();
	int save_ended(size_t k);

	const job_settings &job;
	const std::vector<std::string> &files;
	const std::vector<size_t> &file_blocks;
	const std::atomic<bool> &abort;
	const int device;
	const size_t s0, s1;
	file_settings dflt;  // the context's: the union of its files' types, thresh, filter
	size_t n;            // streams of the context
	const int bps;
	// to the engine's thread: batches drained, oldest first
	std::mutex mu;
	std::condition_variable cv;
	std::deque<batch_result> out;
	bool done;
	// the context (open_context .. close_context)
	tfrec_amd_ctx *ctx;
	int32_t max_events;
	std::vector<int32_t> in_row;  // map_rows: the input row each stream reads
	std::vector<bool> reads;      // the stream's file is read into its row (the first stream of the row)
	size_t n_rows;
	bool map;                     // streams share rows: the context's streams are mapped to them
	std::vector<bool> in_tune, narrow_tune;  // -r: the stream has an input-rate tune / a tune behind the resampler (split_tunes)
	// the reader thread: batch k goes to host[k % kBufs]; it may run at most kBufs batches ahead of the drain
	size_t row;  // bytes of one input row of a batch
	uint8_t *host[kBufs];
	bool pinned[kBufs];
	std::thread reader;
	std::mutex rmu;
	std::condition_variable rcv;
	size_t filled, drained;  // batches read / batches whose buffer is free again
	bool read_failed;
	// -R: per file of this device the blocks submitted so far and the first run that may reach into the next submit; one submit's
	// table, pool and pre
	std::vector<size_t> replay_pos, replay_from;
	std::vector<tfrec_amd_run> rtab;
	std::vector<int16_t> rpool, rpre;
};

inline device_worker::device_worker(const job_settings &job_, const std::vector<std::string> &files_, const std::vector<size_t> &file_blocks_,
			     const std::vector<file_settings> &settings, file_settings dflt_, int device_, size_t s0_, size_t s1_, int bps_,
			     const std::atomic<bool> &abort_)
	: rc(0), job(job_), files(files_), file_blocks(file_blocks_), abort(abort_), device(device_), s0(s0_), s1(s1_), dflt(dflt_),
	  n(s1_ - s0_), bps(bps_), done(false), ctx(NULL), max_events(0), n_rows(0), map(false), row(0), filled(0), drained(0),
	  read_failed(false)
{
	dflt.types = 0;
	for (size_t s = s0; s < s1; s++)
		dflt.types |= settings[s].types;
	if (job.slots > 0)
		n = std::min(n, (size_t)job.slots);
	plan = plan_batches(file_blocks, settings, dflt, s0, s1, n, bps, job.keeping());
}

inline void device_worker::push(batch_result &&b)
{
	{
		std::unique_lock<std::mutex> lk(mu);
		cv.wait(lk, [&]() { return out.size() < 2; });  // the engine's thread is at most two batches behind
		out.push_back(std::move(b));
	}
	cv.notify_all();
}

inline bool device_worker::pop(batch_result &b)
{
	std::unique_lock<std::mutex> lk(mu);
	cv.wait(lk, [&]() { return !out.empty() || done; });
	if (out.empty())
		return false;
	b = std::move(out.front());
	out.pop_front();
	lk.unlock();
	cv.notify_all();
	return true;
}

inline void device_worker::run()
{
	rc = work();
	{
		std::lock_guard<std::mutex> lk(mu);
		done = true;
	}
	cv.notify_all();
}

inline int device_worker::work()
{
	map_rows();
	int r = open_context();
	if (r)
		return r;
	const int depth = std::max(1, std::min(tfrec_amd_fifo_depth(), TFREC_AMD_FIFO_DEPTH));
	row = job.replay ? 0 : (size_t)(bps / job.unit()) * job.piece_bytes();  // (-R: nothing is read, the tables are in memory)
	for (int b = 0; b < kBufs; b++) {
		host[b] = (uint8_t *)tfrec_amd_host_alloc(n_rows * row);
		pinned[b] = host[b] != NULL;  // per buffer: each is released by the allocator it came from
		if (!host[b])  // no page-locked memory: this buffer's copies become synchronous, results are the same
			host[b] = (uint8_t *)malloc(n_rows * row);
	}
	if (!job.replay)
		reader = std::thread([this]() { read_batches(); });
	size_t queued = 0;
	for (size_t k = 0; k < plan.size() && r == 0; k++) {
		while (queued < plan.size() && queued < k + (size_t)depth && r == 0)
			r = submit(queued++);
		if (r)
			break;
		if (abort.load()) {
			r = TFREC_AMD_E_STATE;
			break;
		}
		batch_result b;
		r = collect(k, b);
		if (!r)
			push(std::move(b));
	}
	if (!r && job.keeping())  // -k: the files that ended with the last batch
		r = save_ended(plan.size());
	return close_context(r);
}

// Which stream reads which input row.  Shared inputs (tfrec_amd_map_streams): without -n a stream carries one file for the whole
// job, and the streams whose files are one path share that path's input row -- the file is opened and read once, staged and
// copied once.  Decoders, stream indices and the order of the output stay per -L occurrence.  (A stream without a file reads
// row 0; its events are dropped.)  Otherwise stream s reads row s.
inline void device_worker::map_rows()
{
	in_row.assign(n, 0);
	reads.assign(n, true);
	std::vector<std::string> paths;
	if (job.share() && !plan.empty())
		for (size_t s = 0; s < n; s++) {
			const int f = plan[0].file[s];
			if (f < 0)
				continue;
			const size_t r = std::find(paths.begin(), paths.end(), files[f]) - paths.begin();
			reads[s] = r == paths.size();
			if (reads[s])
				paths.push_back(files[f]);
			in_row[s] = (int32_t)r;
		}
	map = job.share() && !plan.empty() && paths.size() < n;
	n_rows = map ? std::max<size_t>(1, paths.size()) : n;
	for (size_t s = 0; s < n && !map; s++)
		in_row[s] = (int32_t)s;
}

// tfrec_amd_create*, then tfrec_amd_map_streams, then the enables the job asks for; a call that fails is named on stderr and
// leaves no context behind
inline int device_worker::open_context()
{
	tfrec_amd_config cfg;
	memset(&cfg, 0, sizeof(cfg));
	cfg.n_streams = (int32_t)n;
	cfg.types_mask = dflt.types;
	cfg.thresh = dflt.thresh;
	cfg.filter_type = dflt.filter;
	cfg.device = device;
	cfg.max_blocks = bps;
	// (BITS mode: every flush + a chunk per 512 bits, a slicer emits < 0.5 bit per decimated sample)
	cfg.max_events = max_events = (int32_t)std::max<size_t>(4096, n * (size_t)bps * (job.bits_replay ? 256 : 64));
	cfg.flags = job.ctx_flags();
	in_tune.assign(n, false);
	narrow_tune.assign(n, false);
	const char *call = "tfrec_amd_create";
	// (the rows are known: -z and -Z size the blocker and the balancer for them)
	int r = job.replay		       ? tfrec_amd_create_decimated(&cfg, &ctx)
		: job.iq_windows	       ? tfrec_amd_create_iq(&cfg, job.fmt, job.rate_p, job.rate_q, job.dc_windows, job.iq_windows, (int32_t)n_rows, &ctx)
		: job.dc_windows	       ? tfrec_amd_create_dc(&cfg, job.fmt, job.rate_p, job.rate_q, job.dc_windows, (int32_t)n_rows, &ctx)
		: job.fmt != TFREC_AMD_FMT_U8  ? tfrec_amd_create_format(&cfg, job.fmt, job.rate_p, job.rate_q, &ctx)
		: job.resampled()	       ? tfrec_amd_create_rate(&cfg, job.rate_p, job.rate_q, &ctx)
					       : tfrec_amd_create(&cfg, &ctx);
	const bool created = r == 0;
	if (!r && map) {
		std::vector<int32_t> all(n);
		for (size_t s = 0; s < n; s++)
			all[s] = (int32_t)s;
		call = "tfrec_amd_map_streams";
		r = tfrec_amd_map_streams(ctx, all.data(), in_row.data(), (int)n);
	}
	if (!r && job.recorder()) {  // -S, sized so that no submit overflows: every sample, and a stream's runs are >= 356 samples long but two
		call = "tfrec_amd_enable_capture";  // (-M, -Q or -C without -S: the table alone, a pool of one pair; -G: the bitmap has the pool's size)
		r = tfrec_amd_enable_capture(ctx, (uint32_t)(n * ((size_t)bps * TFREC_AMD_BLOCK_DEC / 356 + 3)),
					     job.capture || job.tracking() ? (uint64_t)n * (uint64_t)bps * TFREC_AMD_BLOCK_DEC : 1);
	}
	if (!r && job.capture) {  // ... and the pair ahead of every run
		call = "tfrec_amd_enable_capture_pre";
		r = tfrec_amd_enable_capture_pre(ctx);
	}
	if (!r && job.metering()) {  // -M: the meter on the recorder's table
		call = "tfrec_amd_enable_burst_meter";
		r = tfrec_amd_enable_burst_meter(ctx);
	}
	if (!r && job.enveloping()) {  // -Q: the envelope on the recorder's table
		call = "tfrec_amd_enable_burst_envelope";
		r = tfrec_amd_enable_burst_envelope(ctx);
	}
	if (!r && job.clocking()) {  // -C: the clock on the recorder's table
		call = "tfrec_amd_enable_burst_clock";
		r = tfrec_amd_enable_burst_clock(ctx);
	}
	if (!r && job.amplitude()) {  // -G -O: the track in amplitude mode, every stream at the one level
		call = "tfrec_amd_enable_burst_track_amplitude";
		r = tfrec_amd_enable_burst_track_amplitude(ctx, job.track_smooth());
		if (!r && job.track_level) {
			std::vector<int32_t> all(n), level(n, (int32_t)job.track_level);
			for (size_t i = 0; i < n; i++)
				all[i] = (int32_t)i;
			call = "tfrec_amd_set_burst_track_level";
			r = tfrec_amd_set_burst_track_level(ctx, all.data(), level.data(), (int)n);
		}
	} else if (!r && job.phasing()) {  // -G rate,psk: the track in phase mode, the fallback centre 0
		call = "tfrec_amd_enable_burst_track_phase";
		r = tfrec_amd_enable_burst_track_phase(ctx, job.track_smooth(), kTrackAutoHead, job.track_lag);
	} else if (!r && job.centring()) {  // -G rate,auto: the track in auto-centre mode, the fallback centre 0
		call = "tfrec_amd_enable_burst_track_auto";
		r = tfrec_amd_enable_burst_track_auto(ctx, job.track_smooth(), kTrackAutoHead);
	} else if (!r && job.tracking()) {  // -G: the track on the recorder's table, every stream about the one centre
		call = "tfrec_amd_enable_burst_track";
		r = tfrec_amd_enable_burst_track(ctx, job.track_smooth());
		if (!r && job.track_centre) {
			std::vector<int32_t> all(n), hz(n, (int32_t)job.track_centre);
			for (size_t s = 0; s < n; s++)
				all[s] = (int32_t)s;
			call = "tfrec_amd_set_burst_track_centre";
			r = tfrec_amd_set_burst_track_centre(ctx, all.data(), hz.data(), (int)n);
		}
	}
	if (!r && job.coding()) {  // -U: the line code on the track, at -G's rate
		call = "tfrec_amd_enable_burst_code";
		r = tfrec_amd_enable_burst_code(ctx, (int32_t)job.track_rate, job.code_taps, job.code_invert ? TFREC_AMD_CODE_INVERT : 0u);
	}
	if (!r && job.syncing()) {  // -Y: the sync on the track, at -G's rate
		call = "tfrec_amd_enable_burst_sync";
		r = tfrec_amd_enable_burst_sync(ctx, (int32_t)job.track_rate, job.sync_pattern, job.sync_bits, job.sync_errors,
						job.sync_both ? TFREC_AMD_SYNC_BOTH : 0u);
	}
	if (!r && job.checking()) {  // -V: the frame check on the sync's input track, at -G's rate, on -Y's bytes
		const tfrec_crc::Settings s = job.crc_settings();
		call = "tfrec_amd_enable_burst_crc";
		r = tfrec_amd_enable_burst_crc(ctx, s.rate, s.n_bytes, s.skip, s.width, s.poly, s.init, s.xorout, s.flags);
	}
	if (!r && job.replay) {  // -R, sized so that every submit fits: its files' runs (a cut adds one per stream), every sample at most
		uint64_t runs = 0, pairs = 0;
		for (size_t f = s0; f < s1; f++) {
			runs += (*job.replay)[f].runs.size();
			pairs += (*job.replay)[f].pool.size() / 2;
		}
		runs = std::min<uint64_t>(runs + n, (uint64_t)n * ((uint64_t)bps * TFREC_AMD_BLOCK_DEC / 2 + 1));
		pairs = std::min<uint64_t>(pairs, (uint64_t)n * (uint64_t)bps * TFREC_AMD_BLOCK_DEC);
		call = "tfrec_amd_enable_runs_input";
		r = tfrec_amd_enable_runs_input(ctx, (uint32_t)std::max<uint64_t>(1, runs), std::max<uint64_t>(1, pairs));
		replay_pos.assign(s1 - s0, 0);
		replay_from.assign(s1 - s0, 0);
	}
	if (!r && job.spectrum) {  // -P: the one file's row
		call = "tfrec_amd_enable_spectrum";
		r = tfrec_amd_enable_spectrum(ctx, job.spec_n, job.spec_g, 1);
	}
	if (!r && job.occupancy()) {  // -A: the detector on its records
		call = "tfrec_amd_enable_occupancy";
		r = tfrec_amd_enable_occupancy(ctx, (uint32_t)job.occ_ratio, (uint32_t)job.occ_rel);
	}
	if (r) {
		fprintf(stderr, "%s (device %d): %s (%s)\n", call, device, tfrec_amd_strerror(r), tfrec_amd_last_error());
		if (created)
			tfrec_amd_destroy(ctx);
	}
	return r;
}

// the reader thread: a file is opened when its first batch is read and closed after its last one (a queue of thousands of files)
inline void device_worker::read_batches()
{
	std::vector<FILE *> fd(s1 - s0, (FILE *)NULL);
	std::vector<size_t> fleft(file_blocks.begin() + s0, file_blocks.begin() + s1);
	std::vector<size_t> head_pos(s1 - s0, 0);  // -K: bytes of the file's carried-in rest read so far
	const size_t piece = job.piece_bytes();
	for (size_t k = 0; k < plan.size(); k++) {
		{
			std::unique_lock<std::mutex> lk(rmu);
			rcv.wait(lk, [&]() { return k < drained + kBufs; });
		}
		const batch_plan &b = plan[k];
		uint8_t *buf = host[k % kBufs];
		for (size_t s = 0; s < n; s++) {
			if (n_rows < n && (!reads[s] || b.file[s] < 0))
				continue;  // (a shared row is filled by its first stream)
			uint8_t *dst = buf + (size_t)in_row[s] * row;
			const size_t want = (size_t)(b.nb / job.unit()) * piece;
			const int f = b.file[s];
			size_t got = 0;
			if (f >= 0) {
				FILE *&fp = fd[f - s0];
				if (!fp && !read_failed && !(fp = fopen(files[f].c_str(), "rb"))) {
					perror(files[f].c_str());
					read_failed = true;
				}
				if (fp) {
					if (job.cont) {  // -K: the rest of the part before comes ahead of the file's own bytes
						const std::vector<uint8_t> &head = (*job.cont)[f].rest;
						size_t &pos = head_pos[f - s0];
						got = std::min(want, head.size() - pos);
						memcpy(dst, head.data() + pos, got);
						pos += got;
					}
					got += fread(dst + got, 1, want - got, fp);
					got -= got % piece;
					size_t &left = fleft[f - s0];
					left -= std::min<size_t>(left, (size_t)b.nb);
					if (left == 0) {
						fclose(fp);
						fp = NULL;
					}
				}
			}
			// a shorter file is padded with silence (its events are cut by the engine): u8 128, zero in every other format
			memset(dst + got, job.fmt != TFREC_AMD_FMT_U8 ? 0 : 0x80, want - got);
		}
		{
			std::lock_guard<std::mutex> lk(rmu);
			filled = k + 1;
		}
		rcv.notify_all();
	}
	for (FILE *fp : fd)
		if (fp)
			fclose(fp);
}

// batch k, once the reader has filled its buffer: the resets, configures and tunes its plan asks for, then the submit
inline int device_worker::submit(size_t k)
{
	if (!job.replay) {
		std::unique_lock<std::mutex> lk(rmu);
		rcv.wait(lk, [&]() { return filled > k; });
	}
	const batch_plan &b = plan[k];
	int r = job.keeping() ? save_ended(k) : 0;
	if (r)
		return r;
	if (job.cont && k == 0) {  // -K: the saved settings, tunes and state instead of the files' own configure and tune
		r = load_kept();
		return r ? r : tfrec_amd_submit_host(ctx, host[k % kBufs], row, b.nb);
	}
	if ((job.dc_windows || job.iq_windows) && !job.share()) {
		// -n with -z or -Z: a slot that starts a new file -- by a reset, or by the configure or tune its next file needs -- starts a
		// new DC and a new IQ estimate too.  A stream's row is its own here (nothing is shared); duplicates are allowed.
		std::vector<int32_t> rows(b.reset);
		rows.insert(rows.end(), b.conf.begin(), b.conf.end());
		rows.insert(rows.end(), b.tune.begin(), b.tune.end());
		if (job.dc_windows)
			r = tfrec_amd_reset_dc_rows(ctx, rows.data(), (int)rows.size());
		if (!r && job.iq_windows)
			r = tfrec_amd_reset_iq_rows(ctx, rows.data(), (int)rows.size());
	}
	if (!r && !b.reset.empty())  // the streams whose file ended in the batch before: fresh receivers for the next files
		r = tfrec_amd_reset_streams(ctx, b.reset.data(), (int)b.reset.size());
	if (!r && !b.conf.empty())  // ... with the settings of their next file
		r = tfrec_amd_configure_streams(ctx, b.conf.data(), b.conf_cfg.data(), (int)b.conf.size());
	if (!r && !b.tune.empty() && job.resampled()) {  // ... and tunes, -r: behind the resampler and ahead of it (split_tunes)
		const tune_calls c = split_tunes(b.tune, b.tune_hz, in_tune, narrow_tune);
		if (!c.narrow.empty())
			r = tfrec_amd_tune_streams(ctx, c.narrow.data(), c.narrow_hz.data(), (int)c.narrow.size());
		if (!r && !c.input.empty())
			r = tfrec_amd_tune_streams_input(ctx, c.input.data(), c.input_hz.data(), (int)c.input.size());
	} else if (!r && !b.tune.empty()) {  // ... and tunes
		r = job.wide ? tfrec_amd_tune_streams_wide(ctx, b.tune.data(), b.tune_hz.data(), (int)b.tune.size())
			     : tfrec_amd_tune_streams(ctx, b.tune.data(), b.tune_hz.data(), (int)b.tune.size());
	}
	if (r)
		return r;
	return job.replay ? submit_runs(k) : tfrec_amd_submit_host(ctx, host[k % kBufs], row, b.nb);
}

// -K: every file's saved state into its stream, ahead of the first batch (without -n every file starts there)
inline int device_worker::load_kept()
{
	size_t bytes = 0;
	int r = tfrec_amd_stream_state_bytes(ctx, &bytes);
	std::vector<int32_t> streams;
	std::vector<uint8_t> blobs;
	for (size_t s = 0; s < n && !r; s++) {
		const int f = plan[0].file[s];
		if (f < 0)
			continue;
		const std::vector<uint8_t> &st = (*job.cont)[f].state;
		if (st.size() != bytes) {
			fprintf(stderr, "%s: %zu bytes, a stream's state in this run takes %zu (other -T, -x, -r, -F, -z or -Z than the run that kept it?)\n",
				job_settings::kept_path(job.cont_prefix, (size_t)f, ".state").c_str(), st.size(), bytes);
			return TFREC_AMD_E_INVAL;
		}
		streams.push_back((int32_t)s);
		blobs.insert(blobs.end(), st.begin(), st.end());
	}
	return r ? r : tfrec_amd_load_streams(ctx, streams.data(), (int)streams.size(), blobs.data(), blobs.size());
}

// -k: the streams whose file's last batch was batch k - 1, saved to <prefix>.<file>.state before batch k is submitted (k ==
// plan.size(): at the end of the job).  The save waits for everything queued and drains nothing.
inline int device_worker::save_ended(size_t k)
{
	if (k == 0)
		return 0;
	std::vector<int32_t> streams;
	for (size_t s = 0; s < n; s++)
		if (plan[k - 1].file[s] >= 0 && (k == plan.size() || plan[k].file[s] != plan[k - 1].file[s]))
			streams.push_back((int32_t)s);
	if (streams.empty())
		return 0;
	size_t bytes = 0;
	int r = tfrec_amd_stream_state_bytes(ctx, &bytes);
	std::vector<uint8_t> blobs(streams.size() * bytes);
	if (!r)
		r = tfrec_amd_save_streams(ctx, streams.data(), (int)streams.size(), blobs.data(), blobs.size());
	for (size_t i = 0; i < streams.size() && !r; i++) {
		const std::string path = job_settings::kept_path(job.keep_prefix, (size_t)plan[k - 1].file[streams[i]], ".state");
		FILE *fp = fopen(path.c_str(), "wb");
		const bool ok = fp && fwrite(blobs.data() + i * bytes, 1, bytes, fp) == bytes;
		if ((fp && fclose(fp)) || !ok) {
			perror(path.c_str());
			r = TFREC_AMD_E_INVAL;
		}
	}
	return r;
}

// -R: batch k as a sparse submit -- every stream's part of its file's capture (the tables are ordered by stream)
inline int device_worker::submit_runs(size_t k)
{
	const batch_plan &b = plan[k];
	rtab.clear();
	rpool.clear();
	rpre.clear();
	for (size_t s = 0; s < n; s++) {
		const int f = b.file[s];
		if (f < 0)
			continue;
		size_t &pos = replay_pos[f - s0];
		rebase_runs((*job.replay)[f], (uint32_t)s, (long long)pos * TFREC_AMD_BLOCK_DEC, (long long)b.nb * TFREC_AMD_BLOCK_DEC, replay_from[f - s0],
			    rtab, rpool, rpre);
		pos += (size_t)b.nb;
	}
	return tfrec_amd_submit_runs(ctx, rtab.data(), (uint32_t)rtab.size(), rpool.data(), rpool.size() / 2, rpre.data(), b.nb);
}

// -S: the batch's captures.  stream -> file, as for the events; a run is cut at its file's end
inline int device_worker::read_captures(size_t k, batch_result &b)
{
	uint32_t nr = 0;
	uint64_t np = 0;
	int r = tfrec_amd_read_captures(ctx, NULL, 0, &nr, NULL, 0, &np);  // (the counts: E_INVAL for want of room)
	if (r == TFREC_AMD_E_INVAL && nr) {
		b.runs.resize((size_t)nr + 1);
		b.pool.resize(2 * (size_t)np + 2);
		r = tfrec_amd_read_captures(ctx, b.runs.data(), b.runs.size(), &nr, b.pool.data(), b.pool.size() / 2, &np);
		if (r == 0 || r == TFREC_AMD_E_OVERFLOW) {  // the pair ahead of every run delivered
			uint32_t npre = 0;
			b.pre.resize(2 * ((size_t)nr + 1));
			const int rp = tfrec_amd_read_capture_pre(ctx, b.pre.data(), b.pre.size() / 2, &npre);
			if (rp != 0 && rp != TFREC_AMD_E_OVERFLOW)
				r = rp;
		}
	}
	size_t have = nr;
	if (r == TFREC_AMD_E_OVERFLOW) {  // the runs that fitted were returned (n_samples == 0 ends them); the job goes on
		for (have = 0; have < b.runs.size() && b.runs[have].n_samples; have++) {
		}
		fprintf(stderr, "tfrec_amd: device %d batch %zu: capture overflow, %zu of %u runs kept\n", device, k, have, (unsigned)nr);
		r = 0;
	}
	if (r)
		return r;
	const std::vector<int> &file = plan[k].file;
	size_t kept = 0;
	for (size_t q = 0; q < have; q++) {
		tfrec_amd_run x = b.runs[q];
		if (x.stream >= file.size() || file[x.stream] < 0)
			continue;
		const long long end = (long long)file_blocks[file[x.stream]] * TFREC_AMD_BLOCK_DEC;
		if (x.start_sample >= end)
			continue;
		x.n_samples = (uint32_t)std::min<long long>(x.n_samples, end - x.start_sample);
		b.file.push_back(file[x.stream]);
		b.pre[2 * kept] = b.pre[2 * q];
		b.pre[2 * kept + 1] = b.pre[2 * q + 1];
		b.runs[kept++] = x;
	}
	b.runs.resize(kept);
	b.pre.resize(2 * kept);
	return 0;
}

// -M, -Q, -C: the batch's records of one burst stage by the stage's reader: the count, then the records; an overflow is reported and
// the job goes on.  Then stream -> file, as for the events, and the file-end cut (job.h: cut_at_file_end): a record that begins
// behind its file's end is dropped, one that reaches over it has its n_samples cut there and, but for -M, is OPEN
template <class R>
inline int device_worker::read_run_records(size_t k, int (*reader)(tfrec_amd_ctx *, R *, size_t, uint32_t *), const char *noun, bool cut_opens,
					   std::vector<R> &recs)
{
	uint32_t nr = 0;
	int r = reader(ctx, NULL, 0, &nr);  // (the count: E_INVAL for want of room)
	if (r == TFREC_AMD_E_INVAL && nr) {
		recs.resize(nr);
		r = reader(ctx, recs.data(), recs.size(), &nr);
	}
	if (r == TFREC_AMD_E_OVERFLOW) {  // (cannot happen: the table is sized for the worst case)
		fprintf(stderr, "tfrec_amd: device %d batch %zu: more runs than the table holds, %zu of %u %s records kept\n", device, k, recs.size(),
			(unsigned)nr, noun);
		r = 0;
	}
	if (r)
		return r;
	size_t kept = 0;
	for (size_t q = 0; q < recs.size(); q++) {
		R x = recs[q];
		if (cut_at_file_end(x, plan[k].file, file_blocks, cut_opens))
			recs[kept++] = x;
	}
	recs.resize(kept);
	return 0;
}

// -G, -Y: the batch's records and bitmap words of one stage by the stage's reader: the counts, then both
template <class R>
inline int device_worker::read_run_bitmaps(int (*reader)(tfrec_amd_ctx *, R *, size_t, uint32_t *, uint32_t *, size_t, uint64_t *),
					   std::vector<R> &recs, std::vector<uint32_t> &words)
{
	uint32_t nr = 0;
	uint64_t nw = 0;
	int r = reader(ctx, NULL, 0, &nr, NULL, 0, &nw);  // (the counts: E_INVAL for want of room)
	if (r == TFREC_AMD_E_INVAL && nr) {
		recs.resize(nr);
		words.resize((size_t)nw + 1);
		r = reader(ctx, recs.data(), recs.size(), &nr, words.data(), words.size(), &nw);
	}
	return r;
}

// -G: the batch's track records, each with its bits out of the batch's bitmap.  stream -> file and the file-end cut as above; a
// record that reaches over its file's end is cut there and is OPEN (job.h: track_take).  -Y: the sync records of the same entries
// with them, each with its match track (job.h: sync_take), in b.syncs in place of b.tracks.  -G rate,auto: every track piece with
// the centre record of its entry (job.h: centre_take).  -U: the coded records of the same entries too, each a track piece of its
// own with the coded bits (cut alike): in b.codes beside b.tracks, or with -Y as the sync piece's track piece, b.tracks keeping the
// raw pieces for the bits line.  -V (with -Y): the check records of the same entries, each with its check track (job.h: crc_take),
// in b.crcs beside b.syncs
inline int device_worker::read_tracks(size_t k, batch_result &b)
{
	std::vector<tfrec_amd_track> recs;
	std::vector<uint32_t> words;
	int r = read_run_bitmaps(tfrec_amd_read_burst_tracks, recs, words);
	if (r == TFREC_AMD_E_OVERFLOW)  // (cannot happen: the table and the pool are sized for the worst case)
		fprintf(stderr, "tfrec_amd: device %d batch %zu: more runs or pairs than the recorder holds, the track is incomplete\n", device, k);
	if (r)
		return r;
	std::vector<tfrec_amd_track_centre> crecs;
	if (job.centring()) {
		uint32_t nr = 0;
		r = tfrec_amd_read_burst_track_centres(ctx, NULL, 0, &nr);  // (the count: E_INVAL for want of room)
		if (r == TFREC_AMD_E_INVAL && nr) {
			crecs.resize(nr);
			r = tfrec_amd_read_burst_track_centres(ctx, crecs.data(), crecs.size(), &nr);
		}
		if (r)
			return r;
		if (crecs.size() != recs.size()) {
			fprintf(stderr, "tfrec_amd: device %d batch %zu: %zu centre records beside %zu track records\n", device, k, crecs.size(), recs.size());
			return TFREC_AMD_E_STATE;
		}
	}
	std::vector<tfrec_amd_burst_sync> srecs;
	std::vector<uint32_t> swords;
	if (job.syncing()) {
		if ((r = read_run_bitmaps(tfrec_amd_read_burst_syncs, srecs, swords)))
			return r;
		if (srecs.size() != recs.size()) {
			fprintf(stderr, "tfrec_amd: device %d batch %zu: %zu sync records beside %zu track records\n", device, k, srecs.size(), recs.size());
			return TFREC_AMD_E_STATE;
		}
	}
	std::vector<tfrec_amd_track> urecs;  // -U: the coded records and words of the same entries
	std::vector<uint32_t> uwords;
	if (job.coding()) {
		if ((r = read_run_bitmaps(tfrec_amd_read_burst_codes, urecs, uwords)))
			return r;
		if (urecs.size() != recs.size()) {
			fprintf(stderr, "tfrec_amd: device %d batch %zu: %zu coded records beside %zu track records\n", device, k, urecs.size(), recs.size());
			return TFREC_AMD_E_STATE;
		}
	}
	std::vector<tfrec_amd_burst_crc> vrecs;  // -V: the check records and words of the same entries
	std::vector<uint32_t> vwords;
	if (job.checking()) {
		if ((r = read_run_bitmaps(tfrec_amd_read_burst_crcs, vrecs, vwords)))
			return r;
		if (vrecs.size() != recs.size()) {
			fprintf(stderr, "tfrec_amd: device %d batch %zu: %zu check records beside %zu track records\n", device, k, vrecs.size(), recs.size());
			return TFREC_AMD_E_STATE;
		}
	}
	for (size_t q = 0; q < recs.size(); q++) {
		tfrec_amd_track x = recs[q];
		if (!cut_at_file_end(x, plan[k].file, file_blocks, true))
			continue;
		const uint32_t n = x.n_samples;  // (track_take is given the device's record and what the cut keeps of it)
		x.n_samples = recs[q].n_samples;
		track_piece t = track_take(x, words.data(), n);
		if (job.centring())
			centre_take(t, crecs[q]);
		if (job.checking())
			b.crcs.push_back(crc_take(vrecs[q], vwords.data(), t));
		if (job.coding()) {  // the coded piece: the cut entry with the coded record's n_ones and bits; the sync's frames are read from it
			x.n_ones = urecs[q].n_ones;
			track_piece u = track_take(x, uwords.data(), n);
			if (job.syncing())
				b.syncs.push_back(sync_take(srecs[q], swords.data(), u));
			else
				b.codes.push_back(std::move(u));
			b.tracks.push_back(std::move(t));
		} else if (job.syncing()) {
			b.syncs.push_back(sync_take(srecs[q], swords.data(), t));
		} else {
			b.tracks.push_back(std::move(t));
		}
	}
	return 0;
}

// -z -D, -Z -D: the last estimate of every file's row -- d, or (t, g) -- by the stage's reader
inline int device_worker::read_last_estimate(size_t k, estimate_reader reader, std::vector<int> &files, std::vector<int16_t> &last)
{
	std::vector<int16_t> e;
	int r = 0;
	for (size_t s = 0; s < n && r == 0; s++) {
		if (plan[k].file[s] < 0 || !reads[s])
			continue;
		int nw = 0;
		r = reader(ctx, in_row[s], NULL, 0, &nw);  // (the count: E_INVAL for want of room)
		if (r == TFREC_AMD_E_INVAL && nw > 0) {
			e.resize(2 * (size_t)nw);
			r = reader(ctx, in_row[s], e.data(), (size_t)nw, &nw);
			if (r == 0) {
				files.push_back(plan[k].file[s]);
				last.push_back(e[2 * (size_t)nw - 2]);
				last.push_back(e[2 * (size_t)nw - 1]);
			}
		}
	}
	return r;
}

// batch k's results: its side outputs (captures, then occupancy or spectrum, then DC, then levels), then the drain that pops it
// and frees its host buffer for the reader
inline int device_worker::collect(size_t k, batch_result &b)
{
	int r = job.capture ? read_captures(k, b) : 0;
	if (!r && job.metering())
		r = read_run_records(k, tfrec_amd_read_bursts, "burst", false, b.bursts);  // (-M alone: a cut record is not marked OPEN)
	if (!r && job.enveloping())
		r = read_run_records(k, tfrec_amd_read_burst_envelopes, "envelope", true, b.envelopes);
	if (!r && job.clocking())
		r = read_run_records(k, tfrec_amd_read_burst_clocks, "clock", true, b.clocks);
	if (!r && job.tracking())
		r = read_tracks(k, b);
	if (!r && job.occupancy()) {  // -A: the detector's records in place of the spectrum's, 16 + N / 8 bytes each
		int nr = 0;
		r = tfrec_amd_read_occupancy(ctx, 0, NULL, NULL, 0, &nr);  // (the count: E_INVAL for want of room)
		if (r == TFREC_AMD_E_INVAL && nr > 0) {
			b.occ_recs.resize((size_t)nr);
			b.occ_bits.resize((size_t)nr * (job.spec_n / 32));
			r = tfrec_amd_read_occupancy(ctx, 0, b.occ_recs.data(), b.occ_bits.data(), (size_t)nr, &nr);
		}
	} else if (!r && job.spectrum) {  // -P: the batch's spectrum records
		int nr = 0;
		r = tfrec_amd_read_spectrum(ctx, 0, NULL, NULL, 0, NULL, &nr);  // (the count: E_INVAL for want of room)
		if (r == TFREC_AMD_E_INVAL && nr > 0) {
			b.spec_sum.resize((size_t)nr * job.spec_n);
			b.spec_peak.resize((size_t)nr * job.spec_n);
			b.spec_frames.resize((size_t)nr);
			r = tfrec_amd_read_spectrum(ctx, 0, b.spec_sum.data(), b.spec_peak.data(), (size_t)nr, b.spec_frames.data(), &nr);
		}
	}
	if (!r && job.dc_windows && job.dbg > 0)
		r = read_dc(k, b);
	if (!r && job.iq_windows && job.dbg > 0)
		r = read_iq(k, b);
	if (!r && job.scan) {  // -s: the batch's level records
		int nb = 0;
		b.lv.resize(n * (size_t)bps);
		r = tfrec_amd_read_levels(ctx, b.lv.data(), b.lv.size(), &nb);
		b.lv.resize(n * (size_t)nb);
	}
	if (r)
		return r;
	b.ev.resize(max_events);
	int nev = 0;
	r = tfrec_amd_drain_events(ctx, b.ev.data(), (int)b.ev.size(), &nev);
	if (r == TFREC_AMD_E_OVERFLOW) {  // the events that fit were returned; the replay goes on (those beyond are lost)
		fprintf(stderr, "tfrec_amd: device %d batch %zu: event buffer overflow, %d events kept\n", device, k, nev);
		r = 0;
	}
	if (r)
		return r;
	{
		std::lock_guard<std::mutex> lk(rmu);
		drained = k + 1;  // batch k's host buffer may be refilled
	}
	rcv.notify_all();
	// stream -> the index of the file it carried in this batch, within the whole job (none: silence, dropped)
	const std::vector<int> &file = plan[k].file;
	int kept = 0;
	for (int q = 0; q < nev; q++)
		if (b.ev[q].stream < file.size() && file[b.ev[q].stream] >= 0) {
			b.ev[kept] = b.ev[q];
			b.ev[kept++].stream = (uint32_t)file[b.ev[q].stream];
		}
	b.ev.resize(kept);
	return 0;
}

// the end of work(), r: how the batches went -> the worker's result
inline int device_worker::close_context(int r)
{
	if (r)
		fprintf(stderr, "tfrec_amd (device %d): %s (%s)\n", device, tfrec_amd_strerror(r), tfrec_amd_last_error());
	{
		std::lock_guard<std::mutex> lk(rmu);
		drained = plan.size() + kBufs;  // let the reader run out after an error
	}
	rcv.notify_all();
	if (reader.joinable())
		reader.join();
	tfrec_amd_destroy(ctx);
	for (int b = 0; b < kBufs; b++) {
		if (pinned[b])
			tfrec_amd_host_free(host[b]);
		else
			free(host[b]);
	}
	return !r && read_failed ? TFREC_AMD_E_INVAL : r;
}

#endif
