// tfrec_amd/host/gpu_engine.cpp -- see gpu_engine.h.
#include "gpu_engine.h"

#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <thread>

// decoder.cpp:67-96: "<id> <temp> <hum> <seq> <alarm> <rssi> <flags> <ts>"; every type but WHB folds the sensor type into
// the id, WHB prints its 52-bit id (decoder.cpp:72-91)
void tfrec_handler_args(const sensordata_t &d, sensor_e dec_type, char *out, size_t n)
{
	if (dec_type != TFA_WHB)
		snprintf(out, n, "%04" PRIx64 " %+.1f %g %i %i %i %i %li", (uint64_t)(d.id | ((uint64_t)d.type << 24)), d.temp, d.humidity,
			 d.sequence, d.alarm, d.rssi, d.flags, (long)d.ts);
	else
		snprintf(out, n, "%013" PRIx64 " %+.1f %g %i %i %i %i %li", (uint64_t)d.id, d.temp, d.humidity, d.sequence, d.alarm,
			 d.rssi, d.flags, (long)d.ts);
}

gpu_engine::gpu_engine(const std::vector<std::string> &dumpfiles, int _types, int _thresh, int _filter, int _dbg,
		       const std::vector<int> &_devices, int blocks_per_submit, const std::vector<file_settings> &per_file)
	: files(dumpfiles), settings(per_file), types(_types), thresh(_thresh), filter(_filter), dbg(_dbg), bps(blocks_per_submit),
	  devices(_devices), n_telegrams(0), sink(NULL), psink(NULL), out_mode(0), bits_replay(false), slots(0), wide(false), rate_p(1), rate_q(1), unit(1), fmt(TFREC_AMD_FMT_U8)
{
	if (devices.empty())
		devices.push_back(0);
	if (settings.size() != files.size())
		settings.assign(files.size(), file_settings{ types, thresh, filter, 0 });
	// one set of protocol handlers per stream, registered like main.cpp:173-218 (with the file's own -T)
	for (size_t s = 0; s < files.size(); s++) {
		const int types = settings[s].types;
		std::vector<decoder *> d(TFREC_AMD_NSLOTS, (decoder *)NULL);
		if (types & (1 << TFA_1)) d[TFREC_AMD_SLOT_TFA1] = new sinked_decoder<tfa1_decoder>(TFA_1, &sink, (int)s);
		if (types & (1 << TFA_2)) d[TFREC_AMD_SLOT_TFA2] = new sinked_decoder<tfa2_decoder>(TFA_2, &sink, (int)s);
		if (types & (1 << TFA_3)) d[TFREC_AMD_SLOT_TFA3] = new sinked_decoder<tfa2_decoder>(TFA_3, &sink, (int)s);
		if (types & (1 << TX22)) d[TFREC_AMD_SLOT_TX22] = new sinked_decoder<tfa2_decoder>(TX22, &sink, (int)s);
		if (types & (1 << TFA_WHB)) d[TFREC_AMD_SLOT_WHB] = new sinked_decoder<whb_decoder>(TFA_WHB, &sink, (int)s);
		for (size_t k = 0; k < d.size(); k++)
			if (d[k])
				d[k]->set_params(NULL, 0, dbg);
		decs.push_back(d);
	}
}

pipe_sink::pipe_sink(const char *command) : pipe(popen(command, "w")), n_records(0)
{
	if (!pipe)
		perror(command);
}

pipe_sink::~pipe_sink()
{
	flush();
	if (pipe)
		pclose(pipe);
}

void pipe_sink::put(int stream, const char *args)
{
	char head[32];
	snprintf(head, sizeof(head), "%d ", stream);
	pending += head;
	pending += args;
	pending += '\n';
	n_records++;
}

void pipe_sink::flush()
{
	if (pipe && !pending.empty()) {
		fwrite(pending.data(), 1, pending.size(), pipe);
		fflush(pipe);
	}
	pending.clear();
}

// floor(a / b) for b > 0
static long long floor_div(long long a, long long b) { return a / b - (a % b < 0 ? 1 : 0); }

std::vector<occ_channel> occupancy_channels(const std::vector<unsigned long long> &hits, unsigned long long records, int n_bins, long fs_in,
					    long center_khz, long join_hz)
{
	struct item {
		long long pos;  // twice the middle bin: the order of the list
		occ_channel c;
	};
	std::vector<item> items;
	int group = -1;  // index of the open group in items
	for (int b = -n_bins / 2; b < n_bins / 2; b++) {
		const unsigned long long h = hits[(size_t)(b < 0 ? b + n_bins : b)];
		if (h < 1)
			continue;
		if (2 * h > records) {  // continuous, like a receiver's DC spike: listed, never scanned, and no part of a group
			const long off = (long)floor_div(2LL * b * fs_in + 1000LL * n_bins, 2000LL * n_bins);
			items.push_back(item{ 2LL * b, occ_channel{ true, center_khz + off, b, b, h, false } });
			continue;
		}
		if (group >= 0 && (long long)(b - items[group].c.hi - 1) * fs_in <= (long long)join_hz * n_bins) {
			items[group].c.hi = b;
			items[group].c.hits = std::max(items[group].c.hits, h);
			continue;
		}
		group = (int)items.size();
		items.push_back(item{ 0, occ_channel{ false, 0, b, b, h, false } });
	}
	for (item &it : items) {
		if (it.c.carrier)
			continue;
		const long off = (long)floor_div((long long)(it.c.lo + it.c.hi) * fs_in + 1000LL * n_bins, 2000LL * n_bins);
		it.pos = it.c.lo + it.c.hi;
		it.c.khz = center_khz + off;
		it.c.in_range = 2000LL * (off < 0 ? -off : off) <= (long long)fs_in - 384000;
	}
	std::stable_sort(items.begin(), items.end(), [](const item &a, const item &b) { return a.pos < b.pos; });
	std::vector<occ_channel> out;
	for (const item &it : items)
		out.push_back(it.c);
	return out;
}

void gpu_engine::set_rate(int p, int q)
{
	rate_p = p;
	rate_q = q;
	unit = q;
	while (unit % 2 == 0)
		unit /= 2;
}

void gpu_engine::set_handler(const char *exec, bool batched, int mode)
{
	out_mode = mode;
	if (batched && exec && *exec)
		sink = psink = new pipe_sink(exec);
	for (size_t s = 0; s < decs.size(); s++)
		for (size_t k = 0; k < decs[s].size(); k++)
			if (decs[s][k])
				decs[s][k]->set_params(batched ? NULL : (char *)exec, mode, dbg);
}

gpu_engine::~gpu_engine()
{
	delete psink;
	// (the reference's decoder has no virtual destructor -- main.cpp never frees its plugins either)
}

// The adapter contract: bring the decoder's rdata[0..64) to the state the GPU decoder had,
// set byte_cnt, then let the unchanged handler do CRC, parsing, printing, store_data.
// BITS mode: the decoder receives every bit through its own store_bit (decoder.h:39) -- it then holds rdata / byte_cnt
// by itself, and whatever store_bit prints appears as in the reference -- and every flush, without store_bytes.
void gpu_engine::replay(const tfrec_amd_event &ev)
{
	decoder *dec = decs[ev.stream][ev.slot];
	if (!dec)
		return;
	if (ev.status == TFREC_AMD_STATUS_BITS) {
		for (int k = 0; k < (int)ev.byte_cnt && k < 512; k++)
			dec->store_bit((ev.rdata[k >> 3] >> (k & 7)) & 1);
		return;
	}
	if (!bits_replay) {
		uint8_t buf[256];
		memset(buf, 0, sizeof(buf));
		memcpy(buf, ev.rdata, 64);
		dec->store_bytes(buf, 64);
		int len = ev.byte_cnt > 256 ? 256 : ev.byte_cnt;
		dec->store_bytes(buf, len);
	}
	dec->flush(tfrec_amd_rssi_db(ev.slot, ev.rssi_raw), ev.offset);
	if (ev.status == 1)
		n_telegrams++;
}

namespace {

// One batch of a device context: the blocks every stream gets, the dump file each stream (slot) reads (-1: none, silence),
// the streams reset before it is submitted (their previous file ended in the batch before), and the streams configured
// or tuned before it (their next file's settings or tune differ from the stream's current ones: a configure or a tune is a
// reset with new settings)
struct batch_plan {
	int nb;
	std::vector<int> file;
	std::vector<int32_t> reset;
	std::vector<int32_t> conf;
	std::vector<tfrec_amd_stream_config> conf_cfg;
	std::vector<int32_t> tune;
	std::vector<int32_t> tune_hz;
};

// The batches that push the files [s0, s1) through nslots streams of bps blocks (file_blocks: blocks of every file of the job).
// Files take free streams in order; a file's last batch may be partial (padded with silence, its events cut by the engine).
// A batch has bps blocks unless no stream needs that many.  With one stream per file this is the plan of a run without -n:
// every file starts in the first batch and no stream is ever reset.
// settings: every file's; dflt: the context's.
std::vector<batch_plan> plan_batches(const std::vector<size_t> &file_blocks, const std::vector<file_settings> &settings,
				     const file_settings &dflt, size_t s0, size_t s1, size_t nslots, int bps)
{
	std::vector<batch_plan> plan;
	std::vector<file_settings> has(nslots, dflt);  // the settings each stream runs with
	std::vector<int> cur(nslots, -1);
	std::vector<size_t> left(nslots, 0);    // blocks of the stream's file still to submit
	std::vector<bool> used(nslots, false);  // the stream has carried a file: reset it before the next one
	size_t next = s0;
	for (;;) {
		batch_plan b;
		for (size_t j = 0; j < nslots; j++) {
			while (cur[j] < 0 && next < s1) {
				const size_t f = next++;
				if (file_blocks[f] == 0)
					continue;  // (no block, no event)
				cur[j] = (int)f;
				left[j] = file_blocks[f];
				if (settings[f] != has[j]) {
					if (!settings[f].same_config(has[j])) {
						b.conf.push_back((int32_t)j);
						b.conf_cfg.push_back(tfrec_amd_stream_config{ settings[f].types, settings[f].thresh, settings[f].filter, 0 });
					}
					if (settings[f].tune != has[j].tune) {
						b.tune.push_back((int32_t)j);
						b.tune_hz.push_back(settings[f].tune);
					}
					has[j] = settings[f];
				} else if (used[j]) {
					b.reset.push_back((int32_t)j);
				}
				used[j] = true;
			}
		}
		size_t most = 0;
		for (size_t j = 0; j < nslots; j++)
			if (cur[j] >= 0)
				most = std::max(most, left[j]);
		if (most == 0)
			break;
		b.nb = (int)std::min<size_t>((size_t)bps, most);
		b.file = cur;
		for (size_t j = 0; j < nslots; j++)
			if (cur[j] >= 0) {
				left[j] -= std::min<size_t>(left[j], (size_t)b.nb);
				if (left[j] == 0)
					cur[j] = -1;
			}
		plan.push_back(std::move(b));
	}
	return plan;
}

// engine::run (engine.cpp:63-93) for the dump files [s0, s1) on ONE device, as a three-stage pipeline over batches of
// bps blocks:
//   reader thread : fread batch k+2 of every file into a pinned host buffer (three buffers in rotation)
//   GPU           : H2D copy + hot path of batch k+1 (tfrec_amd_submit_host is asynchronous on pinned memory)
//   worker thread : drain batch k's flush events and queue them for the engine's thread
// The C ABI's submit/drain FIFO (depth TFREC_AMD_FIFO_DEPTH = 4) is what lets batches k+1 .. k+3 be queued before batch
// k is drained; this loop keeps the FIFO full (one pinned host buffer per submit in flight + one being read).
// -S: the captures of one batch of one device: the runs that belong to a file (file[i]: its index in the job), cut at the file's
// end, and the batch's sample pool, which their pool_offset indexes
// -P travels with it: the batch's spectrum records of input row 0, [record][bin], and their frame counts
struct capture_batch {
	std::vector<tfrec_amd_run> runs;
	std::vector<int> file;
	std::vector<int16_t> pool;
	std::vector<uint64_t> spec_sum, spec_peak;
	std::vector<uint32_t> spec_frames;
	std::vector<tfrec_amd_occupancy> occ_recs;  // -A: the detector's records of row 0 and their bitmap words, [record][N / 32]
	std::vector<uint32_t> occ_bits;
	std::vector<int> dc_file;  // -z with -D: per file of the batch its index in the job and the last window's {d_I, d_Q} of its row
	std::vector<int16_t> dc_last;
};

struct device_worker {
	const std::vector<std::string> *files;
	size_t s0, s1;
	int device, types, thresh, filter, bps;
	uint32_t flags;     // TFREC_AMD_F_* of the context
	size_t nslots;      // streams of the context
	const std::vector<size_t> *file_blocks;  // blocks of every file of the job
	std::vector<batch_plan> plan;             // plan_batches
	bool wide;          // -x: 15.36 MS/s dumps (TFREC_AMD_F_INPUT_10X in flags), the files' tunes are wide tunes
	bool share;         // one stream per file for the whole job (no -n): a path given several times is read once, into one row
	int rate_p, rate_q;  // -r: the input rate as p / q of 1.536 MS/s (1 / 1: none)
	int fmt;             // -F: TFREC_AMD_FMT_* of the files (U8: none)
	size_t block_bytes;  // bytes of one block of a file: 65536 p / q (x `unit` blocks when q does not divide it), 655360 with -x
	int unit;            // blocks a block_bytes piece holds: every batch carries a multiple of it
	int rc;
	std::atomic<bool> *abort;  // set by the engine when any worker failed: stop instead of running the whole job
	std::mutex mu;
	std::condition_variable cv;
	std::deque<std::vector<tfrec_amd_event> > out;  // batches drained, oldest first
	std::deque<std::vector<tfrec_amd_level> > out_levels;  // -s: their level records, [stream][the batch's blocks]
	bool capture;  // -S: the contexts record (tfrec_amd_enable_capture)
	int spec_n, spec_g;  // -P: bins and frames per record of the spectrum of row 0 (tfrec_amd_enable_spectrum); 0: none
	int occ_ratio, occ_rel;  // -A: the occupancy detector on it (tfrec_amd_enable_occupancy); 0: none
	int dc_windows;     // -z: the DC blocker's avg_windows (tfrec_amd_create_dc); 0: none
	bool dc_report;     // ... with -D: the batches carry every file's last estimate
	std::deque<capture_batch> out_caps;  // -S: their runs (stream = the file's index in the job) and sample pool
	bool done;
	std::thread th;

	device_worker() : files(NULL), s0(0), s1(0), device(0), types(0), thresh(0), filter(0), bps(1), flags(0), nslots(0), file_blocks(NULL), wide(false), share(false), rate_p(1), rate_q(1), fmt(TFREC_AMD_FMT_U8), block_bytes(TFREC_AMD_BLOCK_BYTES), unit(1), rc(0), abort(NULL), capture(false), spec_n(0), spec_g(0), occ_ratio(0), occ_rel(0), dc_windows(0), dc_report(false), done(false) {}

	void push(std::vector<tfrec_amd_event> &&ev, std::vector<tfrec_amd_level> &&lv, capture_batch &&cb)
	{
		{
			std::unique_lock<std::mutex> lk(mu);
			cv.wait(lk, [&]() { return out.size() < 2; });  // the engine's thread is at most two batches behind
			out.push_back(std::move(ev));
			out_levels.push_back(std::move(lv));
			out_caps.push_back(std::move(cb));
		}
		cv.notify_all();
	}
	// next batch's events and (-s) level records (false: the worker ended -- rc says why)
	bool pop(std::vector<tfrec_amd_event> &ev, std::vector<tfrec_amd_level> &lv, capture_batch &cb)
	{
		std::unique_lock<std::mutex> lk(mu);
		cv.wait(lk, [&]() { return !out.empty() || done; });
		if (out.empty())
			return false;
		ev = std::move(out.front());
		out.pop_front();
		lv = std::move(out_levels.front());
		out_levels.pop_front();
		cb = std::move(out_caps.front());
		out_caps.pop_front();
		lk.unlock();
		cv.notify_all();
		return true;
	}

	void run()
	{
		rc = work();
		{
			std::lock_guard<std::mutex> lk(mu);
			done = true;
		}
		cv.notify_all();
	}

	int work()
	{
		const size_t n = nslots;
		// a file is opened when its first batch is read and closed after its last one (a queue of thousands of files)
		std::vector<FILE *> fd(s1 - s0, (FILE *)NULL);
		std::vector<size_t> fleft(s1 - s0);
		for (size_t f = s0; f < s1; f++)
			fleft[f - s0] = (*file_blocks)[f];
		bool read_failed = false;
		tfrec_amd_config cfg;
		memset(&cfg, 0, sizeof(cfg));
		cfg.n_streams = (int32_t)n;
		cfg.types_mask = types;
		cfg.thresh = thresh;
		cfg.filter_type = filter;
		cfg.device = device;
		cfg.max_blocks = bps;
		// (BITS mode: every flush + a chunk per 512 bits, a slicer emits < 0.5 bit per decimated sample)
		cfg.max_events = (int32_t)std::max<size_t>(4096, n * (size_t)bps * ((flags & TFREC_AMD_F_BITS) ? 256 : 64));
		cfg.flags = flags;
		tfrec_amd_ctx *ctx = NULL;
		const size_t row = (size_t)(bps / unit) * block_bytes;
		const size_t n_batches = plan.size();
		// Shared inputs (tfrec_amd_map_streams): without -n a stream carries one file for the whole job, and the streams whose
		// files are one path share that path's input row -- the file is opened and read once, staged and copied once.  Decoders,
		// stream indices and the order of the output stay per -L occurrence.  (A stream without a file reads row 0; its events
		// are dropped.)
		std::vector<int32_t> in_row(n, 0);
		std::vector<bool> reads(n, true);  // the stream's file is read into its row (the first stream of the row)
		size_t n_rows = n;
		bool map = false;  // streams share rows: the context's streams are mapped to them
		if (share && n_batches) {
			std::vector<std::string> paths;
			for (size_t s = 0; s < n; s++) {
				const int f = plan[0].file[s];
				if (f < 0)
					continue;
				const size_t r = std::find(paths.begin(), paths.end(), (*files)[f]) - paths.begin();
				reads[s] = r == paths.size();
				if (reads[s])
					paths.push_back((*files)[f]);
				in_row[s] = (int32_t)r;
			}
			if (paths.size() < n) {
				map = true;
				n_rows = std::max<size_t>(1, paths.size());
			} else {
				for (size_t s = 0; s < n; s++)
					in_row[s] = (int32_t)s;
			}
		} else {
			for (size_t s = 0; s < n; s++)
				in_row[s] = (int32_t)s;
		}
		// (the rows are known: -z sizes the blocker for them)
		int r = dc_windows		       ? tfrec_amd_create_dc(&cfg, fmt, rate_p, rate_q, dc_windows, (int32_t)n_rows, &ctx)
			: fmt != TFREC_AMD_FMT_U8      ? tfrec_amd_create_format(&cfg, fmt, rate_p, rate_q, &ctx)
			: (rate_p != 1 || rate_q != 1) ? tfrec_amd_create_rate(&cfg, rate_p, rate_q, &ctx)
						       : tfrec_amd_create(&cfg, &ctx);
		if (r) {
			fprintf(stderr, "tfrec_amd_create (device %d): %s (%s)\n", device, tfrec_amd_strerror(r), tfrec_amd_last_error());
			return r;
		}
		if (map) {
			std::vector<int32_t> all(n);
			for (size_t s = 0; s < n; s++)
				all[s] = (int32_t)s;
			r = tfrec_amd_map_streams(ctx, all.data(), in_row.data(), (int)n);
			if (r) {
				fprintf(stderr, "tfrec_amd_map_streams (device %d): %s (%s)\n", device, tfrec_amd_strerror(r), tfrec_amd_last_error());
				tfrec_amd_destroy(ctx);
				return r;
			}
		}
		if (capture) {  // -S, sized so that no submit overflows: every sample, and a stream's runs are >= 356 samples long but two
			r = tfrec_amd_enable_capture(ctx, (uint32_t)(n * ((size_t)bps * TFREC_AMD_BLOCK_DEC / 356 + 3)),
						     (uint64_t)n * (uint64_t)bps * TFREC_AMD_BLOCK_DEC);
			if (r) {
				fprintf(stderr, "tfrec_amd_enable_capture (device %d): %s (%s)\n", device, tfrec_amd_strerror(r), tfrec_amd_last_error());
				tfrec_amd_destroy(ctx);
				return r;
			}
		}
		if (spec_n) {  // -P: the one file's row
			r = tfrec_amd_enable_spectrum(ctx, spec_n, spec_g, 1);
			if (r) {
				fprintf(stderr, "tfrec_amd_enable_spectrum (device %d): %s (%s)\n", device, tfrec_amd_strerror(r), tfrec_amd_last_error());
				tfrec_amd_destroy(ctx);
				return r;
			}
		}
		if (spec_n && occ_ratio) {  // -A: the detector on its records
			r = tfrec_amd_enable_occupancy(ctx, (uint32_t)occ_ratio, (uint32_t)occ_rel);
			if (r) {
				fprintf(stderr, "tfrec_amd_enable_occupancy (device %d): %s (%s)\n", device, tfrec_amd_strerror(r), tfrec_amd_last_error());
				tfrec_amd_destroy(ctx);
				return r;
			}
		}
		const int depth = std::max(1, std::min(tfrec_amd_fifo_depth(), TFREC_AMD_FIFO_DEPTH));
		constexpr int kBufs = TFREC_AMD_FIFO_DEPTH + 1;
		uint8_t *host[kBufs];
		bool pinned[kBufs];  // per buffer: each is released by the allocator it came from
		for (int b = 0; b < kBufs; b++) {
			host[b] = (uint8_t *)tfrec_amd_host_alloc(n_rows * row);
			pinned[b] = host[b] != NULL;
			if (!host[b])  // no page-locked memory: this buffer's copies become synchronous, results are the same
				host[b] = (uint8_t *)malloc(n_rows * row);
		}
		// ---- reader thread: batch k goes to host[k % kBufs]; it may run at most kBufs batches ahead of the drain
		std::mutex rmu;
		std::condition_variable rcv;
		size_t filled = 0, drained = 0;  // batches read / batches whose buffer is free again
		std::thread reader([&]() {
			for (size_t k = 0; k < n_batches; k++) {
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
					const size_t want = (size_t)(b.nb / unit) * block_bytes;
					const int f = b.file[s];
					size_t got = 0;
					if (f >= 0) {
						FILE *&fp = fd[f - s0];
						if (!fp && !read_failed && !(fp = fopen((*files)[f].c_str(), "rb"))) {
							perror((*files)[f].c_str());
							read_failed = true;
						}
						if (fp) {
							got = fread(dst, 1, want, fp);
							got -= got % block_bytes;
							size_t &left = fleft[f - s0];
							left -= std::min<size_t>(left, (size_t)b.nb);
							if (left == 0) {
								fclose(fp);
								fp = NULL;
							}
						}
					}
					// a shorter file is padded with silence (its events are cut by the engine): u8 128, zero in every other format
					memset(dst + got, fmt != TFREC_AMD_FMT_U8 ? 0 : 0x80, want - got);
				}
				{
					std::lock_guard<std::mutex> lk(rmu);
					filled = k + 1;
				}
				rcv.notify_all();
			}
		});
		std::vector<bool> in_tune(n, false), narrow_tune(n, false);  // -r: the stream has an input-rate tune / a tune behind the resampler
		auto submit = [&](size_t k) -> int {
			{
				std::unique_lock<std::mutex> lk(rmu);
				rcv.wait(lk, [&]() { return filled > k; });
			}
			const batch_plan &b = plan[k];
			if (dc_windows && !share) {
				// -n with -z: a slot that starts a new file -- by a reset, or by the configure or tune its next file needs -- starts a new
				// DC estimate too.  A stream's row is its own here (nothing is shared); duplicates are allowed.
				std::vector<int32_t> rows(b.reset);
				rows.insert(rows.end(), b.conf.begin(), b.conf.end());
				rows.insert(rows.end(), b.tune.begin(), b.tune.end());
				const int rd = tfrec_amd_reset_dc_rows(ctx, rows.data(), (int)rows.size());
				if (rd)
					return rd;
			}
			if (!b.reset.empty()) {  // the streams whose file ended in the batch before: fresh receivers for the next files
				const int rr = tfrec_amd_reset_streams(ctx, b.reset.data(), (int)b.reset.size());
				if (rr)
					return rr;
			}
			if (!b.conf.empty()) {  // ... with the settings of their next file
				const int rr = tfrec_amd_configure_streams(ctx, b.conf.data(), b.conf_cfg.data(), (int)b.conf.size());
				if (rr)
					return rr;
			}
			if (!b.tune.empty() && (rate_p != 1 || rate_q != 1)) {
				// ... and tunes, -r: an offset within +-767 kHz is a tune behind the resampler, as it always was; a larger one is
				// the input-rate tune ahead of it (tfrec_amd_tune_streams_input).  A stream that goes from one kind to the other
				// (-n) has the other kind cleared; all of it is one restart.
				std::vector<int32_t> ns, nhz, is, ihz;
				for (size_t i = 0; i < b.tune.size(); i++) {
					const int32_t s = b.tune[i], hz = b.tune_hz[i];
					const bool far = hz <= -768000 || hz >= 768000;
					if (far || in_tune[s]) {
						is.push_back(s);
						ihz.push_back(far ? hz : 0);
						in_tune[s] = far;
					}
					if (!far || narrow_tune[s]) {
						ns.push_back(s);
						nhz.push_back(far ? 0 : hz);
						narrow_tune[s] = !far && hz != 0;
					}
				}
				int rr = ns.empty() ? 0 : tfrec_amd_tune_streams(ctx, ns.data(), nhz.data(), (int)ns.size());
				if (!rr && !is.empty())
					rr = tfrec_amd_tune_streams_input(ctx, is.data(), ihz.data(), (int)is.size());
				if (rr)
					return rr;
			} else if (!b.tune.empty()) {  // ... and tunes
				const int rr = wide ? tfrec_amd_tune_streams_wide(ctx, b.tune.data(), b.tune_hz.data(), (int)b.tune.size())
						    : tfrec_amd_tune_streams(ctx, b.tune.data(), b.tune_hz.data(), (int)b.tune.size());
				if (rr)
					return rr;
			}
			return tfrec_amd_submit_host(ctx, host[k % kBufs], row, b.nb);
		};
		size_t queued = 0;
		for (size_t k = 0; k < n_batches && r == 0; k++) {
			while (queued < n_batches && queued < k + (size_t)depth && r == 0)
				r = submit(queued++);
			if (r)
				break;
			if (abort && abort->load()) {
				r = TFREC_AMD_E_STATE;
				break;
			}
			capture_batch cb;
			if (capture) {  // -S: the batch's captures, then its levels, then the drain that pops it
				uint32_t nr = 0;
				uint64_t np = 0;
				r = tfrec_amd_read_captures(ctx, NULL, 0, &nr, NULL, 0, &np);  // (the counts: E_INVAL for want of room)
				if (r == TFREC_AMD_E_INVAL && nr) {
					cb.runs.resize((size_t)nr + 1);
					cb.pool.resize(2 * (size_t)np + 2);
					r = tfrec_amd_read_captures(ctx, cb.runs.data(), cb.runs.size(), &nr, cb.pool.data(), cb.pool.size() / 2, &np);
				}
				size_t have = nr;
				if (r == TFREC_AMD_E_OVERFLOW) {  // the runs that fitted were returned (n_samples == 0 ends them); the job goes on
					for (have = 0; have < cb.runs.size() && cb.runs[have].n_samples; have++) {
					}
					fprintf(stderr, "tfrec_amd: device %d batch %zu: capture overflow, %zu of %u runs kept\n", device, k, have, (unsigned)nr);
					r = 0;
				}
				if (r)
					break;
				// stream -> file, as for the events below; a run is cut at its file's end
				const std::vector<int> &file = plan[k].file;
				size_t kept = 0;
				for (size_t q = 0; q < have; q++) {
					tfrec_amd_run x = cb.runs[q];
					if (x.stream >= file.size() || file[x.stream] < 0)
						continue;
					const long long end = (long long)(*file_blocks)[file[x.stream]] * TFREC_AMD_BLOCK_DEC;
					if (x.start_sample >= end)
						continue;
					x.n_samples = (uint32_t)std::min<long long>(x.n_samples, end - x.start_sample);
					cb.file.push_back(file[x.stream]);
					cb.runs[kept++] = x;
				}
				cb.runs.resize(kept);
			}
			if (spec_n && occ_ratio) {  // -A: the detector's records in place of the spectrum's, 16 + N / 8 bytes each
				int nr = 0;
				r = tfrec_amd_read_occupancy(ctx, 0, NULL, NULL, 0, &nr);  // (the count: E_INVAL for want of room)
				if (r == TFREC_AMD_E_INVAL && nr > 0) {
					cb.occ_recs.resize((size_t)nr);
					cb.occ_bits.resize((size_t)nr * (spec_n / 32));
					r = tfrec_amd_read_occupancy(ctx, 0, cb.occ_recs.data(), cb.occ_bits.data(), (size_t)nr, &nr);
				}
				if (r)
					break;
			} else if (spec_n) {  // -P: the batch's spectrum records, before the drain pops it
				int nr = 0;
				r = tfrec_amd_read_spectrum(ctx, 0, NULL, NULL, 0, NULL, &nr);  // (the count: E_INVAL for want of room)
				if (r == TFREC_AMD_E_INVAL && nr > 0) {
					cb.spec_sum.resize((size_t)nr * spec_n);
					cb.spec_peak.resize((size_t)nr * spec_n);
					cb.spec_frames.resize((size_t)nr);
					r = tfrec_amd_read_spectrum(ctx, 0, cb.spec_sum.data(), cb.spec_peak.data(), (size_t)nr, cb.spec_frames.data(), &nr);
				}
				if (r)
					break;
			}
			if (dc_windows && dc_report) {  // -z -D: the last estimate of every file's row, before the drain pops the batch
				std::vector<int16_t> d;
				for (size_t s = 0; s < n && r == 0; s++) {
					if (plan[k].file[s] < 0 || !reads[s])
						continue;
					int nw = 0;
					r = tfrec_amd_read_dc(ctx, in_row[s], NULL, 0, &nw);  // (the count: E_INVAL for want of room)
					if (r == TFREC_AMD_E_INVAL && nw > 0) {
						d.resize(2 * (size_t)nw);
						r = tfrec_amd_read_dc(ctx, in_row[s], d.data(), (size_t)nw, &nw);
						if (r == 0) {
							cb.dc_file.push_back(plan[k].file[s]);
							cb.dc_last.push_back(d[2 * (size_t)nw - 2]);
							cb.dc_last.push_back(d[2 * (size_t)nw - 1]);
						}
					}
				}
				if (r)
					break;
			}
			std::vector<tfrec_amd_level> lv;
			if (flags & TFREC_AMD_F_LEVELS) {  // -s: the batch's level records, before the drain pops it
				int nb = 0;
				lv.resize(n * (size_t)bps);
				r = tfrec_amd_read_levels(ctx, lv.data(), lv.size(), &nb);
				if (r)
					break;
				lv.resize(n * (size_t)nb);
			}
			std::vector<tfrec_amd_event> ev(cfg.max_events);
			int nev = 0;
			r = tfrec_amd_drain_events(ctx, ev.data(), (int)ev.size(), &nev);
			if (r == TFREC_AMD_E_OVERFLOW) {  // the events that fit were returned; the replay goes on (those beyond are lost)
				fprintf(stderr, "tfrec_amd: device %d batch %zu: event buffer overflow, %d events kept\n", device, k, nev);
				r = 0;
			}
			if (r)
				break;
			{
				std::lock_guard<std::mutex> lk(rmu);
				drained = k + 1;  // batch k's host buffer may be refilled
			}
			rcv.notify_all();
			// stream -> the index of the file it carried in this batch, within the whole job (none: silence, dropped)
			const std::vector<int> &file = plan[k].file;
			int kept = 0;
			for (int q = 0; q < nev; q++)
				if (ev[q].stream < file.size() && file[ev[q].stream] >= 0) {
					ev[kept] = ev[q];
					ev[kept++].stream = (uint32_t)file[ev[q].stream];
				}
			ev.resize(kept);
			push(std::move(ev), std::move(lv), std::move(cb));
		}
		if (r)
			fprintf(stderr, "tfrec_amd (device %d): %s (%s)\n", device, tfrec_amd_strerror(r), tfrec_amd_last_error());
		{
			std::lock_guard<std::mutex> lk(rmu);
			drained = n_batches + kBufs;  // let the reader run out after an error
		}
		rcv.notify_all();
		reader.join();
		tfrec_amd_destroy(ctx);
		for (int b = 0; b < kBufs; b++) {
			if (pinned[b])
				tfrec_amd_host_free(host[b]);
			else
				free(host[b]);
		}
		for (FILE *fp : fd)
			if (fp)
				fclose(fp);
		if (!r && read_failed)
			r = TFREC_AMD_E_INVAL;
		return r;
	}
};

}  // namespace

// One worker (host thread + context + HIP streams) per device entry, streams sharded by index over them; this thread
// takes the devices' events batch by batch, in device = stream order, and replays them into the decoders: stdout and
// the handler records come out in the order of a single-device run whatever the number of devices.
int gpu_engine::run()
{
	const size_t n = files.size();
	std::vector<size_t> file_blocks(n, 0);
	stream_samples.assign(n, 0);
	// bytes of a piece of `unit` blocks of a file (unit = 1 without -r): 65536 p / q x unit is a whole number
	// (q is unit times a power of two <= 64); -F: times the format's bytes per complex sample / 2
	const size_t sample_bytes = fmt == TFREC_AMD_FMT_F32 ? 8 : fmt == TFREC_AMD_FMT_S16 ? 4 : 2;
	const size_t block_bytes =
		wide ? (size_t)TFREC_AMD_BLOCK_BYTES_10X : (size_t)TFREC_AMD_BLOCK_BYTES * rate_p * unit / rate_q * sample_bytes / 2;
	for (size_t s = 0; s < n; s++) {
		FILE *f = fopen(files[s].c_str(), "rb");
		if (!f) {
			perror(files[s].c_str());
			return TFREC_AMD_E_INVAL;
		}
		fseek(f, 0, SEEK_END);
		// trailing partial block dropped, engine.cpp:72-76 (-r: a trailing partial piece of `unit` blocks)
		const size_t blocks = (size_t)ftell(f) / block_bytes * (size_t)unit;
		fclose(f);
		if (dbg > 0 && fmt != TFREC_AMD_FMT_U8)  // -D with -F: how the file is cut
			fprintf(stderr, "%s: %zu blocks, %zu bytes per %d\n", files[s].c_str(), blocks, block_bytes, unit);
		stream_samples[s] = (long long)blocks * TFREC_AMD_BLOCK_DEC;
		file_blocks[s] = blocks;
	}
	const long fs_in = wide ? 15360000L : 1536000L * rate_p / rate_q;
	// -P: bin k lies at center + (k < N/2 ? k : k - N) fs_in / N; listed (and printed) in ascending frequency
	std::vector<double> spec_khz(spectrum ? spec_n : 0);
	std::vector<int> spec_order(spectrum ? spec_n : 0);
	if (spectrum) {
		fprintf(stderr, "spec: %d bins, %d frames per record, input rate %ld S/s\n", spec_n, spec_g, fs_in);
		for (int i = 0; i < spec_n; i++) {
			const int k = (i + spec_n / 2) % spec_n;
			spec_order[i] = k;
			spec_khz[k] = spec_center + (double)((long)(k < spec_n / 2 ? k : k - spec_n) * fs_in) / spec_n / 1000.0;
			fprintf(stderr, "spec bin %.3f kHz\n", spec_khz[k]);
		}
	}
	const bool occ = spectrum && occ_ratio;  // -A, pass 1
	if (occ)
		fprintf(stderr, "occ: ratio %d, rel %d, join %ld Hz\n", occ_ratio, occ_rel, occ_join);
	if (scan) {  // -s: the channel list, before a device is opened
		fprintf(stderr, "scan: %zu channels, input rate %ld S/s\n", n, fs_in);
		for (size_t s = 0; s < n; s++) {
			const int hz = settings[s].tune;
			const bool far = !wide && (hz <= -768000 || hz >= 768000);
			fprintf(stderr, "scan channel %ld kHz: tune %d Hz %s\n", scan_khz[s], hz,
				hz == 0 ? "(none)" : wide ? "ahead of the 10:1 stage" : far ? "ahead of the resampler" : (rate_p != 1 || rate_q != 1) ? "behind the resampler" : "in the front end");
		}
	}
	size_t n_batches = 0;  // of the device with the most
	const size_t nd = std::min(devices.size(), n);  // never more workers than streams
	bps = (bps + unit - 1) / unit * unit;
	std::vector<device_worker> workers(nd);
	for (size_t d = 0; d < nd; d++) {
		device_worker &w = workers[d];
		const size_t base = n / nd, rem = n % nd;  // contiguous ranges, as evenly as possible (tfrec_amd/shard.py)
		w.s0 = d * base + std::min(d, rem);
		w.s1 = w.s0 + base + (d < rem ? 1 : 0);
		w.files = &files;
		w.device = devices[d];
		w.types = 0;  // the union of the device's files' types
		for (size_t s = w.s0; s < w.s1; s++)
			w.types |= settings[s].types;
		w.thresh = thresh;
		w.filter = filter;
		w.bps = bps;
		w.flags = (bits_replay ? (TFREC_AMD_F_BITS | TFREC_AMD_F_ALL_FLUSHES) : 0u) | (wide ? TFREC_AMD_F_INPUT_10X : 0u) |
			  (scan ? TFREC_AMD_F_LEVELS : 0u);
		w.capture = capture;
		w.spec_n = spectrum ? spec_n : 0;
		w.spec_g = spec_g;
		w.occ_ratio = spectrum ? occ_ratio : 0;
		w.occ_rel = occ_rel;
		w.dc_windows = dc_windows;
		w.dc_report = dbg > 0;
		w.wide = wide;
		w.share = slots <= 0;
		w.rate_p = rate_p;
		w.rate_q = rate_q;
		w.fmt = fmt;
		w.block_bytes = block_bytes;
		w.unit = unit;
		w.nslots = w.s1 - w.s0;
		if (slots > 0)
			w.nslots = std::min(w.nslots, (size_t)slots);
		w.file_blocks = &file_blocks;
		w.plan = plan_batches(file_blocks, settings, file_settings{ w.types, thresh, filter, 0 }, w.s0, w.s1, w.nslots, bps);
		n_batches = std::max(n_batches, w.plan.size());
	}
	std::atomic<bool> abort(false);
	for (size_t d = 0; d < nd; d++) {
		workers[d].abort = &abort;
		workers[d].th = std::thread([&workers, d]() { workers[d].run(); });
	}
	int rc = 0;
	std::vector<tfrec_amd_event> ev;
	std::vector<tfrec_amd_level> lv;
	capture_batch cb;
	FILE *cap_idx = NULL;  // -S: <prefix>.idx, and which files' <prefix>.<file>.cs16 exist already
	std::vector<bool> cap_made(capture ? n : 0, false);
	if (capture && !(cap_idx = fopen((cap_prefix + ".idx").c_str(), "w"))) {
		perror((cap_prefix + ".idx").c_str());
		return TFREC_AMD_E_INVAL;
	}
	// -s: per channel (file) the sums of its level records, its telegrams, and with -D every record
	struct channel_sum {
		unsigned long long blocks = 0, pwr_sum = 0, over = 0, triggered = 0, telegrams = 0;
		int peak = 0, thresh = 0;
		std::vector<tfrec_amd_level> rec;
	};
	std::vector<channel_sum> chan(scan ? n : 0);
	// -P: per bin the sum over every record (a record's sum stays below 2^63, a long file's total need not), the peak, the frames;
	// with -D every record as it came
	std::vector<unsigned __int128> spec_total(spectrum ? spec_n : 0, 0);
	std::vector<uint64_t> spec_peak(spectrum ? spec_n : 0, 0), rec_sum, rec_peak;
	std::vector<uint32_t> rec_frames;
	unsigned long long spec_frames = 0;
	// -A: per bin the records of the file in which it was hit, the records, the file's blocks the batches so far held
	std::vector<unsigned long long> occ_hits(occ ? spec_n : 0, 0);
	unsigned long long occ_records = 0, occ_blocks = 0;
	occ_found.clear();
	for (size_t k = 0; k < n_batches && rc == 0; k++) {
		for (size_t d = 0; d < nd && rc == 0; d++) {
			if (k >= workers[d].plan.size())
				continue;  // (this device's queue has run out)
			if (!workers[d].pop(ev, lv, cb)) {
				rc = workers[d].rc ? workers[d].rc : TFREC_AMD_E_STATE;
				break;
			}
			for (size_t q = 0; q < cb.runs.size() && rc == 0;) {  // -S: the runs of one file are adjacent (the table is ordered by stream)
				const int f = cb.file[q];
				const std::string path = cap_prefix + "." + std::to_string(f) + ".cs16";
				FILE *fp = fopen(path.c_str(), cap_made[f] ? "ab" : "wb");
				if (!fp) {
					perror(path.c_str());
					rc = TFREC_AMD_E_INVAL;
					break;
				}
				cap_made[f] = true;
				for (; q < cb.runs.size() && cb.file[q] == f; q++) {
					const tfrec_amd_run &x = cb.runs[q];
					fprintf(cap_idx, "%d %u %lld %u %d %u\n", f, (unsigned)x.stream, (long long)x.start_sample, (unsigned)x.n_samples, (int)x.thresh,
						(unsigned)x.flags);
					if (fwrite(cb.pool.data() + 2 * (size_t)x.pool_offset, 4, x.n_samples, fp) != x.n_samples)
						rc = TFREC_AMD_E_INVAL;
				}
				if (fclose(fp))
					rc = TFREC_AMD_E_INVAL;
			}
			if (rc)
				break;
			for (size_t q = 0; q < cb.dc_file.size(); q++)  // -z -D
				printf("dc %s I=%d Q=%d\n", files[cb.dc_file[q]].c_str(), (int)cb.dc_last[2 * q], (int)cb.dc_last[2 * q + 1]);
			for (size_t q = 0; q < cb.spec_frames.size(); q++) {  // -P
				spec_frames += cb.spec_frames[q];
				for (int b = 0; b < spec_n; b++) {
					spec_total[b] += cb.spec_sum[q * spec_n + b];
					spec_peak[b] = std::max(spec_peak[b], cb.spec_peak[q * spec_n + b]);
				}
			}
			if (occ) {  // no replay: the channel list is the product
				// the file's samples in this batch: a record that begins behind them lies in the padding and is not the file's
				const unsigned long long nb = workers[d].plan[k].nb;
				const unsigned long long real = std::min<unsigned long long>(nb, file_blocks[0] - std::min<unsigned long long>(file_blocks[0], occ_blocks));
				const unsigned long long real_samples = wide ? real * 327680ull : real * 32768ull * rate_p / rate_q;
				occ_blocks += nb;
				for (size_t q = 0; q < cb.occ_recs.size(); q++) {
					if ((unsigned long long)q * spec_g * spec_n >= real_samples)
						break;
					if (dbg > 0)
						printf("occ-rec %llu floor=%llu hits=%u frames=%u\n", occ_records, (unsigned long long)cb.occ_recs[q].floor,
						       (unsigned)cb.occ_recs[q].n_hit, (unsigned)cb.occ_recs[q].n_frames);
					occ_records++;
					for (int b = 0; b < spec_n; b++)
						occ_hits[b] += (cb.occ_bits[q * (spec_n / 32) + (b >> 5)] >> (b & 31)) & 1u;
				}
				continue;
			}
			if (spectrum && dbg > 0) {
				rec_sum.insert(rec_sum.end(), cb.spec_sum.begin(), cb.spec_sum.end());
				rec_peak.insert(rec_peak.end(), cb.spec_peak.begin(), cb.spec_peak.end());
				rec_frames.insert(rec_frames.end(), cb.spec_frames.begin(), cb.spec_frames.end());
			}
			if (scan) {  // no replay: the table is the product
				const batch_plan &b = workers[d].plan[k];
				for (size_t s = 0; s < b.file.size(); s++) {
					if (b.file[s] < 0)
						continue;
					channel_sum &c = chan[b.file[s]];
					for (int j = 0; j < b.nb && c.blocks < file_blocks[b.file[s]]; j++) {  // (not the padding behind the file's end)
						const tfrec_amd_level &r = lv[s * (size_t)b.nb + j];
						c.blocks++;
						c.pwr_sum += r.pwr_sum;
						c.over += (unsigned long long)r.n_over;
						c.triggered += (unsigned long long)r.triggered;
						c.peak = std::max(c.peak, (int)r.pwr_max);
						c.thresh = r.thresh;
						if (dbg > 0)
							c.rec.push_back(r);
					}
				}
				for (size_t q = 0; q < ev.size(); q++)
					if (ev[q].status == 1 && ev[q].end_sample < stream_samples[ev[q].stream])
						chan[ev[q].stream].telegrams++;
				continue;
			}
			// per stream in time order, slots in registration order like the reference's dispatch loop (fm_demod.cpp:48-49).
			// BITS chunks carry the first sample of their trigger window (a chunk has no per-bit time): a window's bits
			// are replayed when it opens, its flush when it closes -- what store_bit prints keeps its place among the
			// flushes of every window that does not overlap this one.
			std::stable_sort(ev.begin(), ev.end(), [](const tfrec_amd_event &a, const tfrec_amd_event &b) {
				if (a.stream != b.stream) return a.stream < b.stream;
				if (a.end_sample != b.end_sample) return a.end_sample < b.end_sample;
				const bool ab = a.status == TFREC_AMD_STATUS_BITS, bb = b.status == TFREC_AMD_STATUS_BITS;
				if (ab != bb) return ab;
				if (a.slot != b.slot) return a.slot < b.slot;
				return ab && a.offset < b.offset;
			});
			for (size_t q = 0; q < ev.size(); q++)
				if (ev[q].end_sample < stream_samples[ev[q].stream])
					replay(ev[q]);
		}
		if (psink)
			psink->flush();  // the records of the whole batch in one write
	}
	// (after an error: tell the healthy workers to stop, and empty the queues so that they can finish)
	if (rc)
		abort.store(true);
	for (size_t d = 0; d < nd; d++) {
		while (workers[d].pop(ev, lv, cb)) {
		}
		workers[d].th.join();
		if (!rc)
			rc = workers[d].rc;
	}
	if (cap_idx && fclose(cap_idx) && !rc)
		rc = TFREC_AMD_E_INVAL;
	if (scan && !rc)
		for (size_t s = 0; s < n; s++) {
			const channel_sum &c = chan[s];
			for (const tfrec_amd_level &r : c.rec)  // fm_demod.cpp:61, per channel
				printf("%ld Trigger ratio %d/%d, avg %d\n", scan_khz[s], (int)r.triggered, TFREC_AMD_BLOCK_DEC, (int)r.triggered_avg);
			printf("scan %ld blocks=%llu mean_pwr=%llu peak=%d over=%llu triggered=%llu thresh=%d telegrams=%llu\n", scan_khz[s], c.blocks,
			       c.blocks ? c.pwr_sum / ((unsigned long long)TFREC_AMD_BLOCK_DEC * c.blocks) : 0ull, c.peak, c.over, c.triggered,
			       c.blocks ? c.thresh : (settings[s].thresh ? settings[s].thresh : 500), c.telegrams);
		}
	if (out_mode)  // -m 1: summary at the end (decoder.cpp:98-109)
		for (size_t s = 0; s < decs.size(); s++)
			for (size_t k2 = 0; k2 < decs[s].size(); k2++)
				if (decs[s][k2])
					decs[s][k2]->flush_storage();
	if (occ && !rc) {  // -A: the channel list
		const std::vector<occ_channel> ch = occupancy_channels(occ_hits, occ_records, spec_n, fs_in, spec_center, occ_join);
		for (const occ_channel &c : ch) {
			if (c.carrier) {
				printf("carrier %ld hits=%llu/%llu\n", c.khz, c.hits, occ_records);
				continue;
			}
			printf("found %ld bins=%d..%d hits=%llu/%llu%s\n", c.khz, c.lo, c.hi, c.hits, occ_records, c.in_range ? "" : " out-of-range");
			if (c.in_range)
				occ_found.push_back(c.khz);
		}
		if (occ_found.size() > 4096) {
			fprintf(stderr, "tfrec_gpu: -A found %zu channels, at most 4096 are scanned at once\n", occ_found.size());
			rc = TFREC_AMD_E_INVAL;
		}
	}
	if (spectrum && !occ && !rc) {  // -P: behind the telegram output
		for (size_t q = 0; q < rec_frames.size(); q++)
			for (int k : spec_order)
				printf("spec-rec %zu %.3f sum=%llu peak=%llu frames=%u\n", q, spec_khz[k], (unsigned long long)rec_sum[q * spec_n + k],
				       (unsigned long long)rec_peak[q * spec_n + k], (unsigned)rec_frames[q]);
		for (int k : spec_order)
			printf("spec %.3f mean=%llu peak=%llu\n", spec_khz[k],
			       spec_frames ? (unsigned long long)(spec_total[k] / spec_frames) : 0ull, (unsigned long long)spec_peak[k]);
	}
	if (psink)
		psink->flush();
	return rc;
}
