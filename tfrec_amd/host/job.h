// tfrec_amd/host/job.h -- the pure half of tfrec_gpu's engine: what a job is, how its files are cut into batches, and what
// becomes of a batch's results.  Functions of small inputs only: nothing here opens a device, calls the C ABI or knows a
// decoder -- include/tfrec_amd.h is included for its struct types -- so all of it runs in a CPU test (tests/host_engine_driver.cpp).
// device_worker.h is the half that drives a context with these plans; gpu_engine.cpp puts the two together.
#ifndef TFREC_AMD_HOST_JOB_H
#define TFREC_AMD_HOST_JOB_H

#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/tfrec_amd.h"
#include "../csrc/crc_table.h"  // the frame check's settings, as the enable call checks them: plain C++

// -T, -t, -W and the tune of one dump file (tfrec_gpu -p; tune: -f minus -c, in Hz, tfrec_amd_tune_streams)
struct file_settings {
	int types, thresh, filter;
	int tune;  // Hz
	bool same_config(const file_settings &o) const { return types == o.types && thresh == o.thresh && filter == o.filter; }
	bool operator==(const file_settings &o) const { return same_config(o) && tune == o.tune; }
	bool operator!=(const file_settings &o) const { return !(*this == o); }
};

// -R: one file of a capture (tfrec_gpu -S), read back whole: its .idx lines in order -- start_sample counted within the file,
// pool_offset into `pool` --, its .cs16 pairs and its .pre pairs, one per line
struct replay_file {
	int index;  // the file index of the .idx lines
	std::vector<tfrec_amd_run> runs;
	std::vector<int16_t> pool, pre;
	// the last run's end rounded up to blocks
	size_t blocks() const
	{
		const long long end = runs.empty() ? 0 : runs.back().start_sample + (long long)runs.back().n_samples;
		return (size_t)((end + TFREC_AMD_BLOCK_DEC - 1) / TFREC_AMD_BLOCK_DEC);
	}
};

// -K: what a file continues from, read back whole before a device is opened: the stream's state blob (<prefix>.<file>.state,
// tfrec_amd_load_streams) and the bytes of the part before it that did not fill a piece (<prefix>.<file>.rest; none: empty)
struct kept_input {
	std::vector<uint8_t> state, rest;
	long long samples() const  // the decimated samples the stream has run (the blob header's samples_since_restart)
	{
		tfrec_amd_state_header h;
		if (state.size() < sizeof(h))
			return 0;
		memcpy(&h, state.data(), sizeof(h));
		return h.samples_since_restart;
	}
};

// -k / -K: how the bytes of a file that arrives in pieces are used.  The input is `head` bytes carried in (-K's .rest, 0 without)
// followed by the file's `file` bytes; it is processed in whole pieces of `piece` bytes = `unit` blocks and nothing is padded.
// What does not fill a piece is the rest -- its last bytes, rest_head of them still the head's (a file shorter than a piece) and
// rest_file the file's own last ones --, which -k writes out for the next part and a run without -k drops, as it always did.
struct kept_bytes {
	size_t blocks;                // whole blocks processed: pieces x unit
	size_t used_head, used_file;  // bytes of the head and of the file that the pieces hold
	size_t rest_head, rest_file;  // the rest, in input order: the head's last rest_head bytes, then the file's last rest_file
};
inline kept_bytes plan_kept_bytes(size_t head, size_t file, size_t piece, int unit)
{
	kept_bytes k;
	const size_t used = piece ? (head + file) / piece * piece : 0;
	k.blocks = piece ? used / piece * (size_t)unit : 0;
	k.used_head = std::min(head, used);
	k.used_file = used - k.used_head;
	k.rest_head = head - k.used_head;
	k.rest_file = file - k.used_file;
	return k;
}

// Everything gpu_engine's set_* calls store (gpu_engine.h says what each mode does), one copy for the engine and all its workers,
// and the input geometry that follows from it.
struct job_settings {
	bool wide = false;             // set_wide
	int rate_p = 1, rate_q = 1;    // set_rate (1 / 1: none)
	int fmt = TFREC_AMD_FMT_U8;    // set_format
	int slots = 0;                 // set_slots (0: one stream per file)
	bool bits_replay = false;      // set_bits_replay
	int dbg = 0;                   // the constructor's: -1 quiet, 0 normal, >= 1 debug
	bool scan = false;             // set_scan
	std::vector<long> scan_khz;
	bool capture = false;          // set_capture
	std::string cap_prefix;
	bool spectrum = false;         // set_spectrum
	int spec_n = 0, spec_g = 0;
	long spec_center = 0;
	int occ_ratio = 0, occ_rel = 0;  // set_occupancy (0: none)
	long occ_join = 0;
	int dc_windows = 0;            // set_dc (0: none)
	int iq_windows = 0;            // set_iq (0: none)
	bool meter = false;            // set_meter
	bool envelope = false;         // set_envelope
	bool clock = false;            // set_clock
	long track_rate = 0;           // set_track (0: none): the rate in bit/s, 1000 .. 96000
	long track_centre = 0;         // ... and every stream's centre in Hz
	long track_level = -1;         // set_track_level (-1: none): -O, the track is the amplitude's, every stream at this level, 0 .. 65535
	bool track_auto = false;       // set_track_auto: -G rate,auto, every chain about its own measured centre (K = kTrackAutoHead)
	int track_lag = 0;             // set_track_phase (0: none): -G rate,psk, the phase track's m, 1 .. 64 (with track_auto: its centre records)
	int sync_bits = 0;             // set_sync (0: none): P, the sync word's bits, 8 .. 64
	unsigned long long sync_pattern = 0;  // ... the word, in its low P bits
	int sync_errors = 0;           // ... E
	int sync_bytes = 8;            // ... the payload bytes read behind the word
	bool sync_both = false;        // ... the complemented word too
	bool sync_lsb = false;         // ... the frames' hex LSB-first per byte
	uint32_t code_taps = 0;        // set_code (0: none): -U, the line code's taps, bit j - 1 a delay of j symbols at -G's rate
	bool code_invert = false;      // ... and its INVERT
	int crc_width = 0;             // set_crc (0: none): -V, the frame check's width; its N is sync_bytes, its byte order sync_lsb, its rate -G's
	uint32_t crc_poly = 0, crc_init = 0, crc_xorout = 0;  // ...
	int crc_skip = 0;              // ... the bytes behind the sync word that the CRC does not cover
	bool crc_invert = false;       // ... and its INVERT
	const std::vector<replay_file> *replay = NULL;  // set_replay (NULL: the files are dumps)
	std::string keep_prefix;       // set_keep ("": none)
	std::string cont_prefix;       // set_continue ("": none)
	const std::vector<kept_input> *cont = NULL;  // ... and what it read, per file (the engine's, before the workers start)

	bool keeping() const { return !keep_prefix.empty(); }
	bool continuing() const { return !cont_prefix.empty(); }
	static std::string kept_path(const std::string &prefix, size_t file, const char *ext) { return prefix + "." + std::to_string(file) + ext; }

	bool resampled() const { return rate_p != 1 || rate_q != 1; }
	bool occupancy() const { return spectrum && occ_ratio; }  // -A, pass 1
	bool recorder() const { return capture || metering() || enveloping() || clocking() || tracking(); }  // the contexts enable the recorder: for -S, or as the meter's, the envelope's, the clock's or the track's table
	bool tracking() const { return track_rate != 0; }  // -G (never with -s or -A)
	bool syncing() const { return sync_bits != 0; }  // -Y (only with -G)
	bool coding() const { return code_taps != 0; }  // -U (only with -G)
	bool checking() const { return crc_width != 0; }  // -V (only with -Y)
	tfrec_crc::Settings crc_settings() const  // tfrec_amd_enable_burst_crc's arguments
	{
		const tfrec_crc::Settings s = { (int32_t)track_rate, (int32_t)sync_bytes, (int32_t)crc_skip, (int32_t)crc_width, crc_poly, crc_init, crc_xorout,
						(sync_lsb ? TFREC_AMD_CRC_LSB : 0u) | (crc_invert ? TFREC_AMD_CRC_INVERT : 0u) };
		return s;
	}
	bool amplitude() const { return track_level >= 0; }  // -O (only with -G)
	bool centring() const { return track_auto; }  // -G rate,auto or -G rate,psk: the track has centre records (never with -O)
	bool phasing() const { return track_lag != 0; }  // -G rate,psk
	// -G's L: half a symbol, (384000 + rate) / (2 rate) held within 1 .. 16
	int track_smooth() const { return (int)std::max(1L, std::min(16L, (384000 + track_rate) / (2 * track_rate))); }
	bool metering() const { return meter && !occupancy(); }  // -M (under -A: in the scan, not in pass 1)
	bool enveloping() const { return envelope && !occupancy(); }  // -Q (likewise)
	bool clocking() const { return clock && !occupancy(); }  // -C (likewise)
	bool share() const { return slots <= 0; }  // one stream per file for the whole job: a path given several times is read once
	// -r: the blocks a piece of a file holds, q / gcd(q, 64) -- the odd part of a q <= 64, 6 at 625/384; 1 without -r: every
	// batch carries a multiple of it (tfrec_amd_create_rate: Submits)
	int unit() const
	{
		int g = 64;
		while (rate_q % g)
			g /= 2;
		return rate_q / g;
	}
	// bytes of a piece of `unit` blocks of a file: 65536 p / q x unit is a whole number (q is unit times a power of two <= 64);
	// -F: times the format's bytes per complex sample / 2; 655360 with -x
	size_t piece_bytes() const
	{
		const size_t sample_bytes = fmt == TFREC_AMD_FMT_F32 ? 8 : fmt == TFREC_AMD_FMT_S16 ? 4 : 2;
		return wide ? (size_t)TFREC_AMD_BLOCK_BYTES_10X : (size_t)TFREC_AMD_BLOCK_BYTES * rate_p * unit() / rate_q * sample_bytes / 2;
	}
	// input samples of `blocks` blocks (rounded down); of one block: the default record of -P and -A
	unsigned long long input_samples(unsigned long long blocks) const
	{
		return wide ? blocks * 327680ull : blocks * 32768ull * rate_p / rate_q;
	}
	long fs_in() const { return wide ? 15360000L : 1536000L * rate_p / rate_q; }  // input samples per second
	uint32_t ctx_flags() const  // TFREC_AMD_F_* of every context
	{
		return (bits_replay ? (TFREC_AMD_F_BITS | TFREC_AMD_F_ALL_FLUSHES) : 0u) | (wide ? TFREC_AMD_F_INPUT_10X : 0u) |
		       (scan ? TFREC_AMD_F_LEVELS : 0u);
	}
};

// The files [s0, s1) of device d of nd: contiguous ranges of the n files, as evenly as possible (tfrec_amd/shard.py)
inline void shard_range(size_t n, size_t nd, size_t d, size_t &s0, size_t &s1)
{
	const size_t base = n / nd, rem = n % nd;
	s0 = d * base + std::min(d, rem);
	s1 = s0 + base + (d < rem ? 1 : 0);
}

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
// settings: every file's; dflt: the context's.  whole (-k): no batch reaches past the end of a file it carries -- it has the blocks of
// the file with the fewest left --, so that no stream is fed padding before its state is saved.
inline std::vector<batch_plan> plan_batches(const std::vector<size_t> &file_blocks, const std::vector<file_settings> &settings,
					    const file_settings &dflt, size_t s0, size_t s1, size_t nslots, int bps, bool whole = false)
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
		size_t most = 0, least = (size_t)bps;
		for (size_t j = 0; j < nslots; j++)
			if (cur[j] >= 0) {
				most = std::max(most, left[j]);
				least = std::min(least, left[j]);
			}
		if (most == 0)
			break;
		b.nb = (int)(whole ? least : std::min<size_t>((size_t)bps, most));
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

// -R: the part of a capture that one submit of `stream` holds, samples [base, base + M) of the file -> appended to the submit's
// table (start_sample relative to base, pool_offset into `pool`), pool and pre, as tfrec_amd_submit_runs takes them (tfrec_amd/decin.py:
// rebase).  A run is cut at the submit's boundaries: a part that begins inside a run has the run's pair before it as its pre.
// Runs that touch -- the two halves of one the recording cut at a submit boundary -- are joined.  from: the first run that may
// reach into the submit, moved on for the next one.
inline void rebase_runs(const replay_file &rf, uint32_t stream, long long base, long long M, size_t &from, std::vector<tfrec_amd_run> &tab,
			std::vector<int16_t> &pool, std::vector<int16_t> &pre)
{
	const size_t first = tab.size();
	while (from < rf.runs.size() && rf.runs[from].start_sample + (long long)rf.runs[from].n_samples <= base)
		from++;
	for (size_t i = from; i < rf.runs.size() && rf.runs[i].start_sample < base + M; i++) {
		const tfrec_amd_run &r = rf.runs[i];
		const long long a = r.start_sample, lo = std::max(a, base), hi = std::min(a + (long long)r.n_samples, base + M);
		if (lo >= hi)
			continue;
		const int16_t *src = rf.pool.data() + 2 * ((size_t)r.pool_offset + (size_t)(lo - a));
		if (tab.size() > first && tab.back().start_sample + (long long)tab.back().n_samples == lo - base) {
			tab.back().n_samples += (uint32_t)(hi - lo);
		} else {
			tfrec_amd_run x = r;
			x.stream = stream;
			x.start_sample = lo - base;
			x.n_samples = (uint32_t)(hi - lo);
			x.pool_offset = pool.size() / 2;
			tab.push_back(x);
			const int16_t *p = lo == a ? rf.pre.data() + 2 * i : src - 2;
			pre.push_back(p[0]);
			pre.push_back(p[1]);
		}
		pool.insert(pool.end(), src, src + 2 * (size_t)(hi - lo));
	}
}

// -r: a batch's tunes as the two calls they become.  An offset within +-767 kHz is a tune behind the resampler, as it always
// was (tfrec_amd_tune_streams: narrow); a larger one is the input-rate tune ahead of it (tfrec_amd_tune_streams_input: input).
// A stream that goes from one kind to the other (-n) has the other kind cleared to 0; all of it is one restart.  in_tune /
// narrow_tune: per stream, whether it has a tune of that kind now -- a stream that never had one is never sent a clear for it.
struct tune_calls {
	std::vector<int32_t> narrow, narrow_hz, input, input_hz;
};
inline tune_calls split_tunes(const std::vector<int32_t> &tune, const std::vector<int32_t> &tune_hz, std::vector<bool> &in_tune,
			      std::vector<bool> &narrow_tune)
{
	tune_calls c;
	for (size_t i = 0; i < tune.size(); i++) {
		const int32_t s = tune[i], hz = tune_hz[i];
		const bool far = hz <= -768000 || hz >= 768000;
		if (far || in_tune[s]) {
			c.input.push_back(s);
			c.input_hz.push_back(far ? hz : 0);
			in_tune[s] = far;
		}
		if (!far || narrow_tune[s]) {
			c.narrow.push_back(s);
			c.narrow_hz.push_back(far ? 0 : hz);
			narrow_tune[s] = !far && hz != 0;
		}
	}
	return c;
}

// -A: one line of the channel list: a carrier (one bin, listed, never scanned) or a group of active bins lo .. hi (signed bins: b = k
// for k < N/2, else k - N); hits: the carrier's, or the largest of the group's bins
struct occ_channel {
	bool carrier;
	long khz;
	int lo, hi;
	unsigned long long hits;
	bool in_range;  // a group the scan can reach: |khz - center| * 1000 <= fs_in / 2 - 192000
};

// floor(a / b) for b > 0
inline long long floor_div(long long a, long long b) { return a / b - (a % b < 0 ? 1 : 0); }

// Group the hit counts of a recording into channels (tfrec_amd/occupancy.py: channels()), exact integers: hits[k] of
// `records` records, bin k; ascending frequency.
inline std::vector<occ_channel> occupancy_channels(const std::vector<unsigned long long> &hits, unsigned long long records, int n_bins,
						   long fs_in, long center_khz, long join_hz)
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

// What one batch of one device brings to the engine's thread: its flush events (stream = the file's index in the job), and
// -s: its level records, [stream][the batch's blocks]
// -S: the runs that belong to a file (file[i]: its index in the job), cut at the file's end, and the batch's sample pool, which
//     their pool_offset indexes; pre: the pair ahead of every run kept
// -P: the spectrum records of input row 0, [record][bin], and their frame counts
// -A: the detector's records of row 0 and their bitmap words, [record][N / 32]
// -z with -D: per file of the batch its index in the job and the last window's {d_I, d_Q} of its row
// -M: the burst records that belong to a file (stream = its index in the job), n_samples cut at the file's end (cut_at_file_end)
// -Q: the envelope records likewise; one that is cut at the file's end is OPEN (the input's end cut its tail)
// -C: the clock records likewise
// -G: the track records likewise, each with its bits out of the batch's bitmap (track_piece; its functions are further down)
constexpr uint64_t kTrackKeep = 1ull << 20;  // the samples of a chain's track that are kept

// The file-end cut of a burst stage's record (-M, -Q, -C, -G, -Y), as the device delivers it: stream is the batch's slot, `file`
// the batch's map from slot to file (its index in the job; -1: idle) and file_blocks every file's length.  A record of an idle
// slot, of a slot beyond the map, or that begins at or behind its file's end is dropped (false).  Otherwise stream becomes the
// file's index, and a record that reaches over the file's end keeps the n_samples inside the file; cut_opens: it is then OPEN too
// -- the input's end cut its tail --, which every stage's reader asks for but -M's.  The record's sums stay the device's: the
// padding behind a file's end is silence.
template <class R>
inline bool cut_at_file_end(R &x, const std::vector<int> &file, const std::vector<size_t> &file_blocks, bool cut_opens)
{
	if (x.stream >= file.size() || file[x.stream] < 0)
		return false;
	const int f = file[x.stream];
	const long long end = (long long)file_blocks[f] * TFREC_AMD_BLOCK_DEC;
	if (x.start_sample >= end)
		return false;
	if (x.start_sample + (long long)x.n_samples > end) {
		x.n_samples = (uint32_t)(end - x.start_sample);
		if (cut_opens)
			x.flags |= TFREC_AMD_RUN_OPEN;
	}
	x.stream = (uint32_t)f;
	return true;
}

// A record with its track: bit k of the track is bit k & 31 of bits[k >> 5], for k < min(n_samples, 2^20).  -G rate,auto: with
// the centre record of the same table entry (centred; centre_take)
struct track_piece : tfrec_amd_track {
	std::vector<uint32_t> bits;
	bool centred = false;
	tfrec_amd_track_centre cen = {};
	uint64_t kept() const { return std::min<uint64_t>(n_samples, kTrackKeep); }
	bool bit(uint64_t k) const { return (bits[k >> 5] >> (k & 31)) & 1u; }
};

// -Y: a sync record with its match track (packed as a track_piece's bits) and the track piece of the same table entry
struct sync_piece : tfrec_amd_burst_sync {
	std::vector<uint32_t> match;
	track_piece trk;
	uint64_t kept() const { return std::min<uint64_t>(n_samples, kTrackKeep); }
	bool hit(uint64_t k) const { return (match[k >> 5] >> (k & 31)) & 1u; }
};

// -V: a check record with its check track (packed as a track_piece's bits)
struct crc_piece : tfrec_amd_burst_crc {
	std::vector<uint32_t> ok;
	uint64_t kept() const { return std::min<uint64_t>(n_samples, kTrackKeep); }
	bool bit(uint64_t k) const { return (ok[k >> 5] >> (k & 31)) & 1u; }
};

struct batch_result {
	std::vector<track_piece> tracks;
	std::vector<sync_piece> syncs;  // (-Y: in place of tracks; -U -Y: beside them, each with the CODED piece of its entry for its track piece)
	std::vector<track_piece> codes;  // (-U without -Y: the coded pieces of the entries in tracks)
	std::vector<crc_piece> crcs;  // (-V: the check pieces of the entries in syncs)
	std::vector<tfrec_amd_burst> bursts;
	std::vector<tfrec_amd_envelope> envelopes;
	std::vector<tfrec_amd_clock> clocks;
	std::vector<tfrec_amd_event> ev;
	std::vector<tfrec_amd_level> lv;
	std::vector<tfrec_amd_run> runs;
	std::vector<int> file;
	std::vector<int16_t> pool, pre;
	std::vector<uint64_t> spec_sum, spec_peak;
	std::vector<uint32_t> spec_frames;
	std::vector<tfrec_amd_occupancy> occ_recs;
	std::vector<uint32_t> occ_bits;
	std::vector<int> dc_file;
	std::vector<int16_t> dc_last;
	std::vector<int> iq_file;  // -Z -D: as dc_file and dc_last, the last window's {t, g}
	std::vector<int16_t> iq_last;
};

// ---- the sums behind the output modes' tables, one consumer per mode: begin() prints what the mode says before a device is
// opened, take() is given every batch in the order of the output, finish() prints what follows the last one.  take() only adds up
// and is defined here; begin() and finish(), and the two consumers that do nothing but write (-S, -z -D), are gpu_engine.cpp's.

// -P: the spectrum table (gpu_engine.h: set_spectrum).  Per bin the sum over every record (a record's sum stays below 2^63, a long
// file's total need not), the peak, the frames; with -D every record as it came.  Under -A only begin() is used.
struct spectrum_table {
	int n;
	bool keep;  // -D
	std::vector<double> khz;  // bin k lies at center + (k < N/2 ? k : k - N) fs_in / N; listed (and printed) in ascending frequency
	std::vector<int> order;
	std::vector<unsigned __int128> total;
	std::vector<uint64_t> peak, rec_sum, rec_peak;
	std::vector<uint32_t> rec_frames;
	unsigned long long frames;
	spectrum_table() : n(0), keep(false), frames(0) {}
	void begin(const job_settings &job);
	void take(const batch_result &b)
	{
		for (size_t q = 0; q < b.spec_frames.size(); q++) {
			frames += b.spec_frames[q];
			for (int k = 0; k < n; k++) {
				total[k] += b.spec_sum[q * n + k];
				peak[k] = std::max(peak[k], b.spec_peak[q * n + k]);
			}
		}
		if (keep) {
			rec_sum.insert(rec_sum.end(), b.spec_sum.begin(), b.spec_sum.end());
			rec_peak.insert(rec_peak.end(), b.spec_peak.begin(), b.spec_peak.end());
			rec_frames.insert(rec_frames.end(), b.spec_frames.begin(), b.spec_frames.end());
		}
	}
	void finish() const;
};

// -A, pass 1: the channel list (gpu_engine.h: set_occupancy).  Per bin the records of the file in which it was hit, the records, and
// the file's blocks the batches so far held.
struct occupancy_list {
	const job_settings *job;
	std::vector<unsigned long long> hits;
	unsigned long long records, blocks;
	std::vector<long> found;  // the channels a scan can reach, ascending
	occupancy_list() : job(NULL), records(0), blocks(0) {}
	void begin(const job_settings &j);
	// a batch of nb blocks of the file of file_blocks blocks -> how many of its records, from the first on, are the file's
	size_t take(const batch_result &b, unsigned long long nb, unsigned long long file_blocks)
	{
		// the file's samples in this batch: a record that begins behind them lies in the padding and is not the file's
		const unsigned long long real_samples = job->input_samples(std::min(nb, file_blocks - std::min(file_blocks, blocks)));
		const int n = job->spec_n;
		blocks += nb;
		size_t q = 0;
		for (; q < b.occ_recs.size() && (unsigned long long)q * job->spec_g * n < real_samples; q++) {
			records++;
			for (int k = 0; k < n; k++)
				hits[k] += (b.occ_bits[q * (n / 32) + (k >> 5)] >> (k & 31)) & 1u;
		}
		return q;
	}
	int finish();
};

// ---- -M: the burst meter's records (include/tfrec_amd.h: tfrec_amd_burst, whose text is normative; tfrec_amd/burst.py restates
// merge, summary and the line)

// piece p, which CONTINUES the chain c, added to it
inline void burst_add(tfrec_amd_burst &c, const tfrec_amd_burst &p)
{
	c.n_samples += p.n_samples;
	c.n_products += p.n_products;
	c.sum_dot += p.sum_dot;
	c.sum_crs += p.sum_crs;
	c.energy += p.energy;
	for (int j = 0; j < 64; j++)
		c.hist[j] += p.hist[j];
	c.pwr_max = std::max(c.pwr_max, p.pwr_max);
	c.flags = (c.flags & TFREC_AMD_RUN_CONTINUES) | (p.flags & TFREC_AMD_RUN_OPEN);
}

// -> whether a bin is occupied (hist[j] >= (P + 15) / 16, P = n_products > 0); then centre and deviation in Hz from the smallest
// and the largest signed index of an occupied bin
inline bool burst_summary(const tfrec_amd_burst &r, long &centre_hz, long &deviation_hz)
{
	const unsigned long long thr = ((unsigned long long)r.n_products + 15) / 16;
	int lo = 64, hi = -64;
	for (int j = 0; j < 64 && r.n_products; j++)
		if (r.hist[j] >= thr) {
			const int b = j < 32 ? j : j - 64;
			lo = std::min(lo, b);
			hi = std::max(hi, b);
		}
	if (hi < lo)
		return false;
	centre_hz = 3000L * (lo + hi);
	deviation_hz = 3000L * (hi - lo);
	return true;
}

// burst <file> <start_sample> <n_samples> <pwr_max> <centre_hz|-> <deviation_hz|->
inline std::string burst_line(const std::string &file, const tfrec_amd_burst &r)
{
	long c = 0, d = 0;
	std::string s = "burst " + file + " " + std::to_string((long long)r.start_sample) + " " + std::to_string(r.n_samples) + " " +
			std::to_string(r.pwr_max);
	if (burst_summary(r, c, d))
		return s + " " + std::to_string(c) + " " + std::to_string(d);
	return s + " - -";
}

// ---- -Q: the burst envelope's records (include/tfrec_amd.h: tfrec_amd_envelope, whose text is normative; tfrec_amd/envelope.py
// restates merge, summary and the line)

// piece p, which CONTINUES the chain c, merged into it: the record the two would have had as one piece (the header's Cutting)
inline void envelope_add(tfrec_amd_envelope &c, const tfrec_amd_envelope &p)
{
	const long long na = c.n_samples, la = c.last_over, lb = p.last_over;
	const long long joined = (na - 1 - la) + p.lead_not_over;  // the stretch of not-over samples across the cut
	const bool both = la >= 0 && lb >= 0;
	c.n_gaps += p.n_gaps + (both && joined > 0 ? 1u : 0u);
	c.max_gap = std::max(std::max(c.max_gap, p.max_gap), both ? (uint32_t)joined : 0u);
	if (la < 0)
		c.lead_not_over = (uint32_t)(na + p.lead_not_over);
	if (lb >= 0) {  // everything of c lies ahead of p's last over sample: head
		c.energy_head += c.energy_tail + p.energy_head;
		c.dot_head += c.dot_tail + p.dot_head;
		c.crs_head += c.crs_tail + p.crs_head;
		c.nprod_head += c.nprod_tail + p.nprod_head;
		c.energy_tail = p.energy_tail;
		c.dot_tail = p.dot_tail;
		c.crs_tail = p.crs_tail;
		c.nprod_tail = p.nprod_tail;
		c.last_over = (int32_t)(na + lb);
	} else {  // (p's head is empty)
		c.energy_tail += p.energy_tail;
		c.dot_tail += p.dot_tail;
		c.crs_tail += p.crs_tail;
		c.nprod_tail += p.nprod_tail;
	}
	c.n_samples += p.n_samples;
	c.n_over += p.n_over;
	c.flags = (c.flags & TFREC_AMD_RUN_CONTINUES) | (p.flags & TFREC_AMD_RUN_OPEN);
}

// -> the burst's length and its tail's, and whether ratio_c is defined (the chain not OPEN, len > 0, energy_tail > 0, n_tail >= 64);
// then ratio_c = floor(100 energy_head n_tail / (energy_tail len)), in 128-bit integers
inline bool envelope_summary(const tfrec_amd_envelope &r, long long &len, long long &n_tail, unsigned long long &ratio_c)
{
	len = (long long)r.last_over + 1;
	n_tail = (long long)r.n_samples - len;
	if ((r.flags & TFREC_AMD_RUN_OPEN) || len <= 0 || !r.energy_tail || n_tail < 64)
		return false;
	const unsigned __int128 num = (unsigned __int128)100 * r.energy_head * (unsigned long long)n_tail;
	const unsigned __int128 den = (unsigned __int128)r.energy_tail * (unsigned long long)len;
	ratio_c = (unsigned long long)(num / den);  // (< 100 * 2^31 * 2^32)
	return true;
}

// extent <file> <start_sample> <n_samples> <burst_samples> <n_over> <n_gaps> <max_gap> <ratio_c as %d.%02d|-> <snr_db|->
inline std::string envelope_line(const std::string &file, const tfrec_amd_envelope &r)
{
	long long len = 0, n_tail = 0;
	unsigned long long ratio = 0;
	const bool have = envelope_summary(r, len, n_tail, ratio);
	std::string s = "extent " + file + " " + std::to_string((long long)r.start_sample) + " " + std::to_string(r.n_samples) + " " +
			std::to_string(len) + " " + std::to_string(r.n_over) + " " + std::to_string(r.n_gaps) + " " + std::to_string(r.max_gap);
	if (!have)
		return s + " - -";
	char buf[96];
	snprintf(buf, sizeof(buf), " %llu.%02llu", ratio / 100, ratio % 100);
	s += buf;
	if (!ratio)
		return s + " -";
	snprintf(buf, sizeof(buf), " %.1f", 10.0 * log10((double)ratio / 100.0));  // presentation only: ratio_c is the exact figure
	return s + buf;
}

// ---- -C: the burst clock's records (include/tfrec_amd.h: tfrec_amd_clock, whose text is normative; tfrec_amd/clock.py restates
// merge, summary and the line)

// piece p, which CONTINUES the chain c, merged into it: the sums added, spec saturating at 2^64 - 1 (the header's Cutting)
inline void clock_add(tfrec_amd_clock &c, const tfrec_amd_clock &p)
{
	c.n_samples += p.n_samples;
	c.n_segments += p.n_segments;
	c.n_silent += p.n_silent;
	for (int i = 0; i < 128; i++) {
		const uint64_t v = c.spec[i] + p.spec[i];
		c.spec[i] = v < p.spec[i] ? UINT64_MAX : v;
	}
	c.flags = (c.flags & TFREC_AMD_RUN_CONTINUES) | (p.flags & TFREC_AMD_RUN_OPEN);
}

// -> whether the summary is defined (n_segments > 0 and the band j = 12 .. 128 not empty); then clock_hz = 375 jp + off and
// quality_c = floor(100 * 117 * P[jp] / tot), in 128-bit integers (P[j] = spec[j - 4] may be saturated: 117 of them need 71 bits)
inline bool clock_summary(const tfrec_amd_clock &r, long long &clock_hz, unsigned long long &quality_c)
{
	unsigned __int128 tot = 0;
	int jp = 12;
	for (int j = 12; j <= 128; j++) {
		tot += r.spec[j - 4];
		if (r.spec[j - 4] > r.spec[jp - 4])
			jp = j;  // (the lowest j of the maximum)
	}
	if (!r.n_segments || !tot)
		return false;
	const __int128 p0 = r.spec[jp - 4], pm = r.spec[jp - 5], pp = r.spec[jp - 3];
	const __int128 num = pp - pm, den = 2 * p0 - pm - pp;
	__int128 off = 0;
	if (den > 0 && pm <= p0 && pp <= p0) {
		const __int128 a = 375 * num + den, b = 2 * den;  // floor(a / b), b > 0
		off = a / b - ((a % b) < 0 ? 1 : 0);
	}
	clock_hz = 375LL * jp + (long long)off;
	quality_c = (unsigned long long)((unsigned __int128)100 * 117 * (unsigned __int128)p0 / tot);  // (<= 100 * 117)
	return true;
}

// clock <file> <start_sample> <n_samples> <n_segments> <clock_hz|-> <quality_c as %d.%02d|->
inline std::string clock_line(const std::string &file, const tfrec_amd_clock &r)
{
	long long hz = 0;
	unsigned long long q = 0;
	std::string s = "clock " + file + " " + std::to_string((long long)r.start_sample) + " " + std::to_string(r.n_samples) + " " +
			std::to_string(r.n_segments);
	if (!clock_summary(r, hz, q))
		return s + " - -";
	char buf[96];
	snprintf(buf, sizeof(buf), " %lld %llu.%02llu", hz, q / 100, q % 100);
	return s + buf;
}

// ---- -G: the burst track's records and bits (include/tfrec_amd.h: tfrec_amd_track, whose text is normative; tfrec_amd/track.py
// restates merge, the slicer and the line)

// n bits of src from bit src_off on -> dst, from its bit dst_len on, as far as the kept 2^20 reach
inline void track_append(std::vector<uint32_t> &dst, uint64_t dst_len, const uint32_t *src, uint64_t src_off, uint64_t n)
{
	if (dst_len >= kTrackKeep)
		return;
	n = std::min(n, kTrackKeep - dst_len);
	dst.resize((size_t)((dst_len + n + 31) >> 5), 0u);
	for (uint64_t k = 0; k < n; k++)
		if ((src[(src_off + k) >> 5] >> ((src_off + k) & 31)) & 1u)
			dst[(dst_len + k) >> 5] |= 1u << ((dst_len + k) & 31);
}

// a device record and the submit's bitmap -> the piece, n samples of it (n <= the record's: the file's end may cut it): its bits
// from bit_offset on, n_ones counted again on what is kept of a cut piece
inline track_piece track_take(const tfrec_amd_track &r, const uint32_t *words, uint32_t n)
{
	track_piece p;
	static_cast<tfrec_amd_track &>(p) = r;
	const bool cut = n < r.n_samples;
	p.n_samples = n;
	track_append(p.bits, 0, words, r.bit_offset, n);
	if (cut) {
		p.n_ones = 0;
		for (uint64_t k = 0; k < p.kept(); k++)
			p.n_ones += p.bit(k);
		if (p.last_over >= (int32_t)n)  // (the padding behind a file's end is silence: not over)
			p.last_over = (int32_t)n - 1;
	}
	return p;
}

// piece p, which CONTINUES the chain c, merged into it (the header's Cutting): the tracks concatenated, n_samples and n_ones added,
// last_over by the envelope's rule
inline void track_add(track_piece &c, const track_piece &p)
{
	if (!p.bits.empty())
		track_append(c.bits, c.kept(), p.bits.data(), 0, p.kept());
	if (p.last_over >= 0)
		c.last_over = (int32_t)((long long)c.n_samples + p.last_over);
	c.n_samples += p.n_samples;
	c.n_ones += p.n_ones;
	c.flags = (c.flags & TFREC_AMD_RUN_CONTINUES) | (p.flags & TFREC_AMD_RUN_OPEN);
}

// sym(l) = floor((2 l R + 384000) / 768000) (l <= 2^20, R <= 96000: below 2^39)
inline uint64_t track_sym(uint64_t l, long rate) { return (2 * l * (uint64_t)rate + 384000) / 768000; }

// The header's Slicing on the first min(last_over + 1, 2^20) samples of a merged track -> the symbols, one per byte
inline std::vector<uint8_t> track_slice(const track_piece &c, long rate)
{
	std::vector<uint8_t> out;
	const uint64_t n = c.last_over < 0 ? 0 : std::min<uint64_t>((uint64_t)c.last_over + 1, c.kept());
	bool have = false, v = false;
	uint64_t l = 0;
	for (uint64_t k = 0; k < n;) {
		const bool w = c.bit(k);
		uint64_t m = 1;
		while (k + m < n && c.bit(k + m) == w)
			m++;
		k += m;
		if (!have) {
			if (track_sym(m, rate)) {
				have = true;
				v = w;
				l = m;
			}
		} else if (track_sym(m, rate) == 0 || w == v) {
			l += m;
		} else {
			out.insert(out.end(), (size_t)track_sym(l, rate), (uint8_t)v);
			v = w;
			l = m;
		}
	}
	if (have)
		out.insert(out.end(), (size_t)track_sym(l, rate), (uint8_t)v);
	return out;
}

// bits <file> <start_sample> <n_samples> <burst_samples> <n_bits>[+] <hex|->: MSB-first, the last nibble zero-padded; + when the
// chain is longer than the 2^20 samples kept
inline std::string track_line(const std::string &file, const track_piece &c, long rate)
{
	const std::vector<uint8_t> sy = track_slice(c, rate);
	std::string s = "bits " + file + " " + std::to_string((long long)c.start_sample) + " " + std::to_string(c.n_samples) + " " +
			std::to_string((long long)c.last_over + 1) + " " + std::to_string(sy.size()) + (c.n_samples > kTrackKeep ? "+" : "") + " ";
	if (sy.empty())
		return s + "-";
	for (size_t i = 0; i < sy.size(); i += 4) {
		int nib = 0;
		for (size_t j = 0; j < 4; j++)
			nib = 2 * nib + (i + j < sy.size() ? sy[i + j] : 0);
		s += "0123456789abcdef"[nib];
	}
	return s;
}

// ---- -G rate,auto: the centre record of a track piece (include/tfrec_amd.h: "Auto-centre track", tfrec_amd_track_centre, whose text is
// normative; tfrec_amd/track.py restates the merge and the line)
constexpr int kTrackAutoHead = 1024;  // -G rate,auto's K

// The entry's centre record joins its track piece.  Merging a chain (track_add) leaves it alone: the chain's record is the first
// piece's, and its flags and n_samples are the merged track piece's
inline void centre_take(track_piece &p, const tfrec_amd_track_centre &c)
{
	p.cen = c;
	p.centred = true;
}

// centre <file> <start_sample> <n_samples> <n_counted> <centre_hz> <deviation_hz|-> <m|f|i>: the deviation only of a measured centre;
// i: a chain whose first piece the output does not hold
inline std::string centre_line(const std::string &file, const track_piece &c)
{
	const uint32_t src = c.cen.source <= TFREC_AMD_CENTRE_INHERITED ? c.cen.source : TFREC_AMD_CENTRE_INHERITED;
	return "centre " + file + " " + std::to_string((long long)c.start_sample) + " " + std::to_string(c.n_samples) + " " +
	       std::to_string(c.cen.n_counted) + " " + std::to_string(c.cen.centre_hz) + " " +
	       (src == TFREC_AMD_CENTRE_MEASURED ? std::to_string(c.cen.deviation_hz) : std::string("-")) + " " + "mfi"[src];
}

// ---- -O: the pulses of an amplitude track (include/tfrec_amd.h: "Amplitude track", Pulses, whose text is normative; tfrec_amd/track.py
// restates both)
constexpr size_t kPulsesListed = 64;  // the pulses a line lists

// The maximal runs of equal value of the first min(last_over + 1, 2^20) samples of a merged track, less a leading and a trailing
// run of zeros -> pulse, gap, pulse, ..., pulse in samples (empty: no pulse)
inline std::vector<uint64_t> track_pulses(const track_piece &c)
{
	std::vector<uint64_t> out;
	uint64_t n = c.last_over < 0 ? 0 : std::min<uint64_t>((uint64_t)c.last_over + 1, c.kept());
	uint64_t k = 0;
	while (k < n && !c.bit(k))
		k++;
	while (n > k && !c.bit(n - 1))
		n--;
	while (k < n) {
		const bool w = c.bit(k);
		uint64_t m = 1;
		while (k + m < n && c.bit(k + m) == w)
			m++;
		out.push_back(m);
		k += m;
	}
	return out;
}

// pulses <file> <start_sample> <n_samples> <burst_samples> <n_pulses>[+] <w0,g0,w1,...|->: the first 64 pulses with the gaps between
// them; + when the track holds more
inline std::string pulses_line(const std::string &file, const track_piece &c)
{
	const std::vector<uint64_t> w = track_pulses(c);
	const size_t n = (w.size() + 1) / 2, shown = std::min(w.size(), 2 * kPulsesListed - 1);
	std::string s = "pulses " + file + " " + std::to_string((long long)c.start_sample) + " " + std::to_string(c.n_samples) + " " +
			std::to_string((long long)c.last_over + 1) + " " + std::to_string(std::min(n, kPulsesListed)) + (n > kPulsesListed ? "+" : "") + " ";
	if (!shown)
		return s + "-";
	for (size_t i = 0; i < shown; i++)
		s += (i ? "," : "") + std::to_string(w[i]);
	return s;
}

// ---- -Y: the burst sync's records, match tracks and frames (include/tfrec_amd.h: tfrec_amd_burst_sync, whose text is normative;
// tfrec_amd/sync.py restates merge, the framing and the line)

// a device record, the submit's match bitmap and the entry's track piece -> the piece, as many samples of it as the track piece
// has (the file's end may cut both): n_hits counted again on what is kept of a cut piece; its best and best_at stay if best_at lies
// ahead of the cut and are none (0xffffffff, 0) otherwise -- the minimum over the kept part alone is not known, and no line shows it
inline sync_piece sync_take(const tfrec_amd_burst_sync &r, const uint32_t *words, const track_piece &t)
{
	sync_piece p;
	static_cast<tfrec_amd_burst_sync &>(p) = r;
	p.trk = t;
	p.stream = t.stream;
	p.flags = t.flags;
	const bool cut = t.n_samples < r.n_samples;
	p.n_samples = t.n_samples;
	track_append(p.match, 0, words, r.bit_offset, p.n_samples);
	if (cut) {
		p.n_hits = 0;
		for (uint64_t k = 0; k < p.kept(); k++)
			p.n_hits += p.hit(k);
		if (p.best_at >= p.n_samples) {
			p.best = 0xffffffffu;
			p.best_at = 0;
		}
	}
	return p;
}

// piece p, which CONTINUES the chain c, merged into it (the header's Cutting): the match tracks concatenated, n_samples and n_hits
// added, the smaller best (on a tie the earlier piece's) with its best_at offset by the samples ahead; the track pieces by track_add
inline void sync_add(sync_piece &c, const sync_piece &p)
{
	if (!p.match.empty())
		track_append(c.match, c.kept(), p.match.data(), 0, p.kept());
	if (p.best < c.best) {
		c.best = p.best;
		c.best_at = c.n_samples + p.best_at;
	}
	c.n_samples += p.n_samples;
	c.n_hits += p.n_hits;
	c.flags = (c.flags & TFREC_AMD_RUN_CONTINUES) | (p.flags & TFREC_AMD_RUN_OPEN);
	track_add(c.trk, p.trk);
}

// delta(i) = floor((768000 i + R) / (2 R))
inline uint64_t sync_delta(uint64_t i, long rate) { return (768000 * i + (uint64_t)rate) / (2 * (uint64_t)rate); }

struct sync_frame {
	uint64_t c = 0;    // the plateau's sample, chain-relative
	int errors = 0;
	bool plus = true;  // the polarity
	std::vector<uint8_t> bits;  // the payload, one per byte
};

// The header's Framing on the first min(last_over + 1, 2^20) samples of a chain's merged track and match track
inline std::vector<sync_frame> sync_frames(const sync_piece &c, const job_settings &job)
{
	std::vector<sync_frame> out;
	const int P = job.sync_bits, E = job.sync_errors;
	const uint64_t n = c.trk.last_over < 0 ? 0 : std::min<uint64_t>((uint64_t)c.trk.last_over + 1, c.kept());
	for (uint64_t k = 0; k < n;) {
		if (!c.hit(k)) {
			k++;
			continue;
		}
		uint64_t b = k;
		while (b + 1 < n && c.hit(b + 1))
			b++;
		sync_frame f;
		f.c = (k + b) >> 1;
		int d = 0;
		for (int j = 0; j < P; j++) {
			const uint64_t back = sync_delta((uint64_t)j, job.track_rate);
			const bool t = back <= f.c ? c.trk.bit(f.c - back) : false;  // (ahead of the track: 0)
			d += t != (bool)((job.sync_pattern >> j) & 1ull);
		}
		f.plus = d <= E;
		f.errors = f.plus ? d : P - d;
		for (int i = 1; i <= 8 * job.sync_bytes; i++) {
			const uint64_t q = f.c + sync_delta((uint64_t)i, job.track_rate);
			if (q >= n)
				break;
			f.bits.push_back((uint8_t)(c.trk.bit(q) == f.plus));
		}
		out.push_back(f);
		k = b + 1;
	}
	return out;
}

// frame <file> <start_sample> <sync_sample> <errors> <+|-> <n_bits> <hex|->: MSB-first, the last nibble zero-padded -- or, lsb,
// every byte with the first received bit as bit 0, a last partial byte zero-filled at the top, two digits a byte
inline std::string sync_line(const std::string &file, const sync_piece &c, const sync_frame &f, bool lsb = false)
{
	std::string s = "frame " + file + " " + std::to_string((long long)c.start_sample) + " " + std::to_string((long long)c.start_sample + (long long)f.c) +
			" " + std::to_string(f.errors) + " " + (f.plus ? "+" : "-") + " " + std::to_string(f.bits.size()) + " ";
	if (f.bits.empty())
		return s + "-";
	if (lsb) {
		for (size_t i = 0; i < f.bits.size(); i += 8) {
			int byte = 0;
			for (size_t j = 0; j < 8 && i + j < f.bits.size(); j++)
				byte |= f.bits[i + j] << j;
			s += "0123456789abcdef"[byte >> 4];
			s += "0123456789abcdef"[byte & 15];
		}
		return s;
	}
	for (size_t i = 0; i < f.bits.size(); i += 4) {
		int nib = 0;
		for (size_t j = 0; j < 4; j++)
			nib = 2 * nib + (i + j < f.bits.size() ? f.bits[i + j] : 0);
		s += "0123456789abcdef"[nib];
	}
	return s;
}

// ---- -U: the line code (include/tfrec_amd.h: "Line code", whose text is normative; tfrec_amd/linecode.py restates the span and the line).
// A coded piece is a track_piece: track_take, track_add and chain_merger<track_piece> take it as it is.

// -U's argument: g3ruh | nrzi | nrzs | <1 .. 8 hex digits, not 0>, each with an optional ",inv" -> the taps and INVERT (false: bad)
inline bool code_parse(const char *arg, uint32_t &taps, bool &invert)
{
	std::string a(arg);
	invert = false;
	const size_t comma = a.find(',');
	if (comma != std::string::npos) {
		if (a.substr(comma + 1) != "inv")
			return false;
		invert = true;
		a.resize(comma);
	}
	if (a == "g3ruh") {
		taps = 0x10800u;  // 1 + x^12 + x^17
	} else if (a == "nrzi" || a == "nrzs") {
		taps = 1u;
		invert = invert != (a == "nrzs");  // (nrzs is nrzi complemented)
	} else {
		if (a.empty() || a.size() > 8 || a.find_first_not_of("0123456789abcdefABCDEF") != std::string::npos)
			return false;
		taps = (uint32_t)strtoul(a.c_str(), NULL, 16);
	}
	return taps != 0;
}

// span = delta(the highest set tap), taps != 0
inline uint64_t code_span(uint32_t taps, long rate)
{
	int top = 32;
	while (!((taps >> (top - 1)) & 1u))
		top--;
	return sync_delta((uint64_t)top, rate);
}

// code <file> <start_sample> <n_samples> <burst_samples> <n_bits>[+] <hex|->: -G's bits line of the coded piece
inline std::string code_line(const std::string &file, const track_piece &c, long rate) { return "code" + track_line(file, c, rate).substr(4); }

// ---- -V: the frame check (include/tfrec_amd.h: "Frame check", whose text is normative; tfrec_amd/crc.py restates merge, the verdict and
// the line; ../csrc/crc_table.h holds the settings' rules)

// -V's argument: width,poly[,init[,xorout[,skip[,inv]]]] -- width and skip decimal, poly, init and xorout 1 .. 8 hex digits, inv 0 or
// 1 -> the fields (false: bad).  Whether the settings hold together is tfrec_crc::refusal's to say, once -G's rate and -Y's bytes
// are known.
inline bool crc_parse(const char *arg, int &width, uint32_t &poly, uint32_t &init, uint32_t &xorout, int &skip, bool &invert)
{
	std::vector<std::string> part(1);
	for (const char *q = arg; *q; q++) {
		if (*q == ',')
			part.push_back("");
		else
			part.back() += *q;
	}
	if (part.size() < 2 || part.size() > 6)
		return false;
	for (size_t i = 0; i < part.size(); i++) {
		const bool hex = i >= 1 && i <= 3;
		if (part[i].empty() || part[i].size() > (hex ? 8u : 3u) || part[i].find_first_not_of(hex ? "0123456789abcdefABCDEF" : "0123456789") != std::string::npos)
			return false;
	}
	width = atoi(part[0].c_str());
	poly = (uint32_t)strtoul(part[1].c_str(), NULL, 16);
	init = part.size() > 2 ? (uint32_t)strtoul(part[2].c_str(), NULL, 16) : 0u;
	xorout = part.size() > 3 ? (uint32_t)strtoul(part[3].c_str(), NULL, 16) : 0u;
	skip = part.size() > 4 ? atoi(part[4].c_str()) : 0;
	invert = false;
	if (part.size() > 5) {
		if (part[5] != "0" && part[5] != "1")
			return false;
		invert = part[5] == "1";
	}
	return width != 0;
}

// a device record, the submit's check bitmap and the entry's track piece -> the piece, as many samples of it as the track piece has
// (the file's end may cut both): n_ok and first_at counted again on what is kept of a cut piece
inline crc_piece crc_take(const tfrec_amd_burst_crc &r, const uint32_t *words, const track_piece &t)
{
	crc_piece p;
	static_cast<tfrec_amd_burst_crc &>(p) = r;
	p.stream = t.stream;
	p.flags = t.flags;
	const bool cut = t.n_samples < r.n_samples;
	p.n_samples = t.n_samples;
	track_append(p.ok, 0, words, r.bit_offset, p.n_samples);
	if (cut) {
		p.n_ok = 0;
		p.first_at = 0xffffffffu;
		for (uint64_t k = 0; k < p.kept(); k++) {
			if (!p.bit(k))
				continue;
			if (!p.n_ok++)
				p.first_at = (uint32_t)k;
		}
	}
	return p;
}

// piece p, which CONTINUES the chain c, merged into it (the header's Merging): the check tracks concatenated, n_samples and n_ok
// added, first_at that of the first piece that has one, offset by the samples ahead of it
inline void crc_add(crc_piece &c, const crc_piece &p)
{
	if (!p.ok.empty())
		track_append(c.ok, c.kept(), p.ok.data(), 0, p.kept());
	if (c.first_at == 0xffffffffu && p.first_at != 0xffffffffu)
		c.first_at = c.n_samples + p.first_at;
	c.n_samples += p.n_samples;
	c.n_ok += p.n_ok;
	c.flags = (c.flags & TFREC_AMD_RUN_CONTINUES) | (p.flags & TFREC_AMD_RUN_OPEN);
}

// The header's Verdict: a frame of polarity + with all 8 N payload bits is "ok" iff v[c + D] = 1 on the chain's merged check track,
// else "bad"; any other frame has none, "-".  (c + D is the frame's last bit: inside the input; behind the kept 2^20 samples: none)
inline const char *crc_verdict(const crc_piece &v, const sync_frame &f, int n_bytes, uint64_t D)
{
	if (!f.plus || f.bits.size() != (size_t)(8 * n_bytes) || f.c + D >= v.kept())
		return "-";
	return v.bit(f.c + D) ? "ok" : "bad";
}

// crc <file> <start_sample> <n_samples> <n_ok> <sample|->: the last field is start_sample + first_at - D, where a sync word would
// have ended
inline std::string crc_line(const std::string &file, const crc_piece &c, uint64_t D)
{
	return "crc " + file + " " + std::to_string((long long)c.start_sample) + " " + std::to_string(c.n_samples) + " " + std::to_string(c.n_ok) + " " +
	       (c.first_at == 0xffffffffu ? std::string("-") : std::to_string((long long)c.start_sample + (long long)c.first_at - (long long)D));
}

inline void chain_add(tfrec_amd_burst &c, const tfrec_amd_burst &p) { burst_add(c, p); }
inline void chain_add(crc_piece &c, const crc_piece &p) { crc_add(c, p); }
inline void chain_add(sync_piece &c, const sync_piece &p) { sync_add(c, p); }
inline void chain_add(track_piece &c, const track_piece &p) { track_add(c, p); }
inline void chain_add(tfrec_amd_clock &c, const tfrec_amd_clock &p) { clock_add(c, p); }
inline void chain_add(tfrec_amd_envelope &c, const tfrec_amd_envelope &p) { envelope_add(c, p); }

// The chains of pieces across a job's batches, per file (a record's stream is its file's index in the job).  A chain ends with a
// piece that is not OPEN, with a batch that does not continue it, and with its file: a chain still open at a file's end is flushed
// there.  A chain that the next batch does not continue ended with its last piece's last sample -- the trigger's hold ran out with
// the batch --: its record is complete and OPEN is cleared, as in the record of the uncut run.  take() appends the bursts that ended
// with the batch, in the order in which they ended.
template <class R> struct chain_merger {
	std::vector<R> chain;
	std::vector<char> open, seen;
	std::vector<unsigned long long> blocks;  // of every file, in the batches so far
	void begin(size_t n_files)
	{
		chain.resize(n_files);
		open.assign(n_files, 0);
		seen.assign(n_files, 0);
		blocks.assign(n_files, 0);
	}
	void take(const std::vector<R> &recs, const batch_plan &p, const std::vector<size_t> &file_blocks, std::vector<R> &out)
	{
		for (const R &r : recs) {
			const size_t f = r.stream;
			if ((r.flags & TFREC_AMD_RUN_CONTINUES) && open[f]) {
				chain_add(chain[f], r);
			} else {
				if (open[f]) {
					chain[f].flags &= ~TFREC_AMD_RUN_OPEN;
					out.push_back(chain[f]);
				}
				chain[f] = r;
				open[f] = 1;
			}
			seen[f] = 1;
			if (!(r.flags & TFREC_AMD_RUN_OPEN)) {
				out.push_back(chain[f]);
				open[f] = 0;
			}
		}
		for (int f : p.file) {
			if (f < 0)
				continue;
			blocks[f] += (unsigned long long)p.nb;
			if (open[f] && (!seen[f] || blocks[f] >= file_blocks[f])) {
				if (!seen[f])
					chain[f].flags &= ~TFREC_AMD_RUN_OPEN;
				out.push_back(chain[f]);
				open[f] = 0;
			}
			seen[f] = 0;
		}
	}
};
// -M, -Q, -C and -G take a batch_result's bursts, envelopes, clocks and tracks with chain_merger<R>::take as it is; -Y its syncs:
struct sync_merger : chain_merger<sync_piece> {
	void take(const std::vector<sync_piece> &recs, const batch_plan &p, const std::vector<size_t> &file_blocks, std::vector<sync_piece> &out)
	{
		chain_merger<sync_piece>::take(recs, p, file_blocks, out);
		for (sync_piece &x : out)  // (the merger clears OPEN on the chain's own flags: the track piece's follow)
			x.trk.flags = x.flags;
	}
};

// -s: the scan table (gpu_engine.h: set_scan).  Per channel (file) the sums of its level records, its telegrams, and with -D
// every record; with -M the centre of the channel's burst with the largest pwr_max (the first of them).
struct scan_table {
	struct channel_sum {
		unsigned long long blocks = 0, pwr_sum = 0, over = 0, triggered = 0, telegrams = 0;
		int peak = 0, thresh = 0;
		std::vector<tfrec_amd_level> rec;
		int burst_peak = -1;  // -M: no burst so far
		bool burst_carrier = false;
		long burst_centre = 0;
		void note(const tfrec_amd_burst &r)
		{
			long dev = 0;
			if (r.pwr_max > burst_peak) {
				burst_peak = r.pwr_max;
				burst_carrier = burst_summary(r, burst_centre, dev);
			}
		}
		std::vector<unsigned long long> ratios;  // -Q: ratio_c of the channel's chains that have one
		void note(const tfrec_amd_envelope &r)
		{
			long long len = 0, n_tail = 0;
			unsigned long long ratio = 0;
			if (envelope_summary(r, len, n_tail, ratio))
				ratios.push_back(ratio);
		}
		bool have_clock = false;  // -C: the clock of the channel's chain with the largest quality_c, the earliest among equals
		long long clock_hz = 0;
		unsigned long long clock_quality = 0;
		void note(const tfrec_amd_clock &r)
		{
			long long hz = 0;
			unsigned long long q = 0;
			if (clock_summary(r, hz, q) && (!have_clock || q > clock_quality)) {
				have_clock = true;
				clock_hz = hz;
				clock_quality = q;
			}
		}
		// the median: of an even count the lower of the two in the middle
		bool burst_snr(unsigned long long &ratio) const
		{
			if (ratios.empty())
				return false;
			std::vector<unsigned long long> v(ratios);
			std::sort(v.begin(), v.end());
			ratio = v[(v.size() - 1) / 2];
			return true;
		}
	};
	const job_settings *job;
	const std::vector<file_settings> *settings;
	std::vector<channel_sum> chan;
	scan_table() : job(NULL), settings(NULL) {}
	// the channel list, before a device is opened
	void begin(const job_settings &j, const std::vector<file_settings> &per_file);
	// a batch with its plan; file_blocks: the blocks every file really holds
	void take(const batch_result &b, const batch_plan &p, const std::vector<size_t> &file_blocks)
	{
		for (size_t s = 0; s < p.file.size(); s++) {
			if (p.file[s] < 0)
				continue;
			channel_sum &c = chan[p.file[s]];
			for (int j = 0; j < p.nb && c.blocks < file_blocks[p.file[s]]; j++) {  // (not the padding behind the file's end)
				const tfrec_amd_level &r = b.lv[s * (size_t)p.nb + j];
				c.blocks++;
				c.pwr_sum += r.pwr_sum;
				c.over += (unsigned long long)r.n_over;
				c.triggered += (unsigned long long)r.triggered;
				c.peak = std::max(c.peak, (int)r.pwr_max);
				c.thresh = r.thresh;
				if (job->dbg > 0)
					c.rec.push_back(r);
			}
		}
		for (size_t q = 0; q < b.ev.size(); q++)
			if (b.ev[q].status == 1 && b.ev[q].end_sample < (int64_t)file_blocks[b.ev[q].stream] * TFREC_AMD_BLOCK_DEC)
				chan[b.ev[q].stream].telegrams++;
	}
	void finish() const;
};

#endif
