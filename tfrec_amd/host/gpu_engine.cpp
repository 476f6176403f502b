// tfrec_amd/host/gpu_engine.cpp -- see gpu_engine.h.
#include "gpu_engine.h"

#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <deque>

#include "device_worker.h"

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

std::vector<decoder *> make_decoders(int types, batch_sink *const *sink, int stream)
{
	std::vector<decoder *> d(TFREC_AMD_NSLOTS, (decoder *)NULL);
	if (types & (1 << TFA_1)) d[TFREC_AMD_SLOT_TFA1] = new sinked_decoder<tfa1_decoder>(TFA_1, sink, stream);
	if (types & (1 << TFA_2)) d[TFREC_AMD_SLOT_TFA2] = new sinked_decoder<tfa2_decoder>(TFA_2, sink, stream);
	if (types & (1 << TFA_3)) d[TFREC_AMD_SLOT_TFA3] = new sinked_decoder<tfa2_decoder>(TFA_3, sink, stream);
	if (types & (1 << TX22)) d[TFREC_AMD_SLOT_TX22] = new sinked_decoder<tfa2_decoder>(TX22, sink, stream);
	if (types & (1 << TFA_WHB)) d[TFREC_AMD_SLOT_WHB] = new sinked_decoder<whb_decoder>(TFA_WHB, sink, stream);
	return d;
}

gpu_engine::gpu_engine(const std::vector<std::string> &dumpfiles, int types, int thresh, int filter, int dbg,
		       const std::vector<int> &_devices, int blocks_per_submit, const std::vector<file_settings> &per_file)
	: files(dumpfiles), settings(per_file), dflt(file_settings{ types, thresh, filter, 0 }), bps(blocks_per_submit), devices(_devices),
	  n_telegrams(0), sink(NULL), psink(NULL), out_mode(0)
{
	job.dbg = dbg;
	if (devices.empty())
		devices.push_back(0);
	if (settings.size() != files.size())
		settings.assign(files.size(), dflt);
	// one set of protocol handlers per stream (with the file's own -T)
	for (size_t s = 0; s < files.size(); s++) {
		decs.push_back(make_decoders(settings[s].types, &sink, (int)s));
		for (decoder *d : decs.back())
			if (d)
				d->set_params(NULL, 0, dbg);
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

void gpu_engine::set_handler(const char *exec, bool batched, int mode)
{
	out_mode = mode;
	if (batched && exec && *exec)
		sink = psink = new pipe_sink(exec);
	for (size_t s = 0; s < decs.size(); s++)
		for (size_t k = 0; k < decs[s].size(); k++)
			if (decs[s][k])
				decs[s][k]->set_params(batched ? NULL : (char *)exec, mode, job.dbg);
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
	if (!job.bits_replay) {
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

// ---- the output modes' consumers (job.h): what they print and write

// -S: <prefix>.idx and the files' <prefix>.<file>.cs16 and .pre (gpu_engine.h: set_capture)
struct capture_writer {
	std::string prefix;
	FILE *idx;
	std::vector<bool> made;  // which files' .cs16 exist already
	capture_writer() : idx(NULL) {}
	int begin(const job_settings &job, size_t n_files)
	{
		prefix = job.cap_prefix;
		made.assign(n_files, false);
		if ((idx = fopen((prefix + ".idx").c_str(), "w")))
			return 0;
		perror((prefix + ".idx").c_str());
		return TFREC_AMD_E_INVAL;
	}
	int take(const batch_result &b)
	{
		int rc = 0;
		for (size_t q = 0; q < b.runs.size() && rc == 0;) {  // the runs of one file are adjacent (the table is ordered by stream)
			const int f = b.file[q];
			const std::string path = prefix + "." + std::to_string(f) + ".cs16";
			FILE *fp = fopen(path.c_str(), made[f] ? "ab" : "wb");
			if (!fp) {
				perror(path.c_str());
				return TFREC_AMD_E_INVAL;
			}
			const std::string pre_path = prefix + "." + std::to_string(f) + ".pre";
			FILE *pp = fopen(pre_path.c_str(), made[f] ? "ab" : "wb");
			if (!pp) {
				perror(pre_path.c_str());
				fclose(fp);
				return TFREC_AMD_E_INVAL;
			}
			made[f] = true;
			for (; q < b.runs.size() && b.file[q] == f; q++) {
				const tfrec_amd_run &x = b.runs[q];
				fprintf(idx, "%d %u %lld %u %d %u\n", f, (unsigned)x.stream, (long long)x.start_sample, (unsigned)x.n_samples, (int)x.thresh,
					(unsigned)x.flags);
				if (fwrite(b.pool.data() + 2 * (size_t)x.pool_offset, 4, x.n_samples, fp) != x.n_samples ||
				    fwrite(b.pre.data() + 2 * q, 4, 1, pp) != 1)
					rc = TFREC_AMD_E_INVAL;
			}
			if (fclose(fp))
				rc = TFREC_AMD_E_INVAL;
			if (fclose(pp))
				rc = TFREC_AMD_E_INVAL;
		}
		return rc;
	}
	int finish() { return idx && fclose(idx) ? TFREC_AMD_E_INVAL : 0; }
};

// -z -D: the "dc" lines (gpu_engine.h: set_dc); they hold no state, so there is nothing to begin or to finish
struct dc_report {
	void take(const batch_result &b, const std::vector<std::string> &files) const
	{
		for (size_t q = 0; q < b.dc_file.size(); q++)
			printf("dc %s I=%d Q=%d\n", files[b.dc_file[q]].c_str(), (int)b.dc_last[2 * q], (int)b.dc_last[2 * q + 1]);
		for (size_t q = 0; q < b.iq_file.size(); q++)  // -Z -D (set_iq)
			printf("iq %s t=%d g=%d\n", files[b.iq_file[q]].c_str(), (int)b.iq_last[2 * q], (int)b.iq_last[2 * q + 1]);
	}
};

// -Y's frame line; with -V its verdict as one more field (job.h: crc_verdict) on the check piece of the same burst: checked[i]
// belongs to the i-th burst that ended with the batch -- the mergers see the same flags, so the chains end together, in one order
static std::string frame_line(const std::string &file, const sync_piece &x, const sync_frame &f, const job_settings &job,
			      const std::vector<crc_piece> &checked, size_t i, uint64_t crc_reach)
{
	std::string s = sync_line(file, x, f, job.sync_lsb);
	if (job.checking())
		s += std::string(" ") + crc_verdict(checked.at(i), f, job.sync_bytes, crc_reach);
	return s;
}

// -M, -Q, -C: a stage's chains across the batches (job.h: chain_merger); take() sends the bursts that ended with a batch into the
// scan table, or prints the stage's line for each
template <class R>
struct chain_report : chain_merger<R> {
	std::string (*line)(const std::string &file, const R &r);
	std::vector<R> ended;
	explicit chain_report(std::string (*l)(const std::string &, const R &)) : line(l) {}
	void take(const std::vector<R> &recs, const batch_plan &p, const std::vector<size_t> &file_blocks, const std::vector<std::string> &files,
		  scan_table *scan)
	{
		ended.clear();
		chain_merger<R>::take(recs, p, file_blocks, ended);
		for (const R &x : ended) {
			if (scan)
				scan->chan[x.stream].note(x);
			else
				printf("%s\n", line(files[x.stream], x).c_str());
		}
	}
};

void spectrum_table::begin(const job_settings &job)
{
	n = job.spec_n;
	keep = job.dbg > 0;
	khz.resize(n);
	order.resize(n);
	total.assign(n, 0);
	peak.assign(n, 0);
	fprintf(stderr, "spec: %d bins, %d frames per record, input rate %ld S/s\n", n, job.spec_g, job.fs_in());
	for (int i = 0; i < n; i++) {
		const int k = (i + n / 2) % n;
		order[i] = k;
		khz[k] = job.spec_center + (double)((long)(k < n / 2 ? k : k - n) * job.fs_in()) / n / 1000.0;
		fprintf(stderr, "spec bin %.3f kHz\n", khz[k]);
	}
}

void spectrum_table::finish() const
{
	for (size_t q = 0; q < rec_frames.size(); q++)
		for (int k : order)
			printf("spec-rec %zu %.3f sum=%llu peak=%llu frames=%u\n", q, khz[k], (unsigned long long)rec_sum[q * n + k],
			       (unsigned long long)rec_peak[q * n + k], (unsigned)rec_frames[q]);
	for (int k : order)
		printf("spec %.3f mean=%llu peak=%llu\n", khz[k], frames ? (unsigned long long)(total[k] / frames) : 0ull,
		       (unsigned long long)peak[k]);
}

void occupancy_list::begin(const job_settings &j)
{
	job = &j;
	hits.assign(j.spec_n, 0);
	fprintf(stderr, "occ: ratio %d, rel %d, join %ld Hz\n", j.occ_ratio, j.occ_rel, j.occ_join);
}

int occupancy_list::finish()
{
	for (const occ_channel &c : occupancy_channels(hits, records, job->spec_n, job->fs_in(), job->spec_center, job->occ_join)) {
		if (c.carrier) {
			printf("carrier %ld hits=%llu/%llu\n", c.khz, c.hits, records);
			continue;
		}
		printf("found %ld bins=%d..%d hits=%llu/%llu%s\n", c.khz, c.lo, c.hi, c.hits, records, c.in_range ? "" : " out-of-range");
		if (c.in_range)
			found.push_back(c.khz);
	}
	if (found.size() <= 4096)
		return 0;
	fprintf(stderr, "tfrec_gpu: -A found %zu channels, at most 4096 are scanned at once\n", found.size());
	return TFREC_AMD_E_INVAL;
}

void scan_table::begin(const job_settings &j, const std::vector<file_settings> &per_file)
{
	job = &j;
	settings = &per_file;
	chan.assign(per_file.size(), channel_sum());
	fprintf(stderr, "scan: %zu channels, input rate %ld S/s\n", chan.size(), j.fs_in());
	for (size_t s = 0; s < chan.size(); s++) {
		const int hz = per_file[s].tune;
		const bool far = !j.wide && (hz <= -768000 || hz >= 768000);
		fprintf(stderr, "scan channel %ld kHz: tune %d Hz %s\n", j.scan_khz[s], hz,
			hz == 0 ? "(none)" : j.wide ? "ahead of the 10:1 stage" : far ? "ahead of the resampler" : j.resampled() ? "behind the resampler" : "in the front end");
	}
}

void scan_table::finish() const
{
	for (size_t s = 0; s < chan.size(); s++) {
		const channel_sum &c = chan[s];
		for (const tfrec_amd_level &r : c.rec)  // fm_demod.cpp:61, per channel
			printf("%ld Trigger ratio %d/%d, avg %d\n", job->scan_khz[s], (int)r.triggered, TFREC_AMD_BLOCK_DEC, (int)r.triggered_avg);
		printf("scan %ld blocks=%llu mean_pwr=%llu peak=%d over=%llu triggered=%llu thresh=%d telegrams=%llu", job->scan_khz[s], c.blocks,
		       c.blocks ? c.pwr_sum / ((unsigned long long)TFREC_AMD_BLOCK_DEC * c.blocks) : 0ull, c.peak, c.over, c.triggered,
		       c.blocks ? c.thresh : ((*settings)[s].thresh ? (*settings)[s].thresh : 500), c.telegrams);
		if (job->metering() && c.burst_carrier)  // -M: where the channel's strongest burst sits relative to the channel, in Hz
			printf(" burst_centre=%ld", c.burst_centre);
		else if (job->metering())
			printf(" burst_centre=-");
		unsigned long long ratio = 0;
		if (job->enveloping() && c.burst_snr(ratio))  // -Q: the median ratio_c of the channel's bursts that have one
			printf(" burst_snr=%llu.%02llu", ratio / 100, ratio % 100);
		else if (job->enveloping())
			printf(" burst_snr=-");
		if (job->clocking() && c.have_clock)  // -C: the clock of the channel's burst with the largest quality_c
			printf(" burst_clock=%lld", c.clock_hz);
		else if (job->clocking())
			printf(" burst_clock=-");
		printf("\n");
	}
}

// -A with -D: the file's records of a batch, `count` of them, the first being record `first` of the file
static void print_occ_records(const batch_result &b, unsigned long long first, size_t count)
{
	for (size_t q = 0; q < count; q++)
		printf("occ-rec %llu floor=%llu hits=%u frames=%u\n", first + q, (unsigned long long)b.occ_recs[q].floor,
		       (unsigned)b.occ_recs[q].n_hit, (unsigned)b.occ_recs[q].n_frames);
}

// per stream in time order, slots in registration order like the reference's dispatch loop (fm_demod.cpp:48-49).
// BITS chunks carry the first sample of their trigger window (a chunk has no per-bit time): a window's bits
// are replayed when it opens, its flush when it closes -- what store_bit prints keeps its place among the
// flushes of every window that does not overlap this one.
static bool replays_before(const tfrec_amd_event &a, const tfrec_amd_event &b)
{
	if (a.stream != b.stream) return a.stream < b.stream;
	if (a.end_sample != b.end_sample) return a.end_sample < b.end_sample;
	const bool ab = a.status == TFREC_AMD_STATUS_BITS, bb = b.status == TFREC_AMD_STATUS_BITS;
	if (ab != bb) return ab;
	if (a.slot != b.slot) return a.slot < b.slot;
	return ab && a.offset < b.offset;
}

// -K: a whole file into `to` -> whether it could be read (must: a missing file is reported)
static bool read_whole(const std::string &path, std::vector<uint8_t> &to, bool must)
{
	to.clear();
	FILE *f = fopen(path.c_str(), "rb");
	if (!f) {
		if (must)
			perror(path.c_str());
		return false;
	}
	uint8_t buf[65536];
	for (size_t got; (got = fread(buf, 1, sizeof(buf), f)) > 0;)
		to.insert(to.end(), buf, buf + got);
	const bool ok = !ferror(f);
	fclose(f);
	if (!ok)
		perror(path.c_str());
	return ok;
}

// -k: file s's <prefix>.<s>.rest -- the last bytes of (the head carried in, the file) that filled no piece -- and, for a file that
// ran nothing, the .state it continued from
static int write_kept_rest(const job_settings &job, size_t s, const std::string &file, const kept_bytes &k)
{
	const kept_input *in = job.cont ? &(*job.cont)[s] : NULL;
	const std::string path = job_settings::kept_path(job.keep_prefix, s, ".rest");
	std::vector<uint8_t> rest;
	if (in)
		rest.assign(in->rest.end() - (long)k.rest_head, in->rest.end());
	rest.resize(k.rest_head + k.rest_file);
	FILE *f = fopen(file.c_str(), "rb");
	bool ok = f && fseek(f, -(long)k.rest_file, SEEK_END) == 0 && fread(rest.data() + k.rest_head, 1, k.rest_file, f) == k.rest_file;
	if (f)
		fclose(f);
	if (!ok) {
		perror(file.c_str());
		return TFREC_AMD_E_INVAL;
	}
	FILE *o = fopen(path.c_str(), "wb");
	ok = o && fwrite(rest.data(), 1, rest.size(), o) == rest.size();
	if (o && fclose(o))
		ok = false;
	if (ok && k.blocks == 0 && in) {  // nothing ran: the state goes on unchanged
		const std::string sp = job_settings::kept_path(job.keep_prefix, s, ".state");
		FILE *so = fopen(sp.c_str(), "wb");
		ok = so && fwrite(in->state.data(), 1, in->state.size(), so) == in->state.size();
		if (so && fclose(so))
			ok = false;
	}
	if (!ok) {
		perror(path.c_str());
		return TFREC_AMD_E_INVAL;
	}
	return 0;
}

// One worker (host thread + context + HIP streams) per device entry, streams sharded by index over them; this thread
// takes the devices' events batch by batch, in device = stream order, and replays them into the decoders: stdout and
// the handler records come out in the order of a single-device run whatever the number of devices.
int gpu_engine::run()
{
	const size_t n = files.size();
	std::vector<size_t> file_blocks(n, 0);
	stream_samples.assign(n, 0);
	const size_t piece = job.piece_bytes();
	const int unit = job.unit();
	for (size_t s = 0; s < n && job.replay; s++) {  // -R: a capture is as long as its last run reaches
		file_blocks[s] = (*job.replay)[s].blocks();
		stream_samples[s] = (long long)file_blocks[s] * TFREC_AMD_BLOCK_DEC;
	}
	std::vector<kept_input> cont(job.continuing() ? n : 0);  // -K: every file's state and rest, before a device is opened
	for (size_t s = 0; s < cont.size(); s++) {
		if (!read_whole(job_settings::kept_path(job.cont_prefix, s, ".state"), cont[s].state, true) ||
		    cont[s].state.size() < sizeof(tfrec_amd_state_header))
			return TFREC_AMD_E_INVAL;
		read_whole(job_settings::kept_path(job.cont_prefix, s, ".rest"), cont[s].rest, false);
		tfrec_amd_state_header h;  // the saved settings are the stream's: this run's must not ask for others
		memcpy(&h, cont[s].state.data(), sizeof(h));
		const file_settings &fs = settings[s];
		if (h.config.types_mask != fs.types || h.config.thresh != fs.thresh || h.config.filter_type != fs.filter) {
			fprintf(stderr, "%s: kept with -T %x -t %d%s, this run asks for -T %x -t %d%s\n",
				job_settings::kept_path(job.cont_prefix, s, ".state").c_str(), (unsigned)h.config.types_mask, (int)h.config.thresh,
				h.config.filter_type ? " -W" : "", (unsigned)fs.types, fs.thresh, fs.filter ? " -W" : "");
			return TFREC_AMD_E_INVAL;
		}
	}
	job.cont = job.continuing() ? &cont : NULL;
	std::vector<kept_bytes> kept(n);
	for (size_t s = 0; s < n && !job.replay; s++) {
		FILE *f = fopen(files[s].c_str(), "rb");
		if (!f) {
			perror(files[s].c_str());
			return TFREC_AMD_E_INVAL;
		}
		fseek(f, 0, SEEK_END);
		// trailing partial block dropped, engine.cpp:72-76 (-r: a trailing partial piece of `unit` blocks; -k keeps it for the next
		// part, -K reads the last part's ahead of the file)
		kept[s] = plan_kept_bytes(cont.empty() ? 0 : cont[s].rest.size(), (size_t)ftell(f), piece, unit);
		const size_t blocks = kept[s].blocks;
		fclose(f);
		if (job.dbg > 0 && job.fmt != TFREC_AMD_FMT_U8)  // -D with -F: how the file is cut
			fprintf(stderr, "%s: %zu blocks, %zu bytes per %d\n", files[s].c_str(), blocks, piece, unit);
		// (-K: end_sample goes on counting from the saved sample count)
		stream_samples[s] = (cont.empty() ? 0 : cont[s].samples()) + (long long)blocks * TFREC_AMD_BLOCK_DEC;
		file_blocks[s] = blocks;
	}
	// what the output modes say before a device is opened
	capture_writer cap;
	dc_report dc;
	spectrum_table spec;
	occupancy_list occ;
	scan_table scan;
	chain_report<tfrec_amd_burst> bursts(burst_line);
	bursts.begin(n);
	chain_report<tfrec_amd_envelope> envelopes(envelope_line);
	envelopes.begin(n);
	chain_report<tfrec_amd_clock> clocks(clock_line);
	clocks.begin(n);
	chain_merger<track_piece> tracks, codes;
	std::vector<track_piece> said, coded;
	tracks.begin(n);
	codes.begin(n);
	sync_merger syncs;
	std::vector<sync_piece> framed;
	syncs.begin(n);
	chain_merger<crc_piece> crcs;
	std::vector<crc_piece> checked;
	crcs.begin(n);
	const uint64_t crc_reach = job.checking() ? (uint64_t)tfrec_crc::reach(job.crc_settings()) : 0;
	if (job.spectrum)
		spec.begin(job);
	if (job.occupancy())
		occ.begin(job);
	if (job.scan)
		scan.begin(job, settings);
	if (job.capture && cap.begin(job, n))
		return TFREC_AMD_E_INVAL;
	const size_t nd = std::min(devices.size(), n);  // never more workers than streams
	const int blocks = (bps + unit - 1) / unit * unit;
	std::atomic<bool> abort(false);  // set when any worker failed: the others stop instead of running the whole job
	std::deque<device_worker> workers;
	size_t n_batches = 0;  // of the device with the most
	for (size_t d = 0; d < nd; d++) {
		size_t s0, s1;
		shard_range(n, nd, d, s0, s1);
		workers.emplace_back(job, files, file_blocks, settings, dflt, devices[d], s0, s1, blocks, abort);
		n_batches = std::max(n_batches, workers.back().plan.size());
	}
	for (device_worker &w : workers)
		w.start();
	int rc = 0;
	batch_result b;
	for (size_t k = 0; k < n_batches && rc == 0; k++) {
		for (size_t d = 0; d < nd && rc == 0; d++) {
			if (k >= workers[d].plan.size())
				continue;  // (this device's queue has run out)
			if (!workers[d].pop(b)) {
				rc = workers[d].rc ? workers[d].rc : TFREC_AMD_E_STATE;
				break;
			}
			if ((rc = cap.take(b)))
				break;
			dc.take(b, files);
			scan_table *const into = job.scan ? &scan : NULL;
			if (job.metering())  // -M: the bursts that ended with this batch -- into the scan table, or a line each
				bursts.take(b.bursts, workers[d].plan[k], file_blocks, files, into);
			if (job.enveloping())  // -Q: likewise, behind -M's lines of the batch
				envelopes.take(b.envelopes, workers[d].plan[k], file_blocks, files, into);
			if (job.clocking())  // -C: likewise, behind -Q's lines of the batch
				clocks.take(b.clocks, workers[d].plan[k], file_blocks, files, into);
			checked.clear();
			if (job.checking())  // -V (with -Y): the check pieces of the sync's entries -- the same flags, so the chains end together, in one order
				crcs.take(b.crcs, workers[d].plan[k], file_blocks, checked);
			if (job.coding()) {  // -G -U: -G's lines of each burst, its code line, and with -Y a line per frame found on the coded track
				said.clear();
				tracks.take(b.tracks, workers[d].plan[k], file_blocks, said);
				framed.clear();
				coded.clear();
				if (job.syncing())
					syncs.take(b.syncs, workers[d].plan[k], file_blocks, framed);
				else
					codes.take(b.codes, workers[d].plan[k], file_blocks, coded);
				if (job.checking() && checked.size() != framed.size()) {
					fprintf(stderr, "tfrec_amd: batch %zu: %zu check chains ended beside %zu sync chains\n", k, checked.size(), framed.size());
					rc = TFREC_AMD_E_STATE;
					break;
				}
				for (size_t i = 0; i < said.size(); i++) {  // (the same entries with the same flags: the chains end together, in one order)
					const track_piece &x = said[i];
					if (job.centring())
						printf("%s\n", centre_line(files[x.stream], x).c_str());
					printf("%s\n", track_line(files[x.stream], x, job.track_rate).c_str());
					if (job.amplitude())
						printf("%s\n", pulses_line(files[x.stream], x).c_str());
					printf("%s\n", code_line(files[x.stream], job.syncing() ? framed[i].trk : coded[i], job.track_rate).c_str());
					if (job.syncing())
						for (const sync_frame &f : sync_frames(framed[i], job))
							printf("%s\n", frame_line(files[x.stream], framed[i], f, job, checked, i, crc_reach).c_str());
					if (job.checking())  // -V: the burst's crc line behind its frame lines
						printf("%s\n", crc_line(files[x.stream], checked[i], crc_reach).c_str());
				}
			} else if (job.syncing()) {  // -G -Y: -G's line of each burst, and behind it a line per frame found in it
				framed.clear();
				syncs.take(b.syncs, workers[d].plan[k], file_blocks, framed);
				if (job.checking() && checked.size() != framed.size()) {
					fprintf(stderr, "tfrec_amd: batch %zu: %zu check chains ended beside %zu sync chains\n", k, checked.size(), framed.size());
					rc = TFREC_AMD_E_STATE;
					break;
				}
				for (size_t i = 0; i < framed.size(); i++) {
					const sync_piece &x = framed[i];
					if (job.centring())  // -G rate,auto and -G rate,psk: the burst's centre ahead of its bits
						printf("%s\n", centre_line(files[x.stream], x.trk).c_str());
					printf("%s\n", track_line(files[x.stream], x.trk, job.track_rate).c_str());
					if (job.amplitude())  // -O: the burst's pulses behind its bits
						printf("%s\n", pulses_line(files[x.stream], x.trk).c_str());
					for (const sync_frame &f : sync_frames(x, job))
						printf("%s\n", frame_line(files[x.stream], x, f, job, checked, i, crc_reach).c_str());
					if (job.checking())  // -V: the burst's crc line behind its frame lines
						printf("%s\n", crc_line(files[x.stream], checked[i], crc_reach).c_str());
				}
			} else if (job.tracking()) {  // -G: likewise, behind -C's lines of the batch
				said.clear();
				tracks.take(b.tracks, workers[d].plan[k], file_blocks, said);
				for (const track_piece &x : said) {
					if (job.centring())
						printf("%s\n", centre_line(files[x.stream], x).c_str());
					printf("%s\n", track_line(files[x.stream], x, job.track_rate).c_str());
					if (job.amplitude())
						printf("%s\n", pulses_line(files[x.stream], x).c_str());
				}
			}
			if (job.occupancy()) {  // no replay: the channel list is the product
				const unsigned long long first = occ.records;
				const size_t count = occ.take(b, workers[d].plan[k].nb, file_blocks[0]);
				if (job.dbg > 0)
					print_occ_records(b, first, count);
				continue;
			}
			if (job.spectrum)
				spec.take(b);
			if (job.scan) {  // no replay: the table is the product
				scan.take(b, workers[d].plan[k], file_blocks);
				continue;
			}
			std::stable_sort(b.ev.begin(), b.ev.end(), replays_before);
			for (size_t q = 0; q < b.ev.size(); q++)
				if (b.ev[q].end_sample < stream_samples[b.ev[q].stream])
					replay(b.ev[q]);
		}
		if (psink)
			psink->flush();  // the records of the whole batch in one write
	}
	// (after an error: tell the healthy workers to stop, and empty the queues so that they can finish)
	if (rc)
		abort.store(true);
	for (device_worker &w : workers) {
		while (w.pop(b)) {
		}
		w.th.join();
		if (!rc)
			rc = w.rc;
	}
	if (cap.finish() && !rc)
		rc = TFREC_AMD_E_INVAL;
	for (size_t s = 0; s < n && job.keeping() && !rc; s++)  // -k: what is left of every file for its next part
		rc = write_kept_rest(job, s, files[s], kept[s]);
	job.cont = NULL;
	if (job.scan && !rc)
		scan.finish();
	if (out_mode)  // -m 1: summary at the end (decoder.cpp:98-109)
		for (size_t s = 0; s < decs.size(); s++)
			for (size_t k2 = 0; k2 < decs[s].size(); k2++)
				if (decs[s][k2])
					decs[s][k2]->flush_storage();
	occ_found.clear();
	if (job.occupancy() && !rc) {  // -A: the channel list
		rc = occ.finish();
		occ_found = occ.found;
	}
	if (job.spectrum && !job.occupancy() && !rc)  // -P: behind the telegram output
		spec.finish();
	if (psink)
		psink->flush();
	return rc;
}
