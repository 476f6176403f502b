// tests/merge_driver.cpp -- tfrec_gpu's pure output code for the five burst stages (tfrec_amd/host/job.h: cut_at_file_end,
// chain_merger, and each stage's take, summary and line functions) behind a text interface, for tests/test_burst_cpu.py,
// test_envelope_cpu.py, test_clock_cpu.py, test_track_cpu.py, test_sync_cpu.py, test_recorder_campaign_cpu.py and
// test_burst_cut_cpu.py.  The stage is the first argument: burst (-M), envelope (-Q), clock (-C), track (-G) or sync (-G -Y).  stdin:
//   rate <bit/s>                                  track: once, first
//   sync <rate> <hex pattern> <n_bits> <errors> <bytes> <both>     sync: once, first
//   file <name> <blocks>                          one per file of the job, in order
//   batch <nb> <file of slot 0> <file of slot 1> ...     (-1: the slot is idle)
//   words <hex word> <hex word> ...               track, sync: the track bitmap of the batch announced last (may be missing: no bits)
//   match <hex word> <hex word> ...               sync: its match bitmap
//   rec <file> ...                                a record of that batch, in table order, as the device delivers it -- but that it
//                                                 names its file: the driver puts it into the batch's slot that holds the file
//                                                 (an idle slot for -1; a slot beyond the map if none does) and applies job.h's
//                                                 file-end cut with the file line's block count, as device_worker does.  By stage:
//     burst     <file> <flags> <start_sample> <n_samples> <thresh> <pwr_max> <n_products> <sum_dot> <sum_crs> <energy> <hist 0> .. <hist 63>
//     envelope  <file> <flags> <start_sample> <n_samples> <thresh> <n_over> <last_over> <energy_head> <energy_tail> <n_gaps> <max_gap>
//               <lead_not_over> <nprod_head> <dot_head> <crs_head> <dot_tail> <crs_tail> <nprod_tail>
//     clock     <file> <flags> <start_sample> <n_samples> <thresh> <n_segments> <n_silent> <spec[0]> ... <spec[127]>
//     track     <file> <flags> <start_sample> <n_samples> <thresh> <bit_offset> <last_over> <n_ones> <kept_samples>
//     sync      <file> <flags> <start_sample> <n_samples> <thresh> <bit_offset> <last_over> <n_ones> <n_hits> <best> <best_at> <kept_samples>
//               kept_samples <= n_samples: what the cut must keep of the record (checked against it)
// stdout, in the order in which the bursts end: the stage's line of each burst (burst, extent, clock, bits); sync: the burst's bits
// line, a line
//   sync <file> <start_sample> <n_samples> <flags> <n_hits> <best> <best_at>
// of the merged sync record, and the burst's frame lines.
#include <stdio.h>
#include <string.h>

#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../tfrec_amd/host/job.h"

// What the protocol has gathered for the batch announced last
struct batch_input {
	std::vector<size_t> blocks;  // of every file
	batch_plan plan;
	std::vector<uint32_t> words, match;
};

// The record as the device names it, then as device_worker keeps it (false: dropped)
template <class R>
static bool cut(R &r, int file, const batch_input &bi, bool cut_opens)
{
	size_t slot = 0;
	while (slot < bi.plan.file.size() && bi.plan.file[slot] != file)
		slot++;
	r.stream = (uint32_t)slot;
	return cut_at_file_end(r, bi.plan.file, bi.blocks, cut_opens);
}

// ---- a stage: its piece and merger, a settings line of its own, a rec line -> the batch's pieces (false: a bad line), a burst's output
struct burst_stage {
	typedef tfrec_amd_burst piece;
	typedef chain_merger<piece> merger;
	bool setting(const std::string &, std::istringstream &) { return false; }
	bool rec(std::istringstream &in, const batch_input &bi, std::vector<piece> &out)
	{
		piece r;
		memset(&r, 0, sizeof(r));
		int file = 0;
		long long start = 0, sd = 0, sc = 0;
		unsigned long long en = 0;
		in >> file >> r.flags >> start >> r.n_samples >> r.thresh >> r.pwr_max >> r.n_products >> sd >> sc >> en;
		r.start_sample = start;
		r.sum_dot = sd;
		r.sum_crs = sc;
		r.energy = en;
		for (int j = 0; j < 64; j++)
			in >> r.hist[j];
		if (!in)
			return false;
		if (cut(r, file, bi, false))
			out.push_back(r);
		return true;
	}
	void print(const std::string &file, const piece &x) const { printf("%s\n", burst_line(file, x).c_str()); }
};

struct envelope_stage {
	typedef tfrec_amd_envelope piece;
	typedef chain_merger<piece> merger;
	bool setting(const std::string &, std::istringstream &) { return false; }
	bool rec(std::istringstream &in, const batch_input &bi, std::vector<piece> &out)
	{
		piece r;
		memset(&r, 0, sizeof(r));
		int file = 0;
		long long start = 0, dh = 0, ch = 0, dt = 0, ct = 0;
		unsigned long long eh = 0, et = 0;
		in >> file >> r.flags >> start >> r.n_samples >> r.thresh >> r.n_over >> r.last_over >> eh >> et >> r.n_gaps >> r.max_gap >>
			r.lead_not_over >> r.nprod_head >> dh >> ch >> dt >> ct >> r.nprod_tail;
		r.start_sample = start;
		r.energy_head = eh;
		r.energy_tail = et;
		r.dot_head = dh;
		r.crs_head = ch;
		r.dot_tail = dt;
		r.crs_tail = ct;
		if (!in)
			return false;
		if (cut(r, file, bi, true))
			out.push_back(r);
		return true;
	}
	void print(const std::string &file, const piece &x) const { printf("%s\n", envelope_line(file, x).c_str()); }
};

struct clock_stage {
	typedef tfrec_amd_clock piece;
	typedef chain_merger<piece> merger;
	bool setting(const std::string &, std::istringstream &) { return false; }
	bool rec(std::istringstream &in, const batch_input &bi, std::vector<piece> &out)
	{
		piece r;
		memset(&r, 0, sizeof(r));
		int file = 0;
		long long start = 0;
		in >> file >> r.flags >> start >> r.n_samples >> r.thresh >> r.n_segments >> r.n_silent;
		r.start_sample = start;
		for (int i = 0; i < 128; i++) {
			unsigned long long v = 0;
			in >> v;
			r.spec[i] = v;
		}
		if (!in)
			return false;
		if (cut(r, file, bi, true))
			out.push_back(r);
		return true;
	}
	void print(const std::string &file, const piece &x) const { printf("%s\n", clock_line(file, x).c_str()); }
};

// A track record's fields and kept_samples, cut -> the piece (track_take is given the device's record and what the cut keeps of
// it).  ok: the line is sound; the result: the record is kept
static bool track_rec(std::istringstream &in, bool with_sync, tfrec_amd_burst_sync &s, const batch_input &bi, bool cut_opens, bool &ok, track_piece &out)
{
	tfrec_amd_track r;
	memset(&r, 0, sizeof(r));
	memset(&s, 0, sizeof(s));
	int file = 0;
	long long start = 0;
	unsigned long long off = 0;
	uint32_t keep = 0;
	in >> file >> r.flags >> start >> r.n_samples >> r.thresh >> off >> r.last_over >> r.n_ones;
	if (with_sync)
		in >> s.n_hits >> s.best >> s.best_at;
	in >> keep;
	r.start_sample = start;
	r.bit_offset = off;
	ok = in && keep <= r.n_samples && off + r.n_samples <= 32ull * bi.words.size() && (!with_sync || off + r.n_samples <= 32ull * bi.match.size());
	if (!ok)
		return false;
	s.stream = r.stream;
	s.flags = r.flags;
	s.start_sample = r.start_sample;
	s.n_samples = r.n_samples;
	s.thresh = r.thresh;
	s.bit_offset = r.bit_offset;
	tfrec_amd_track x = r;
	if (!cut(x, file, bi, cut_opens))
		return false;
	ok = x.n_samples == keep;
	const uint32_t n = x.n_samples;
	x.n_samples = r.n_samples;
	out = track_take(x, bi.words.data(), n);
	return ok;
}

struct track_stage {
	typedef track_piece piece;
	typedef chain_merger<piece> merger;
	long rate;
	track_stage() : rate(0) {}
	bool setting(const std::string &cmd, std::istringstream &in)
	{
		if (cmd != "rate")
			return false;
		in >> rate;
		return true;
	}
	bool rec(std::istringstream &in, const batch_input &bi, std::vector<piece> &out)
	{
		// (not OPEN by the cut, as device_worker would have it: test_track_cpu.py's cut record lies in a file of 4096 blocks of
		// which a few batches come, so the chain of an OPEN piece would never be flushed; the sync stage cuts as device_worker does)
		tfrec_amd_burst_sync s;
		track_piece t;
		bool ok = false;
		if (track_rec(in, false, s, bi, false, ok, t))
			out.push_back(t);
		return ok;
	}
	void print(const std::string &file, const piece &x) const { printf("%s\n", track_line(file, x, rate).c_str()); }
};

struct sync_stage {
	typedef sync_piece piece;
	typedef sync_merger merger;
	job_settings job;
	bool setting(const std::string &cmd, std::istringstream &in)
	{
		if (cmd != "sync")
			return false;
		std::string hex;
		int both = 0;
		in >> job.track_rate >> hex >> job.sync_bits >> job.sync_errors >> job.sync_bytes >> both;
		job.sync_pattern = strtoull(hex.c_str(), NULL, 16);
		job.sync_both = both != 0;
		return true;
	}
	bool rec(std::istringstream &in, const batch_input &bi, std::vector<piece> &out)
	{
		tfrec_amd_burst_sync s;
		track_piece t;
		bool ok = false;
		if (track_rec(in, true, s, bi, true, ok, t))
			out.push_back(sync_take(s, bi.match.data(), t));
		return ok;
	}
	void print(const std::string &file, const piece &x) const
	{
		printf("%s\n", track_line(file, x.trk, job.track_rate).c_str());
		printf("sync %s %lld %u %u %u %u %u\n", file.c_str(), (long long)x.start_sample, x.n_samples, x.flags, x.n_hits, x.best, x.best_at);
		for (const sync_frame &f : sync_frames(x, job))
			printf("%s\n", sync_line(file, x, f).c_str());
	}
};

// ---- the protocol, once
// the batch announced last: the bursts that ended with it
template <class Stage>
static void flush(const Stage &stage, typename Stage::merger &m, std::vector<typename Stage::piece> &recs, const batch_input &bi,
		  const std::vector<std::string> &names)
{
	std::vector<typename Stage::piece> out;
	m.take(recs, bi.plan, bi.blocks, out);
	for (const typename Stage::piece &x : out)
		stage.print(names[x.stream], x);
	recs.clear();
}

template <class Stage>
static int run()
{
	Stage stage;
	typename Stage::merger m;
	std::vector<typename Stage::piece> recs;
	std::vector<std::string> names;
	batch_input bi;
	bool have = false;
	std::string line;
	while (std::getline(std::cin, line)) {
		std::istringstream in(line);
		std::string cmd;
		in >> cmd;
		if (cmd == "file") {
			std::string name;
			size_t nb = 0;
			in >> name >> nb;
			names.push_back(name);
			bi.blocks.push_back(nb);
		} else if (cmd == "batch") {
			if (have)
				flush(stage, m, recs, bi, names);
			else
				m.begin(names.size());
			have = true;
			bi.plan = batch_plan();
			bi.words.clear();
			bi.match.clear();
			in >> bi.plan.nb;
			for (int f; in >> f;)
				bi.plan.file.push_back(f);
		} else if (cmd == "words" || cmd == "match") {
			for (std::string w; in >> w;)
				(cmd == "words" ? bi.words : bi.match).push_back((uint32_t)strtoul(w.c_str(), NULL, 16));
		} else if (cmd == "rec") {
			if (!stage.rec(in, bi, recs)) {
				fprintf(stderr, "bad rec line\n");
				return 1;
			}
		} else {
			stage.setting(cmd, in);
		}
	}
	if (have)
		flush(stage, m, recs, bi, names);
	return 0;
}

int main(int argc, char **argv)
{
	const std::string stage = argc > 1 ? argv[1] : "";
	if (stage == "burst")
		return run<burst_stage>();
	if (stage == "envelope")
		return run<envelope_stage>();
	if (stage == "clock")
		return run<clock_stage>();
	if (stage == "track")
		return run<track_stage>();
	if (stage == "sync")
		return run<sync_stage>();
	fprintf(stderr, "usage: merge_driver burst|envelope|clock|track|sync < lines\n");
	return 2;
}
