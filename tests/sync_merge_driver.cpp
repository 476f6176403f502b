// tests/sync_merge_driver.cpp -- tfrec_gpu -G -Y's pure output code (tfrec_amd/host/job.h: track_take, sync_take, sync_merger,
// sync_frames, sync_line) behind a text interface, for tests/test_sync_cpu.py.  stdin:
//   sync <rate> <hex pattern> <n_bits> <errors> <bytes> <both>     once, first
//   file <name> <blocks>                          one per file of the job, in order
//   batch <nb> <file of slot 0> <file of slot 1> ...     (-1: the slot is idle)
//   words <hex word> <hex word> ...               the track bitmap of the batch announced last (may be missing: no bits)
//   match <hex word> <hex word> ...               its match bitmap
//   rec <file> <flags> <start_sample> <n_samples> <thresh> <bit_offset> <last_over> <n_ones> <n_hits> <best> <best_at> <kept_samples>
//                                                 the track and sync records of an entry of that batch, in table order;
//                                                 kept_samples <= n_samples: where the file's end cuts it
// stdout, in the order in which the bursts end: the burst's bits line, a line
//   sync <file> <start_sample> <n_samples> <flags> <n_hits> <best> <best_at>
// of the merged sync record, and the burst's frame lines.
#include <stdio.h>
#include <string.h>

#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../tfrec_amd/host/job.h"

static void flush(sync_merger &m, batch_result &b, const batch_plan &p, const std::vector<size_t> &blocks, const std::vector<std::string> &names,
		  const job_settings &job)
{
	std::vector<sync_piece> out;
	m.take(b, p, blocks, out);
	for (const sync_piece &x : out) {
		printf("%s\n", track_line(names[x.stream], x.trk, job.track_rate).c_str());
		printf("sync %s %lld %u %u %u %u %u\n", names[x.stream].c_str(), (long long)x.start_sample, x.n_samples, x.flags, x.n_hits, x.best,
		       x.best_at);
		for (const sync_frame &f : sync_frames(x, job))
			printf("%s\n", sync_line(names[x.stream], x, f).c_str());
	}
	b.syncs.clear();
}

int main()
{
	std::vector<std::string> names;
	std::vector<size_t> blocks;
	std::vector<uint32_t> words, match;
	sync_merger m;
	batch_result b;
	batch_plan p;
	job_settings job;
	bool have = false;
	std::string line;
	while (std::getline(std::cin, line)) {
		std::istringstream in(line);
		std::string cmd;
		in >> cmd;
		if (cmd == "sync") {
			std::string hex;
			int both = 0;
			in >> job.track_rate >> hex >> job.sync_bits >> job.sync_errors >> job.sync_bytes >> both;
			job.sync_pattern = strtoull(hex.c_str(), NULL, 16);
			job.sync_both = both != 0;
		} else if (cmd == "file") {
			std::string name;
			size_t nb = 0;
			in >> name >> nb;
			names.push_back(name);
			blocks.push_back(nb);
		} else if (cmd == "batch") {
			if (have)
				flush(m, b, p, blocks, names, job);
			else
				m.begin(names.size());
			have = true;
			p = batch_plan();
			words.clear();
			match.clear();
			in >> p.nb;
			for (int f; in >> f;)
				p.file.push_back(f);
		} else if (cmd == "words" || cmd == "match") {
			for (std::string w; in >> w;)
				(cmd == "words" ? words : match).push_back((uint32_t)strtoul(w.c_str(), NULL, 16));
		} else if (cmd == "rec") {
			tfrec_amd_track r;
			tfrec_amd_burst_sync s;
			memset(&r, 0, sizeof(r));
			memset(&s, 0, sizeof(s));
			long long start = 0;
			unsigned long long off = 0;
			uint32_t keep = 0;
			in >> r.stream >> r.flags >> start >> r.n_samples >> r.thresh >> off >> r.last_over >> r.n_ones >> s.n_hits >> s.best >> s.best_at >> keep;
			r.start_sample = start;
			r.bit_offset = off;
			if (!in || keep > r.n_samples || off + r.n_samples > 32ull * words.size() || off + r.n_samples > 32ull * match.size()) {
				fprintf(stderr, "bad rec line\n");
				return 1;
			}
			s.stream = r.stream;
			s.flags = r.flags;
			s.start_sample = r.start_sample;
			s.n_samples = r.n_samples;
			s.thresh = r.thresh;
			s.bit_offset = r.bit_offset;
			tfrec_amd_track x = r;
			if (keep < r.n_samples)  // (as device_worker::read_tracks marks a record that the file's end cuts)
				x.flags |= TFREC_AMD_RUN_OPEN;
			b.syncs.push_back(sync_take(s, match.data(), track_take(x, words.data(), keep)));
		}
	}
	if (have)
		flush(m, b, p, blocks, names, job);
	return 0;
}
