// tests/track_merge_driver.cpp -- tfrec_gpu -G's pure output code (tfrec_amd/host/job.h: track_take, track_merger, track_slice,
// track_line) behind a text interface, for tests/test_track_cpu.py.  stdin:
//   rate <bit/s>                                  once, first
//   file <name> <blocks>                          one per file of the job, in order
//   batch <nb> <file of slot 0> <file of slot 1> ...     (-1: the slot is idle)
//   words <hex word> <hex word> ...               the bitmap of the batch announced last (may be missing: no bits)
//   rec <file> <flags> <start_sample> <n_samples> <thresh> <bit_offset> <last_over> <n_ones> <kept_samples>
//                                                 a record of that batch, in table order; kept_samples <= n_samples: where the
//                                                 file's end cuts it
// stdout: the bits lines, in the order in which the bursts end.
#include <stdio.h>
#include <string.h>

#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../tfrec_amd/host/job.h"

static void flush(track_merger &m, batch_result &b, const batch_plan &p, const std::vector<size_t> &blocks, const std::vector<std::string> &names,
		  long rate)
{
	std::vector<track_piece> out;
	m.take(b, p, blocks, out);
	for (const track_piece &x : out)
		printf("%s\n", track_line(names[x.stream], x, rate).c_str());
	b.tracks.clear();
}

int main()
{
	std::vector<std::string> names;
	std::vector<size_t> blocks;
	std::vector<uint32_t> words;
	track_merger m;
	batch_result b;
	batch_plan p;
	bool have = false;
	long rate = 0;
	std::string line;
	while (std::getline(std::cin, line)) {
		std::istringstream in(line);
		std::string cmd;
		in >> cmd;
		if (cmd == "rate") {
			in >> rate;
		} else if (cmd == "file") {
			std::string name;
			size_t nb = 0;
			in >> name >> nb;
			names.push_back(name);
			blocks.push_back(nb);
		} else if (cmd == "batch") {
			if (have)
				flush(m, b, p, blocks, names, rate);
			else
				m.begin(names.size());
			have = true;
			p = batch_plan();
			words.clear();
			in >> p.nb;
			for (int f; in >> f;)
				p.file.push_back(f);
		} else if (cmd == "words") {
			for (std::string w; in >> w;)
				words.push_back((uint32_t)strtoul(w.c_str(), NULL, 16));
		} else if (cmd == "rec") {
			tfrec_amd_track r;
			memset(&r, 0, sizeof(r));
			long long start = 0;
			unsigned long long off = 0;
			uint32_t keep = 0;
			in >> r.stream >> r.flags >> start >> r.n_samples >> r.thresh >> off >> r.last_over >> r.n_ones >> keep;
			r.start_sample = start;
			r.bit_offset = off;
			if (!in || keep > r.n_samples || off + r.n_samples > 32ull * words.size()) {
				fprintf(stderr, "bad rec line\n");
				return 1;
			}
			b.tracks.push_back(track_take(r, words.data(), keep));
		}
	}
	if (have)
		flush(m, b, p, blocks, names, rate);
	return 0;
}
