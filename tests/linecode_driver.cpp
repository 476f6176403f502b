// tests/linecode_driver.cpp -- tfrec_gpu's pure code for the line code and the frames' byte order (tfrec_amd/host/job.h: code_parse,
// code_span, code_line on coded pieces merged by chain_merger<track_piece>, sync_line's lsb) behind a text interface, for
// tests/test_linecode_cpu.py.  A stand-alone program: built with the sanitizers and run, never loaded.  stdin, a command a line:
//   parse <-U's argument>                         -> "taps <hex> <invert>" or "bad"
//   span <hex taps> <rate>                        -> "span <samples>"
//   frame <lsb> <bits as a string of 0 and 1, or -> -> sync_line of a frame with those payload bits, in a chain that starts at 1000
//                                                 with its plateau's sample at 30, no errors, polarity +, file "f"
//   rate <bit/s>                                  the slicer's rate for what follows
//   file <blocks>                                 the one file "f" and its length; begins a job
//   piece <nb> <flags> <start_sample> <n_samples> <bit_offset> <last_over> <n_ones> <hex word> ...
//                                                 a batch of nb blocks that holds one coded record of file 0 and its bitmap: taken by
//                                                 track_take, merged by chain_merger<track_piece>; every burst that ends with the
//                                                 batch -> its code_line
#include <stdio.h>

#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../tfrec_amd/host/job.h"

int main()
{
	std::string line;
	long rate = 6000;
	chain_merger<track_piece> merger;
	std::vector<size_t> blocks;
	while (std::getline(std::cin, line)) {
		std::istringstream in(line);
		std::string cmd;
		in >> cmd;
		if (cmd == "parse") {
			std::string arg;
			in >> arg;
			uint32_t taps = 0;
			bool inv = false;
			if (code_parse(arg.c_str(), taps, inv))
				printf("taps %x %d\n", (unsigned)taps, (int)inv);
			else
				printf("bad\n");
		} else if (cmd == "span") {
			std::string hex;
			long r = 0;
			in >> hex >> r;
			printf("span %llu\n", (unsigned long long)code_span((uint32_t)strtoul(hex.c_str(), NULL, 16), r));
		} else if (cmd == "frame") {
			int lsb = 0;
			std::string bits;
			in >> lsb >> bits;
			sync_piece c;
			static_cast<tfrec_amd_burst_sync &>(c) = tfrec_amd_burst_sync();
			c.start_sample = 1000;
			sync_frame f;
			f.c = 30;
			if (bits != "-")
				for (char ch : bits)
					f.bits.push_back((uint8_t)(ch == '1'));
			printf("%s\n", sync_line("f", c, f, lsb != 0).c_str());
		} else if (cmd == "rate") {
			in >> rate;
		} else if (cmd == "file") {
			size_t nb = 0;
			in >> nb;
			blocks.assign(1, nb);
			merger = chain_merger<track_piece>();
			merger.begin(1);
		} else if (cmd == "piece") {
			tfrec_amd_track r = tfrec_amd_track();
			batch_plan plan;
			long long start = 0;
			unsigned long long off = 0;
			in >> plan.nb >> r.flags >> start >> r.n_samples >> off >> r.last_over >> r.n_ones;
			r.start_sample = start;
			r.bit_offset = off;
			std::vector<uint32_t> words;
			std::string hex;
			while (in >> hex)
				words.push_back((uint32_t)strtoul(hex.c_str(), NULL, 16));
			words.push_back(0u);
			plan.file.assign(1, 0);
			std::vector<track_piece> recs(1, track_take(r, words.data(), r.n_samples)), out;
			merger.take(recs, plan, blocks, out);
			for (const track_piece &x : out)
				printf("%s\n", code_line("f", x, rate).c_str());
		} else if (!cmd.empty()) {
			fprintf(stderr, "linecode_driver: bad line '%s'\n", line.c_str());
			return 2;
		}
	}
	return 0;
}
