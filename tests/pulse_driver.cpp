// tests/pulse_driver.cpp -- tfrec_gpu's pure code for the pulse slicer (tfrec_amd/host/job.h: symbols_take, symbols_add through
// chain_merger<symbol_piece>, symbols_line) behind a text interface, for tests/test_pulsecode_cpu.py.  A stand-alone program: built
// with the sanitizers and run, never loaded.  stdin, a command a line: "file <blocks>" begins a job of one file "f";
// "piece <nb> <flags> <start_sample> <n_samples> <bit_offset> <n_breaks> <n_glitches> <symbols as 0, 1 and /, or ->" is a batch of nb
// blocks with one symbols record of file 0, its symbols from bit_offset on in both bitmaps -> the symbols_line of every burst it ends
#include <stdio.h>

#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../tfrec_amd/host/job.h"

int main()
{
	std::string line;
	chain_merger<symbol_piece> merger;
	std::vector<size_t> blocks;
	while (std::getline(std::cin, line)) {
		std::istringstream in(line);
		std::string cmd;
		in >> cmd;
		if (cmd == "file") {
			size_t nb = 0;
			in >> nb;
			blocks.assign(1, nb);
			merger = chain_merger<symbol_piece>();
			merger.begin(1);
		} else if (cmd == "piece") {
			tfrec_amd_burst_symbols r = tfrec_amd_burst_symbols();
			batch_plan plan;
			long long start = 0;
			unsigned long long off = 0;
			std::string text;
			in >> plan.nb >> r.flags >> start >> r.n_samples >> off >> r.n_breaks >> r.n_glitches >> text;
			r.start_sample = start;
			r.bit_offset = off;
			r.n_symbols = text == "-" ? 0u : (uint32_t)text.size();
			std::vector<uint32_t> bits((size_t)((off + r.n_symbols) / 32 + 1), 0u), marks(bits);
			for (uint64_t i = 0; i < r.n_symbols; i++)
				(text[i] == '/' ? marks : bits)[(off + i) >> 5] |= (uint32_t)(text[i] != '0') << ((off + i) & 31);
			track_piece t;
			static_cast<tfrec_amd_track &>(t) = tfrec_amd_track();
			t.flags = r.flags;
			t.n_samples = r.n_samples;
			plan.file.assign(1, 0);
			std::vector<symbol_piece> recs(1, symbols_take(r, bits.data(), marks.data(), t)), out;
			merger.take(recs, plan, blocks, out);
			for (const symbol_piece &x : out)
				printf("%s\n", symbols_line("f", x).c_str());
		} else if (!cmd.empty()) {
			fprintf(stderr, "pulse_driver: bad line '%s'\n", line.c_str());
			return 2;
		}
	}
	return 0;
}
