// tests/pulses_driver.cpp -- tfrec_gpu -O's pulses (tfrec_amd/host/job.h: track_pulses, pulses_line) in a stand-alone program, for
// tests/test_amplitude_cpu.py, which builds it under the address and undefined-behaviour sanitizers.  stdin: one merged track a line,
//   track <file> <start_sample> <n_samples> <last_over> <the kept bits as a string of 0 and 1, or - for none>
// (as many bits as min(n_samples, 2^20)); stdout: the track's pulses line, and behind it `widths <n> <w0> <g0> ...`, what
// track_pulses returned in full.
#include <stdio.h>

#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../tfrec_amd/host/job.h"

int main()
{
	std::string line;
	while (std::getline(std::cin, line)) {
		std::istringstream in(line);
		std::string word, file, bits;
		long long start = 0, n = 0, last = 0;
		in >> word >> file >> start >> n >> last >> bits;
		if (!in || word != "track" || n < 0 || n > 0xffffffffLL || last < -1 || last >= n) {
			fprintf(stderr, "pulses_driver: bad line '%s'\n", line.c_str());
			return 1;
		}
		if (bits == "-")
			bits.clear();
		track_piece p;
		static_cast<tfrec_amd_track &>(p) = tfrec_amd_track();
		p.start_sample = start;
		p.n_samples = (uint32_t)n;
		p.last_over = (int32_t)last;
		if (bits.size() != p.kept()) {
			fprintf(stderr, "pulses_driver: %zu bits for %llu kept samples\n", bits.size(), (unsigned long long)p.kept());
			return 1;
		}
		p.bits.assign((bits.size() + 31) / 32, 0u);
		for (size_t k = 0; k < bits.size(); k++)
			if (bits[k] == '1') {
				p.bits[k >> 5] |= 1u << (k & 31);
				p.n_ones++;
			}
		printf("%s\n", pulses_line(file, p).c_str());
		const std::vector<uint64_t> w = track_pulses(p);
		printf("widths %zu", w.size());
		for (size_t i = 0; i < w.size(); i++)
			printf(" %llu", (unsigned long long)w[i]);
		printf("\n");
	}
	return 0;
}
