// tests/band_driver.cpp -- tfrec_gpu's output code for -I (tfrec_amd/host/job.h: chain_merger<tfrec_amd_band>, band_add, band_summary
// and band_line) behind a text interface, for tests/test_band_cpu.py.  One file of one slot; stdin, a line per piece of one batch each:
//   <flags> <start_sample> <n_samples> <n_segments> <n_silent> <bin>:<value> ...        (bins -128 .. 127, the others 0)
// stdout: the band line of each burst as it ends; a chain still open at the input's end is flushed there.
#include <stdio.h>

#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../tfrec_amd/host/job.h"

int main()
{
	chain_merger<tfrec_amd_band> m;
	m.begin(1);
	const std::vector<size_t> file_blocks(1, (size_t)1 << 40);  // (the file does not end)
	batch_plan p;
	p.nb = 1;
	p.file.assign(1, 0);
	std::vector<tfrec_amd_band> ended;
	std::string ln;
	while (std::getline(std::cin, ln)) {
		std::istringstream in(ln);
		tfrec_amd_band r = tfrec_amd_band();
		long long start = 0;
		in >> r.flags >> start >> r.n_samples >> r.n_segments >> r.n_silent;
		r.start_sample = start;
		std::string tok;
		while (in >> tok) {
			const size_t c = tok.find(':');
			const int j = atoi(tok.substr(0, c).c_str());
			if (c == std::string::npos || j < -128 || j > 127)
				return 2;
			r.spec[j + 128] = strtoull(tok.c_str() + c + 1, NULL, 10);
		}
		m.take(std::vector<tfrec_amd_band>(1, r), p, file_blocks, ended);
	}
	if (m.open[0])
		ended.push_back(m.chain[0]);
	for (size_t i = 0; i < ended.size(); i++)
		printf("%s\n", band_line("f", ended[i]).c_str());
	return 0;
}
