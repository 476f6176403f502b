// tests/corr_driver.cpp -- tfrec_gpu's output code for -y (tfrec_amd/host/job.h: corr_parse, chain_merger<tfrec_amd_corr>, corr_add,
// corr_summary and corr_line) behind a text interface, for tests/test_corr_cpu.py.  argv[1]: -y's argument.  One file of one slot;
// stdin, a line per piece of one batch each:
//   <flags> <start_sample> <n_samples> <t>:<peak>:<peak_at>:<trough>:<trough_at>:<n_pos>:<sum_abs> ...     (the other templates: none)
// stdout: the corr line of each burst as it ends; a chain still open at the input's end is flushed there.
#include <limits.h>
#include <stdio.h>

#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../tfrec_amd/host/job.h"

int main(int argc, char **argv)
{
	job_settings::corr_bank bank;
	if (argc != 2 || !corr_parse(argv[1], bank))
		return 3;
	chain_merger<tfrec_amd_corr> m;
	m.begin(1);
	const std::vector<size_t> file_blocks(1, (size_t)1 << 40);  // (the file does not end)
	batch_plan p;
	p.nb = 1;
	p.file.assign(1, 0);
	std::vector<tfrec_amd_corr> ended;
	std::string ln;
	while (std::getline(std::cin, ln)) {
		std::istringstream in(ln);
		tfrec_amd_corr r = tfrec_amd_corr();
		for (int t = 0; t < 16; t++) {
			r.t[t].peak = INT_MIN;
			r.t[t].trough = INT_MAX;
		}
		long long start = 0;
		in >> r.flags >> start >> r.n_samples;
		r.start_sample = start;
		std::string tok;
		while (in >> tok) {
			int t = 0, peak = 0, trough = 0;
			unsigned peak_at = 0, trough_at = 0, n_pos = 0;
			unsigned long long sum_abs = 0;
			if (sscanf(tok.c_str(), "%d:%d:%u:%d:%u:%u:%llu", &t, &peak, &peak_at, &trough, &trough_at, &n_pos, &sum_abs) != 7 || t < 0 || t > 15)
				return 2;
			r.t[t].peak = peak;
			r.t[t].peak_at = peak_at;
			r.t[t].trough = trough;
			r.t[t].trough_at = trough_at;
			r.t[t].n_pos = n_pos;
			r.t[t].sum_abs = sum_abs;
		}
		m.take(std::vector<tfrec_amd_corr>(1, r), p, file_blocks, ended);
	}
	if (m.open[0])
		ended.push_back(m.chain[0]);
	for (size_t i = 0; i < ended.size(); i++)
		printf("%s\n", corr_line("f", ended[i], bank).c_str());
	return 0;
}
