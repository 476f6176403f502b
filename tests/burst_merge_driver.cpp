// tests/burst_merge_driver.cpp -- tfrec_gpu -M's pure output code (tfrec_amd/host/job.h: burst_merger, burst_summary, burst_line) behind
// a text interface, for tests/test_burst_cpu.py.  stdin:
//   file <name> <blocks>                         one per file of the job, in order
//   batch <nb> <file of slot 0> <file of slot 1> ...     (-1: the slot is idle)
//   rec <file> <flags> <start_sample> <n_samples> <thresh> <pwr_max> <n_products> <sum_dot> <sum_crs> <energy> <hist 0> .. <hist 63>
//                                                a record of the batch announced last, in table order
// stdout: the burst lines, in the order in which the bursts end.
#include <stdio.h>
#include <string.h>

#include <sstream>
#include <string>
#include <vector>

#include "../tfrec_amd/host/job.h"

static void flush(burst_merger &m, batch_result &b, const batch_plan &p, const std::vector<size_t> &blocks, const std::vector<std::string> &names)
{
	std::vector<tfrec_amd_burst> out;
	m.take(b, p, blocks, out);
	for (const tfrec_amd_burst &x : out)
		printf("%s\n", burst_line(names[x.stream], x).c_str());
	b.bursts.clear();
}

int main()
{
	std::vector<std::string> names;
	std::vector<size_t> blocks;
	burst_merger m;
	batch_result b;
	batch_plan p;
	bool have = false;
	char buf[4096];
	while (fgets(buf, sizeof(buf), stdin)) {
		std::istringstream in(buf);
		std::string cmd;
		in >> cmd;
		if (cmd == "file") {
			std::string name;
			size_t nb = 0;
			in >> name >> nb;
			names.push_back(name);
			blocks.push_back(nb);
		} else if (cmd == "batch") {
			if (have)
				flush(m, b, p, blocks, names);
			else
				m.begin(names.size());
			have = true;
			p = batch_plan();
			in >> p.nb;
			for (int f; in >> f;)
				p.file.push_back(f);
		} else if (cmd == "rec") {
			tfrec_amd_burst r;
			memset(&r, 0, sizeof(r));
			long long start = 0, sd = 0, sc = 0;
			unsigned long long en = 0;
			in >> r.stream >> r.flags >> start >> r.n_samples >> r.thresh >> r.pwr_max >> r.n_products >> sd >> sc >> en;
			r.start_sample = start;
			r.sum_dot = sd;
			r.sum_crs = sc;
			r.energy = en;
			for (int j = 0; j < 64; j++)
				in >> r.hist[j];
			if (!in) {
				fprintf(stderr, "bad rec line\n");
				return 1;
			}
			b.bursts.push_back(r);
		}
	}
	if (have)
		flush(m, b, p, blocks, names);
	return 0;
}
