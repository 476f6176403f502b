// tests/clock_merge_driver.cpp -- tfrec_gpu -C's pure output code (tfrec_amd/host/job.h: clock_merger, clock_summary, clock_line)
// behind a text interface, for tests/test_clock_cpu.py.  stdin:
//   file <name> <blocks>                         one per file of the job, in order
//   batch <nb> <file of slot 0> <file of slot 1> ...     (-1: the slot is idle)
//   rec <file> <flags> <start_sample> <n_samples> <thresh> <n_segments> <n_silent> <spec[0]> ... <spec[127]>
//                                                a record of the batch announced last, in table order
// stdout: the clock lines, in the order in which the bursts end.
#include <stdio.h>
#include <string.h>

#include <sstream>
#include <string>
#include <vector>

#include "../tfrec_amd/host/job.h"

static void flush(clock_merger &m, batch_result &b, const batch_plan &p, const std::vector<size_t> &blocks, const std::vector<std::string> &names)
{
	std::vector<tfrec_amd_clock> out;
	m.take(b, p, blocks, out);
	for (const tfrec_amd_clock &x : out)
		printf("%s\n", clock_line(names[x.stream], x).c_str());
	b.clocks.clear();
}

int main()
{
	std::vector<std::string> names;
	std::vector<size_t> blocks;
	clock_merger m;
	batch_result b;
	batch_plan p;
	bool have = false;
	static char buf[16384];
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
			tfrec_amd_clock r;
			memset(&r, 0, sizeof(r));
			long long start = 0;
			in >> r.stream >> r.flags >> start >> r.n_samples >> r.thresh >> r.n_segments >> r.n_silent;
			r.start_sample = start;
			for (int i = 0; i < 128; i++) {
				unsigned long long v = 0;
				in >> v;
				r.spec[i] = v;
			}
			if (!in) {
				fprintf(stderr, "bad rec line\n");
				return 1;
			}
			b.clocks.push_back(r);
		}
	}
	if (have)
		flush(m, b, p, blocks, names);
	return 0;
}
