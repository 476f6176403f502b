// tests/envelope_merge_driver.cpp -- tfrec_gpu -Q's pure output code (tfrec_amd/host/job.h: envelope_merger, envelope_summary,
// envelope_line) behind a text interface, for tests/test_envelope_cpu.py.  stdin:
//   file <name> <blocks>                         one per file of the job, in order
//   batch <nb> <file of slot 0> <file of slot 1> ...     (-1: the slot is idle)
//   rec <file> <flags> <start_sample> <n_samples> <thresh> <n_over> <last_over> <energy_head> <energy_tail> <n_gaps> <max_gap>
//       <lead_not_over> <nprod_head> <dot_head> <crs_head> <dot_tail> <crs_tail> <nprod_tail>
//                                                a record of the batch announced last, in table order
// stdout: the extent lines, in the order in which the bursts end.
#include <stdio.h>
#include <string.h>

#include <sstream>
#include <string>
#include <vector>

#include "../tfrec_amd/host/job.h"

static void flush(envelope_merger &m, batch_result &b, const batch_plan &p, const std::vector<size_t> &blocks, const std::vector<std::string> &names)
{
	std::vector<tfrec_amd_envelope> out;
	m.take(b, p, blocks, out);
	for (const tfrec_amd_envelope &x : out)
		printf("%s\n", envelope_line(names[x.stream], x).c_str());
	b.envelopes.clear();
}

int main()
{
	std::vector<std::string> names;
	std::vector<size_t> blocks;
	envelope_merger m;
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
			tfrec_amd_envelope r;
			memset(&r, 0, sizeof(r));
			long long start = 0, dh = 0, ch = 0, dt = 0, ct = 0;
			unsigned long long eh = 0, et = 0;
			in >> r.stream >> r.flags >> start >> r.n_samples >> r.thresh >> r.n_over >> r.last_over >> eh >> et >> r.n_gaps >> r.max_gap >>
				r.lead_not_over >> r.nprod_head >> dh >> ch >> dt >> ct >> r.nprod_tail;
			r.start_sample = start;
			r.energy_head = eh;
			r.energy_tail = et;
			r.dot_head = dh;
			r.crs_head = ch;
			r.dot_tail = dt;
			r.crs_tail = ct;
			if (!in) {
				fprintf(stderr, "bad rec line\n");
				return 1;
			}
			b.envelopes.push_back(r);
		}
	}
	if (have)
		flush(m, b, p, blocks, names);
	return 0;
}
