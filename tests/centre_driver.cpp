// tests/centre_driver.cpp -- tfrec_gpu -G rate,auto's centre pieces (tfrec_amd/host/job.h: centre_take, the chain merge that keeps the
// first piece's centre, centre_line) in a stand-alone program, for tests/test_centre_cpu.py, which builds it under the address and
// undefined-behaviour sanitizers.  stdin: the pieces of one file's batches in order, and `batch` behind each batch's pieces,
//   piece <flags> <start_sample> <n_samples> <last_over> <n_counted> <source> <centre_hz> <deviation_hz> <index>
// (a piece carries no track bits here: track_add is given empty ones); stdout: per chain that ended, in the merger's order, its
// centre line and behind it `merged <flags> <n_samples> <last_over> <index>`.
#include <stdio.h>

#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../tfrec_amd/host/job.h"

int main()
{
	const std::string file = "f.iq";
	chain_merger<track_piece> merger;
	merger.begin(1);
	batch_plan plan;
	plan.file.assign(1, 0);
	plan.nb = 1;
	const std::vector<size_t> file_blocks(1, (size_t)1 << 20);  // (the file does not end here)
	std::vector<track_piece> batch, out;
	std::string line;
	while (std::getline(std::cin, line)) {
		std::istringstream in(line);
		std::string word;
		in >> word;
		if (word == "batch") {
			out.clear();
			merger.take(batch, plan, file_blocks, out);
			batch.clear();
			for (size_t i = 0; i < out.size(); i++) {
				printf("%s\n", centre_line(file, out[i]).c_str());
				printf("merged %u %u %d %d\n", (unsigned)out[i].flags, (unsigned)out[i].n_samples, (int)out[i].last_over, (int)out[i].cen.index);
			}
			continue;
		}
		long long flags = 0, start = 0, n = 0, last = 0, counted = 0, source = 0, hz = 0, dev = 0, index = 0;
		in >> flags >> start >> n >> last >> counted >> source >> hz >> dev >> index;
		if (!in || word != "piece" || n < 1 || n > 0xffffffffLL || last < -1 || last >= n || source < 0 || source > 2) {
			fprintf(stderr, "centre_driver: bad line '%s'\n", line.c_str());
			return 1;
		}
		track_piece p;
		static_cast<tfrec_amd_track &>(p) = tfrec_amd_track();
		p.flags = (uint32_t)flags;
		p.start_sample = start;
		p.n_samples = (uint32_t)n;
		p.last_over = (int32_t)last;
		tfrec_amd_track_centre c = tfrec_amd_track_centre();
		c.flags = p.flags;
		c.start_sample = start;
		c.n_samples = p.n_samples;
		c.n_counted = (uint32_t)counted;
		c.source = (uint32_t)source;
		c.centre_hz = (int32_t)hz;
		c.deviation_hz = (int32_t)dev;
		c.index = (int32_t)index;
		centre_take(p, c);
		batch.push_back(p);
	}
	return 0;
}
