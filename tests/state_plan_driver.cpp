// tests/state_plan_driver.cpp -- the byte plan of tfrec_gpu -k / -K (tfrec_amd/host/job.h: plan_kept_bytes, plan_batches with
// whole = true) behind a text interface, for tests/test_state_cpu.py: compiled there with the address and undefined-behaviour
// sanitizers, nothing of the device library linked.
//   bytes:   lines "<head> <file> <rate_p> <rate_q> <fmt> <wide>" -> "<unit> <piece> <blocks> <used_head> <used_file> <rest_head> <rest_file>"
//   batches: lines "<bps> <blocks of file 0> <blocks of file 1> ..." -> per batch "<nb> <file of stream 0> ...", then "end"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <sstream>

#include "../tfrec_amd/host/job.h"

int main(int argc, char **argv)
{
	if (argc != 2)
		return 2;
	char line[4096];
	while (fgets(line, sizeof(line), stdin)) {
		std::istringstream in(line);
		if (!strcmp(argv[1], "bytes")) {
			unsigned long long head = 0, file = 0;
			job_settings job;
			int wide = 0;
			if (!(in >> head >> file >> job.rate_p >> job.rate_q >> job.fmt >> wide)) {
				printf("bad case\n");
				continue;
			}
			job.wide = wide != 0;
			const kept_bytes k = plan_kept_bytes((size_t)head, (size_t)file, job.piece_bytes(), job.unit());
			printf("%d %zu %zu %zu %zu %zu %zu\n", job.unit(), job.piece_bytes(), k.blocks, k.used_head, k.used_file, k.rest_head, k.rest_file);
		} else if (!strcmp(argv[1], "batches")) {
			int bps = 0;
			std::vector<size_t> blocks;
			in >> bps;
			for (unsigned long long b; in >> b;)
				blocks.push_back((size_t)b);
			if (bps < 1 || blocks.empty()) {
				printf("bad case\n");
				continue;
			}
			const file_settings dflt = { 0x2f, 500, 0, 0 };
			const std::vector<file_settings> settings(blocks.size(), dflt);
			for (const batch_plan &b : plan_batches(blocks, settings, dflt, 0, blocks.size(), blocks.size(), bps, true)) {
				printf("%d", b.nb);
				for (int f : b.file)
					printf(" %d", f);
				printf("\n");
			}
			printf("end\n");
		} else {
			return 2;
		}
	}
	return 0;
}
