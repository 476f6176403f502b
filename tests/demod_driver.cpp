// tests/demod_driver.cpp -- tfrec_gpu's output code for -w (tfrec_amd/host/job.h: demod_parse, demod_take, chain_merger<demod_piece>,
// demod_add and demod_line) behind a text interface, for tests/test_demod_cpu.py.  argv[1]: -w's argument.  One file of one slot;
// stdin, a line per piece of one batch each:
//   <flags> <start_sample> <n_samples> <phase> <timing> <e_best> <e_sum> <n_symbols> <decision> ...
// stdout: the demod line of each burst as it ends; a chain still open at the input's end is flushed there.
#include <stdio.h>

#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../tfrec_amd/host/job.h"

int main(int argc, char **argv)
{
	job_settings::demod_setting set;
	if (argc != 2 || !demod_parse(argv[1], set))
		return 3;
	chain_merger<demod_piece> m;
	m.begin(1);
	const std::vector<size_t> file_blocks(1, (size_t)1 << 40);  // (the file does not end)
	batch_plan p;
	p.nb = 1;
	p.file.assign(1, 0);
	std::vector<demod_piece> ended;
	std::string ln;
	while (std::getline(std::cin, ln)) {
		std::istringstream in(ln);
		tfrec_amd_demod r = tfrec_amd_demod();
		long long start = 0;
		in >> r.flags >> start >> r.n_samples >> r.phase >> r.timing >> r.e_best >> r.e_sum >> r.n_symbols;
		r.start_sample = start;
		r.pool_offset = 3;  // (the piece's decisions lie behind three others in its batch's pool)
		std::vector<int16_t> pool(3, 77);
		int d = 0;
		while (in >> d)
			pool.push_back((int16_t)d);
		if (pool.size() != 3 + (size_t)r.n_symbols)
			return 2;
		m.take(std::vector<demod_piece>(1, demod_take(r, pool.data())), p, file_blocks, ended);
	}
	if (m.open[0])
		ended.push_back(m.chain[0]);
	for (size_t i = 0; i < ended.size(); i++)
		printf("%s\n", demod_line("f", ended[i], set).c_str());
	return 0;
}
