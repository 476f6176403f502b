// tests/host_engine_driver.cpp -- the pure pieces of tfrec_gpu's engine (tfrec_amd/host/job.h) behind a text interface, for
// tests/test_host_engine_cpu.py: cases on stdin, one per line, results on stdout.  Links nothing of the device library.
//
//   plan      <nslots> <bps> <T> <t> <W> <nfiles> then per file <blocks> <T> <t> <W> <tune>      (T t W: the context's, the file's)
//             -> "plan <batches>", per batch "b <nb>;<file per slot ...>;<reset slots ...>;<slot:T:t:W ...>;<slot:hz ...>"
//   tunes     "new <streams>" starts a sequence with no stream tuned; then per batch "<stream> <hz> ..."
//             -> per batch "<stream:hz ...>;<stream:hz ...>": the tunes behind the resampler; the input-rate tunes
//   channels  <records> <n_bins> <fs_in> <center_khz> <join_hz> <hits[0]> ... <hits[n_bins - 1]>
//             -> per channel "carrier <khz> <bin> <hits>" or "found <khz> <lo> <hi> <hits> <in_range>", then "end"
#include <string.h>

#include <iostream>
#include <sstream>

#include "../tfrec_amd/host/job.h"

template <class A, class B>
static std::string pairs(const std::vector<A> &a, const std::vector<B> &b)
{
	std::ostringstream o;
	for (size_t i = 0; i < a.size(); i++)
		o << (i ? " " : "") << a[i] << ":" << b[i];
	return o.str();
}

static void plan(std::istringstream &in)
{
	size_t nslots, nfiles;
	int bps;
	file_settings dflt = { 0, 0, 0, 0 };
	in >> nslots >> bps >> dflt.types >> dflt.thresh >> dflt.filter >> nfiles;
	std::vector<size_t> blocks(nfiles);
	std::vector<file_settings> settings(nfiles, dflt);
	for (size_t f = 0; f < nfiles; f++)
		in >> blocks[f] >> settings[f].types >> settings[f].thresh >> settings[f].filter >> settings[f].tune;
	if (!in) {
		std::cout << "bad case" << std::endl;
		return;
	}
	const std::vector<batch_plan> p = plan_batches(blocks, settings, dflt, 0, nfiles, nslots, bps);
	std::cout << "plan " << p.size() << "\n";
	for (const batch_plan &b : p) {
		std::cout << "b " << b.nb << ";";
		for (size_t j = 0; j < b.file.size(); j++)
			std::cout << (j ? " " : "") << b.file[j];
		std::cout << ";";
		for (size_t j = 0; j < b.reset.size(); j++)
			std::cout << (j ? " " : "") << b.reset[j];
		std::cout << ";";
		for (size_t j = 0; j < b.conf.size(); j++)
			std::cout << (j ? " " : "") << b.conf[j] << ":" << b.conf_cfg[j].types_mask << ":" << b.conf_cfg[j].thresh << ":"
				  << b.conf_cfg[j].filter_type;
		std::cout << ";" << pairs(b.tune, b.tune_hz) << "\n";
	}
}

static void channels(std::istringstream &in)
{
	unsigned long long records;
	int n_bins;
	long fs_in, center, join;
	in >> records >> n_bins >> fs_in >> center >> join;
	std::vector<unsigned long long> hits(in && n_bins > 0 ? n_bins : 0);
	for (unsigned long long &h : hits)
		in >> h;
	if (!in || hits.empty()) {
		std::cout << "bad case" << std::endl;
		return;
	}
	for (const occ_channel &c : occupancy_channels(hits, records, n_bins, fs_in, center, join)) {
		if (c.carrier)
			std::cout << "carrier " << c.khz << " " << c.lo << " " << c.hits << "\n";
		else
			std::cout << "found " << c.khz << " " << c.lo << " " << c.hi << " " << c.hits << " " << (c.in_range ? 1 : 0) << "\n";
	}
	std::cout << "end\n";
}

int main(int argc, char **argv)
{
	const std::string cmd = argc == 2 ? argv[1] : "";
	if (cmd != "plan" && cmd != "tunes" && cmd != "channels") {
		std::cerr << "usage: host_engine_driver plan|tunes|channels < cases" << std::endl;
		return 1;
	}
	std::vector<bool> in_tune, narrow_tune;  // tunes: the sequence's state
	std::string line;
	while (std::getline(std::cin, line)) {
		std::istringstream in(line);
		if (cmd == "plan") {
			plan(in);
		} else if (cmd == "channels") {
			channels(in);
		} else if (!line.compare(0, 4, "new ")) {
			size_t n = 0;
			in.ignore(4) >> n;
			in_tune.assign(n, false);
			narrow_tune.assign(n, false);
		} else {
			std::vector<int32_t> s, hz;
			int32_t a, b;
			while (in >> a >> b) {
				if (a < 0 || (size_t)a >= in_tune.size()) {
					std::cout << "bad case" << std::endl;
					return 1;
				}
				s.push_back(a);
				hz.push_back(b);
			}
			const tune_calls c = split_tunes(s, hz, in_tune, narrow_tune);
			std::cout << pairs(c.narrow, c.narrow_hz) << ";" << pairs(c.input, c.input_hz) << "\n";
		}
	}
	return 0;
}
