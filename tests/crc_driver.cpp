// tests/crc_driver.cpp -- the frame check's plain C++ (tfrec_amd/csrc/crc_table.h: refusal, reach, build; tfrec_amd/host/job.h:
// crc_parse, check pieces merged by chain_merger<crc_piece>, crc_verdict, crc_line) behind a text interface, for
// tests/test_crc_cpu.py.  A stand-alone program: built with the sanitizers and run, never loaded.  stdin, a command a line:
//   table <rate> <n_bytes> <skip> <width> <poly> <init> <xorout> <flags>   (poly, init, xorout hex)
//                                                 -> "refused" or "table <D> <r0 hex> <off>:<col hex> ..."
//   parse <-V's argument>                         -> "crc <width> <poly> <init> <xorout> <skip> <invert>" or "bad"
//   reach <D>                                     D for the lines and verdicts that follow
//   file <blocks>                                 the one file "f" and its length; begins a job
//   piece <nb> <flags> <start_sample> <n_samples> <cut_samples> <bit_offset> <n_ok> <first_at> <hex word> ...
//                                                 a batch of nb blocks that holds one check record of file 0 and its bitmap: taken by
//                                                 crc_take beside a track piece of cut_samples samples, merged by
//                                                 chain_merger<crc_piece>; every burst that ends with the batch -> its crc_line
//   verdict <c> <plus> <n_bits> <n_bytes>         -> crc_verdict of such a frame on the burst that ended last
#include <stdio.h>

#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../tfrec_amd/host/job.h"

int main()
{
	std::string line;
	uint64_t D = 0;
	chain_merger<crc_piece> merger;
	std::vector<size_t> blocks;
	crc_piece last;
	static_cast<tfrec_amd_burst_crc &>(last) = tfrec_amd_burst_crc();
	while (std::getline(std::cin, line)) {
		std::istringstream in(line);
		std::string cmd;
		in >> cmd;
		if (cmd == "table") {
			tfrec_crc::Settings s = tfrec_crc::Settings();
			std::string poly, init, xorout;
			in >> s.rate >> s.n_bytes >> s.skip >> s.width >> poly >> init >> xorout >> s.flags;
			s.poly = (uint32_t)strtoul(poly.c_str(), NULL, 16);
			s.init = (uint32_t)strtoul(init.c_str(), NULL, 16);
			s.xorout = (uint32_t)strtoul(xorout.c_str(), NULL, 16);
			if (tfrec_crc::refusal(s)) {
				printf("refused\n");
				continue;
			}
			std::vector<tfrec_crc::Term> terms;
			uint32_t r0 = 0;
			tfrec_crc::build(s, terms, r0);
			printf("table %lld %x", tfrec_crc::reach(s), (unsigned)r0);
			for (const tfrec_crc::Term &t : terms)
				printf(" %u:%x", (unsigned)t.off, (unsigned)t.col);
			printf("\n");
		} else if (cmd == "parse") {
			std::string arg;
			in >> arg;
			int width = 0, skip = 0;
			uint32_t poly = 0, init = 0, xorout = 0;
			bool inv = false;
			if (crc_parse(arg.c_str(), width, poly, init, xorout, skip, inv))
				printf("crc %d %x %x %x %d %d\n", width, (unsigned)poly, (unsigned)init, (unsigned)xorout, skip, (int)inv);
			else
				printf("bad\n");
		} else if (cmd == "reach") {
			in >> D;
		} else if (cmd == "file") {
			size_t nb = 0;
			in >> nb;
			blocks.assign(1, nb);
			merger = chain_merger<crc_piece>();
			merger.begin(1);
		} else if (cmd == "piece") {
			tfrec_amd_burst_crc r = tfrec_amd_burst_crc();
			batch_plan plan;
			long long start = 0;
			unsigned long long off = 0;
			uint32_t cut = 0;
			in >> plan.nb >> r.flags >> start >> r.n_samples >> cut >> off >> r.n_ok >> r.first_at;
			r.start_sample = start;
			r.bit_offset = off;
			std::vector<uint32_t> words;
			std::string hex;
			while (in >> hex)
				words.push_back((uint32_t)strtoul(hex.c_str(), NULL, 16));
			words.push_back(0u);
			plan.file.assign(1, 0);
			track_piece t;
			static_cast<tfrec_amd_track &>(t) = tfrec_amd_track();
			t.flags = r.flags;
			t.n_samples = cut;
			std::vector<crc_piece> recs(1, crc_take(r, words.data(), t)), out;
			merger.take(recs, plan, blocks, out);
			for (const crc_piece &x : out) {
				printf("%s\n", crc_line("f", x, D).c_str());
				last = x;
			}
		} else if (cmd == "verdict") {
			sync_frame f;
			int plus = 1, n_bytes = 0;
			size_t n_bits = 0;
			in >> f.c >> plus >> n_bits >> n_bytes;
			f.plus = plus != 0;
			f.bits.assign(n_bits, 0);
			printf("%s\n", crc_verdict(last, f, n_bytes, D));
		} else if (!cmd.empty()) {
			fprintf(stderr, "crc_driver: bad line '%s'\n", line.c_str());
			return 2;
		}
	}
	return 0;
}
