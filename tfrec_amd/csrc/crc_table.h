// tfrec_amd/csrc/crc_table.h -- the frame check's settings and term table (include/tfrec_amd.h: "Frame check"), in plain
// C++ with no HIP in it: the enable call uses it, the host program's -V checks its argument with it, and a stand-alone test driver
// compiles it under the host sanitizers and compares it with tfrec_amd/crc.py's.
//
// residue(b) = crc(covered bytes of b) ^ xorout ^ field(b) is affine over GF(2) in the 8 N frame bits b_1 .. b_8N, so
//   residue(b) = r0 ^ XOR over the set b_i of col_i,   r0 = residue(0),   col_i = residue(e_i) ^ r0,
// and with INVERT (every bit complemented before use) r0 = residue(all ones) with the same columns.  b_i is read D - delta(i) samples
// ahead of the frame's last bit: the table holds (off_i = D - delta(i), col_i) for the i with col_i != 0, in the order of i.  The
// skipped bytes drop out.  The builder runs the CRC as the header words it, once per frame bit.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <vector>

namespace tfrec_crc {

constexpr uint32_t kFlagLsb = 1u, kFlagInvert = 2u;  // TFREC_AMD_CRC_LSB, TFREC_AMD_CRC_INVERT
constexpr long long kReach = 16383;                  // the largest D: the carried history's bits

struct Settings {
	int32_t rate, n_bytes, skip, width;
	uint32_t poly, init, xorout, flags;
};

struct Term {
	uint32_t off;  // the bit is read at k - off
	uint32_t col;  // what it contributes to the residue
};

// delta(i) = floor((768000 i + R) / (2 R)), the burst sync's
inline long long delta(long long i, long long rate) { return (768000LL * i + rate) / (2LL * rate); }

// D = delta(8 N): the samples from the sync's centre to the frame's last bit
inline long long reach(const Settings &s) { return delta(8LL * s.n_bytes, s.rate); }

// NULL where the settings are the header's, else what is wrong with them
inline const char *refusal(const Settings &s)
{
	if (s.rate < 1000 || s.rate > 96000)
		return "the frame check's rate is within [1000, 96000] bit/s";
	if (s.n_bytes < 1 || s.n_bytes > 256)
		return "the frame check's frame has 1 .. 256 bytes";
	if (s.width != 8 && s.width != 16 && s.width != 24 && s.width != 32)
		return "the frame check's width is 8, 16, 24 or 32";
	if (s.skip < 0 || (long long)s.skip + s.width / 8 >= s.n_bytes)
		return "the frame check covers at least one byte: 0 <= skip and skip + width / 8 < n_bytes";
	const uint64_t top = 1ull << s.width;
	if (!s.poly || s.poly >= top || s.init >= top || s.xorout >= top)
		return "the frame check's poly is non-zero, and poly, init and xorout are below 2^width";
	if (s.flags & ~(kFlagLsb | kFlagInvert))
		return "the frame check's flags are 1, LSB-first bytes, and 2, complemented bits";
	if (reach(s) > kReach)
		return "the frame check's frame reaches more than 16383 samples at the rate";
	return nullptr;
}

// residue of the frame whose bits b_1 .. b_8N (after INVERT) are bits[0 .. 8 N): the bitwise CRC of the header over the covered
// bytes, ^ xorout ^ the field
inline uint32_t residue(const Settings &s, const uint8_t *bits)
{
	const uint32_t mask = s.width == 32 ? 0xffffffffu : (1u << s.width) - 1u, top = 1u << (s.width - 1);
	const int fb = s.width / 8;
	uint32_t r = s.init, field = 0;
	for (int j = 0; j < s.n_bytes; j++) {
		uint32_t byte = 0;
		for (int q = 0; q < 8; q++)
			byte |= (uint32_t)(bits[8 * j + q] & 1) << ((s.flags & kFlagLsb) ? q : 7 - q);
		if (j >= s.n_bytes - fb) {
			field = (field << 8) | byte;
		} else if (j >= s.skip) {
			r ^= byte << (s.width - 8);
			for (int q = 0; q < 8; q++)
				r = ((r & top) ? (r << 1) ^ s.poly : r << 1) & mask;
		}
	}
	return (r ^ s.xorout ^ field) & mask;
}

// The table and r0 of settings that refusal() passes.  At most 8 N terms.
inline void build(const Settings &s, std::vector<Term> &terms, uint32_t &r0)
{
	const int nb = 8 * s.n_bytes;
	const long long D = reach(s);
	std::vector<uint8_t> bits((size_t)nb, 0);
	const uint32_t z = residue(s, bits.data());
	terms.clear();
	for (int i = 1; i <= nb; i++) {
		bits[(size_t)i - 1] = 1;
		const uint32_t col = residue(s, bits.data()) ^ z;
		bits[(size_t)i - 1] = 0;
		if (col)
			terms.push_back({ (uint32_t)(D - delta(i, s.rate)), col });
	}
	if (s.flags & kFlagInvert) {
		std::fill(bits.begin(), bits.end(), (uint8_t)1);
		r0 = residue(s, bits.data());
	} else {
		r0 = z;
	}
}

}  // namespace tfrec_crc
