// tfrec_amd/csrc/packet_table.h -- the packet check's settings and power tables (include/tfrec_amd.h: "Packet check"), in
// plain C++ with no HIP in it, beside crc_table.h: the enable call checks its arguments and builds its tables with it.
//
// A packet's length is data, so the frame check's fixed-offset term table does not apply; what stays linear is the register as a
// polynomial.  With r -> (r ^ byte << (W - 8)) x^8 mod poly per covered byte, a packet of T bytes whose bytes j >= skip are d_j has
//   residue = init x^(8 n) ^ XOR over skip <= j < T of d_j x^(8 (T - 1 - j)) ^ xorout  (mod poly),   n = T - W / 8 - skip,
// where the covered bytes' x^(W - 8) x^(8 (n - (j - skip))) and the field bytes' own place, x^(8 (T - 1 - j)) with no reduction, are
// the same expression; the packet checks iff the residue is 0.  The tables are x8[k] = x^(8 k) mod poly and i8[k] = init x^(8 k) mod
// poly, k = 0 .. 275: a byte's term is then eight shift / XOR steps, whatever the width.
#pragma once

#include <stdint.h>

#include <vector>

namespace tfrec_packet {

constexpr uint32_t kFlagLsb = 1u, kFlagInvert = 2u;  // TFREC_AMD_CRC_LSB, TFREC_AMD_CRC_INVERT
constexpr long long kReach = 16383;                  // the carried history's bits: the largest delta(8 T)
constexpr int kMaxAdd = 16, kMaxWhiten = 274;
constexpr int kMaxBytes = 1 + 255 + kMaxAdd + 4;     // the largest T: 276
constexpr int kTable = kMaxBytes;                    // x8 and i8 hold the exponents 0 .. 275

struct Settings {
	int32_t rate, len_min, len_max, len_add, skip, width;
	uint32_t poly, init, xorout, flags;
	int32_t n_whiten;
};

// delta(i) = floor((768000 i + R) / (2 R)), the burst sync's
inline long long delta(long long i, long long rate) { return (768000LL * i + rate) / (2LL * rate); }

// T of a length byte L: the length byte, the L bytes it counts, the len_add it does not and the CRC field
inline int total(const Settings &s, int L) { return 1 + L + s.len_add + s.width / 8; }

// delta(8 T_max): the samples from the sync's centre to the last bit of the longest packet
inline long long reach(const Settings &s) { return delta(8LL * total(s, s.len_max), s.rate); }

// NULL where the settings are the header's, else what is wrong with them
inline const char *refusal(const Settings &s)
{
	if (s.rate < 1000 || s.rate > 96000)
		return "the packet check's rate is within [1000, 96000] bit/s";
	if (s.len_min < 0 || s.len_max > 255 || s.len_min > s.len_max)
		return "the packet check's lengths are 0 <= len_min <= len_max <= 255";
	if (s.len_add < 0 || s.len_add > kMaxAdd)
		return "the packet check's len_add is within 0 .. 16";
	if (s.width != 8 && s.width != 16 && s.width != 24 && s.width != 32)
		return "the packet check's width is 8, 16, 24 or 32";
	if (s.skip < 0 || s.skip >= 1 + s.len_min + s.len_add)  // (T - W / 8 - skip covered bytes)
		return "the packet check covers at least one byte: 0 <= skip < 1 + len_min + len_add";
	const uint64_t top = 1ull << s.width;
	if (!s.poly || s.poly >= top || s.init >= top || s.xorout >= top)
		return "the packet check's poly is non-zero, and poly, init and xorout are below 2^width";
	if (s.flags & ~(kFlagLsb | kFlagInvert))
		return "the packet check's flags are 1, LSB-first bytes, and 2, complemented bits";
	if (s.n_whiten < 0 || s.n_whiten > kMaxWhiten)
		return "the packet check's whitening sequence has 0 .. 274 bytes";
	if (reach(s) > kReach)
		return "the packet check's longest packet reaches more than 16383 samples at the rate";
	return nullptr;
}

// r x^8 mod poly
inline uint32_t times_x8(const Settings &s, uint32_t r)
{
	const uint32_t mask = s.width == 32 ? 0xffffffffu : (1u << s.width) - 1u, top = 1u << (s.width - 1);
	for (int q = 0; q < 8; q++)
		r = ((r & top) ? (r << 1) ^ s.poly : r << 1) & mask;
	return r;
}

// out[k] = x^(8 k) mod poly, out[kTable + k] = init x^(8 k) mod poly, k = 0 .. kTable - 1
inline void build(const Settings &s, std::vector<uint32_t> &out)
{
	out.assign(2 * (size_t)kTable, 0u);
	uint32_t x = 1u, i = s.init;
	for (int k = 0; k < kTable; k++) {
		out[(size_t)k] = x;
		out[(size_t)kTable + k] = i;
		x = times_x8(s, x);
		i = times_x8(s, i);
	}
}

}  // namespace tfrec_packet
