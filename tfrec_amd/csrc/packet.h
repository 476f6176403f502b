// tfrec_amd/csrc/packet.h -- the packet check (tfrec_amd_enable_burst_packets, include/tfrec_amd.h: "Packet check"): an
// optional stage behind the burst sync and beside the frame check, for packets that carry their own length.  Every set bit c of the
// sync's match track is a candidate: the byte behind it (de-whitened) is a length L, the packet has T = 1 + L + len_add + W / 8
// bytes and ends at k = c + delta(8 T); per captured sample one bit, 1 at k where a candidate that ends there carries its own CRC,
// packed where the track's bit lies; per run a 48-byte record.  The window depends on the data, so crc_kernel's dense bit-sliced
// form does not apply; the candidates are sparse and each is a small serial job, which a wave shares, a byte per lane.  Three
// kernels (capture.h's run_records_init_kernel, packet_kernel, packet_carry_kernel) on the recorder's low-priority lane behind the
// sync's carry kernel; they read the recorder's table and working set, the input bitmap and the match bitmap of the same set --
// complete: their kernels have ended -- and the 2 x 16384 bits and H they carried themselves.  Integers only: the bits are joined by
// OR on a zeroed bitmap, n_seen and n_ok are sums and first_at a minimum, so the order of the atomics cannot matter.  The geometry,
// the run lookup, the chain word and the carry are the frame check's.  Included by frontend.hip (inside namespace tfrec) behind
// crc.h.  tfrec_amd/packet.py restates the result.
#pragma once

static_assert(sizeof(tfrec_amd_burst_packet) == 48 && offsetof(tfrec_amd_burst_packet, bit_offset) == 24 && offsetof(tfrec_amd_burst_packet, n_seen) == 32 &&
		      offsetof(tfrec_amd_burst_packet, n_ok) == 36 && offsetof(tfrec_amd_burst_packet, first_at) == 40 &&
		      offsetof(tfrec_amd_burst_packet, reserved) == 44,
	      "the init kernel copies a table entry's 32 bytes; packet_kernel adds into n_seen and n_ok and takes a 32-bit minimum on first_at");
// run_records_init_kernel's rule -- the entry's 32 bytes, n_seen = n_ok = 0, first_at all ones (the minimum's start and "none"), the
// reserved 0 --; it zeroes the ok bitmap too
template <>
__device__ inline uint32_t run_record_word<tfrec_amd_burst_packet>(const uint32_t *src, int w)
{
	return w < 8 ? src[w] : w == 10 ? 0xffffffffu : 0u;
}

constexpr int kPacketDeltas = 8 * kPacketMaxBytes + 1;   // delta(0 .. 8 T_max)
constexpr int kPacketWaves = kSyncThreads / 64;
constexpr int kPacketWaveWords = (kCrcLds + kPacketWaves - 1) / kPacketWaves;  // the match words a wave walks: 193
static_assert(kPacketCarryWords == 2 * kCrcCarryWords && 4 * (2 * kCrcLds + kPacketDeltas) + 16 < 16384, "packet_kernel's LDS stays under 16 KB");

__device__ inline uint32_t packet_bit(const uint32_t *l, int p) { return (l[p >> 5] >> (p & 31)) & 1u; }

// Block blockIdx.x of stream blockIdx.y, with crc_kernel's geometry and run loop: for every run of the stream that meets the block
// and fits the pool, the candidates that END in the run's part [a, e) of the block.
//   1. LDS: l_x and l_m, word i of each the chain's input bits and match bits at the submit-relative samples b0 - 16384 + 32 i ..
//      + 31 (crc_chain_word on the stage's own carried words and the two bitmaps), as far as a packet that ends in [a, e) can
//      reach back: behind a - delta(8 T_max) and before e.  Match bits ahead of the chain's H available samples read 0, so a
//      candidate is one the chain holds from c on.  l_delta[i] = delta(i), i = 0 .. 8 T_max, once per workgroup.
//   2. Each wave owns a quarter of the 769 match words.  A lane reads one word, a ballot says which are non-zero, and the wave
//      takes those in order, broadcast, bit by bit with ffs on the uniform value: no queue, no counter, no divergent search.
//   3. A candidate at LDS bit cl, the whole wave: lanes 0 .. 7 read the length byte's bits, a ballot and the LSB / MSB rule give
//      the byte, ^ whiten[0] = L.  The wave leaves uniformly if L is out of range or k = c + delta(8 T) lies outside [a, e) -- ahead
//      of both if even the shortest packet would end at or behind e, which keeps every read below that: inside the filled words.
//      Otherwise lane i assembles the bytes i, i + 64, ... of the T: eight single-bit reads at cl + l_delta[..], the whitening XOR.
//   4. The CRC by linearity (packet_table.h): byte j >= skip contributes d_j x^(8 (T - 1 - j)) mod poly -- Horner over the byte's
//      eight bits on x8[T - 1 - j], whatever the width --, the wave XOR-reduces, and the packet checks iff the sum equals i8[n] ^
//      xorout.
//   5. n_seen, n_ok and first_at are wave-uniform registers, joined in LDS; one round of atomics per (run, block).  The ok bit goes
//      to the zeroed bitmap at the run's pool_offset + k with an integer OR: its index is below pool_offset + n <= max_samples.
// tab: x8[276], i8[276], whiten[276] (one byte a word; 0 behind the sequence).
__global__ __launch_bounds__(kSyncThreads) void packet_kernel(const CaptureStage *__restrict__ stage, int stage_cap, const uint2 *__restrict__ cnt,
							       const uint4 *__restrict__ base, uint32_t max_runs, unsigned long long max_samples,
							       const uint32_t *__restrict__ track, const uint32_t *__restrict__ match,
							       const uint32_t *__restrict__ carry, const uint32_t *__restrict__ hist,
							       const uint32_t *__restrict__ tab, PacketSettings ps, tfrec_amd_burst_packet *__restrict__ out,
							       uint32_t *__restrict__ words)
{
	const int b = blockIdx.x, s = blockIdx.y, t = threadIdx.x;
	const int nr = (int)cnt[s].x;  // (<= stage_cap)
	if (nr == 0)
		return;
	const CaptureStage *srow = stage + (size_t)s * stage_cap;
	const uint4 bs = base[s];
	const uint32_t e0 = bs.x;  // the stream's first table entry
	const unsigned long long pool0 = (unsigned long long)bs.z | ((unsigned long long)bs.w << 32);
	__shared__ uint32_t l_seen, l_ok, l_first;
	__shared__ uint32_t l_x[kCrcLds], l_m[kCrcLds];
	__shared__ int l_delta[kPacketDeltas];
	if (t == 0) {
		l_seen = l_ok = 0;
		l_first = 0xffffffffu;
	}
	const int fb = ps.width >> 3;
	const int t_min = 1 + ps.len_min + ps.len_add + fb, t_max = 1 + ps.len_max + ps.len_add + fb;  // (t_max <= 276)
	const unsigned rate = (unsigned)ps.rate;
	for (int i = t; i <= 8 * t_max; i += kSyncThreads)
		l_delta[i] = (int)((768000u * (unsigned)i + rate) / (2u * rate));  // (768000 * 2208 + 96000 < 2^32)
	const int d_min = (int)((768000u * (unsigned)(8 * t_min) + rate) / (2u * rate));
	const int d_max = (int)((768000u * (unsigned)(8 * t_max) + rate) / (2u * rate));  // (<= 16383: the enable call)
	const int b0 = b * kBlockDec, b1 = b0 + kBlockDec;
	int lo, hi;
	capture_run_range(srow, nr, b0, b1, t, kSyncThreads, lo, hi);
	if (lo >= hi)
		return;
	const size_t nw = (size_t)((max_samples + 31) >> 5);
	const int H0 = (int)hist[s];  // (<= 16383)
	const uint32_t *xrow = carry + (size_t)s * kPacketCarryWords, *mrow = xrow + kCrcCarryWords;
	const int lane = t & 63, wave = t >> 6;
	const int w0 = wave * kPacketWaveWords, w1 = w0 + kPacketWaveWords < kCrcLds ? w0 + kPacketWaveWords : kCrcLds;
	const uint32_t inv = (ps.flags & TFREC_AMD_CRC_INVERT) ? 1u : 0u;
	const bool lsb = ps.flags & TFREC_AMD_CRC_LSB;
	const uint32_t mask = ps.width == 32 ? 0xffffffffu : (1u << ps.width) - 1u, top = 1u << (ps.width - 1);
	const uint32_t *x8 = tab, *i8 = tab + kPacketMaxBytes, *wh = tab + 2 * kPacketMaxBytes;
	const int wh0 = (int)wh[0];
	const int org = b0 - kCrcCarryBits;  // LDS bit 0 is this submit-relative sample
	for (int k = lo; k < hi; k++) {
		if ((unsigned long long)e0 + (unsigned)k >= max_runs)
			break;  // (and every later run of the stream: no record)
		const CaptureStage r = srow[k];
		const unsigned long long dst0 = pool0 + r.rank;  // the run's first bit
		const int n = r.end - r.start;  // (1 .. M)
		if (dst0 + (unsigned)n > max_samples)
			continue;  // (uniform) the inputs have no bits of it
		const bool cont = r.flags & TFREC_AMD_RUN_CONTINUES;
		const int H = cont ? H0 : 0;
		const int a = r.start > b0 ? r.start : b0, e = r.end < b1 ? r.end : b1;  // b0 <= a < e <= b1 <= M
		for (int i = t; i < kCrcLds; i += kSyncThreads) {
			const int m0 = org + 32 * i;  // the word's first sample
			uint32_t x = 0u, m = 0u;
			if (m0 + 32 > a - d_max && m0 < e) {
				const int k0 = m0 - r.start;
				x = crc_chain_word(k0, cont, xrow, track, nw, dst0, n);
				m = crc_chain_word(k0, cont, mrow, match, nw, dst0, n);
				const int z = -H - k0;  // the word's bits ahead of the chain's H samples
				if (z > 0)
					m = z >= 32 ? 0u : m & (~0u << z);
			}
			l_x[i] = x;
			l_m[i] = m;
		}
		__syncthreads();
		const int al = a - org, el = e - org;  // [a, e) as LDS bits: 16384 <= al < el <= 24576
		uint32_t seen = 0, ok = 0, first = 0xffffffffu;  // the wave's; uniform
		for (int wb = w0; wb < w1; wb += 64) {
			const uint32_t mine = wb + lane < w1 ? l_m[wb + lane] : 0u;
			unsigned long long any = __ballot(mine != 0u);
			while (any) {
				const int src = __ffsll((long long)any) - 1;
				any &= any - 1ull;
				uint32_t word = (uint32_t)__builtin_amdgcn_readfirstlane((int)__shfl(mine, src));
				while (word) {
					const int cl = 32 * (wb + src) + __ffs((int)word) - 1;  // the candidate, an LDS bit
					word &= word - 1u;
					if (cl + d_min >= el)
						continue;  // the shortest packet ends at or behind e (and every read below stays before e)
					const uint32_t lb = lane < 8 ? packet_bit(l_x, cl + l_delta[lane + 1]) ^ inv : 0u;
					const uint32_t got = (uint32_t)__ballot(lb != 0u) & 0xffu;  // bit q: the q-th bit received
					const int L = (int)(lsb ? got : __brev(got) >> 24) ^ wh0;
					if (L < ps.len_min || L > ps.len_max)
						continue;
					const int T = 1 + L + ps.len_add + fb;
					const int kl = cl + l_delta[8 * T];
					if (kl < al || kl >= el)
						continue;  // it ends in another piece, or behind the burst
					seen++;
					uint32_t acc = 0u;
					for (int j = lane; j < T; j += 64) {
						if (j < ps.skip)
							continue;
						const int *dl = l_delta + 8 * j + 1;
						uint32_t byte = 0u;
#pragma unroll
						for (int q = 0; q < 8; q++)
							byte |= (packet_bit(l_x, cl + dl[q]) ^ inv) << (lsb ? q : 7 - q);
						byte ^= wh[j];
						const uint32_t y = x8[T - 1 - j];
						uint32_t p = 0u;  // byte * y mod poly
#pragma unroll
						for (int q = 7; q >= 0; q--) {
							p = ((p & top) ? (p << 1) ^ ps.poly : p << 1) & mask;
							p ^= ((byte >> q) & 1u) ? y : 0u;
						}
						acc ^= p;
					}
#pragma unroll
					for (int d = 32; d >= 1; d >>= 1)
						acc ^= __shfl_xor(acc, d);
					if (acc == (i8[T - fb - ps.skip] ^ ps.xorout)) {
						const uint32_t kr = (uint32_t)(kl + org - r.start);  // run-relative: < n
						ok++;
						first = kr < first ? kr : first;
						if (lane == 0) {
							const unsigned long long bit = dst0 + kr;
							atomicOr(words + (bit >> 5), 1u << (bit & 31));
						}
					}
				}
			}
		}
		if (lane == 0 && seen) {
			atomicAdd(&l_seen, seen);
			atomicAdd(&l_ok, ok);
			atomicMin(&l_first, first);
		}
		__syncthreads();
		if (t == 0) {
			tfrec_amd_burst_packet *o = out + (e0 + (unsigned)k);
			if (l_seen)
				atomicAdd(&o->n_seen, l_seen);
			if (l_ok) {
				atomicAdd(&o->n_ok, l_ok);
				atomicMin(&o->first_at, l_first);
			}
			l_seen = l_ok = 0;
			l_first = 0xffffffffu;
		}
		__syncthreads();
	}
}

// What the next submit needs of this one, behind packet_kernel on the same stream: crc_carry_kernel's form on both arrays and one
// H.  One workgroup of 512 lanes per stream; if the stream's last run reaches the submit's last sample, has a record and fits the
// pool, lane i builds word i of the chain's last 16384 input bits and of its last 16384 match bits -- out of the old words and the
// run's bits (crc_chain_word) -- and H = min(16383, H' + n), H' = 0 unless it CONTINUES; every lane has read before any writes.
// Otherwise H = 0 and the words stay.
__global__ __launch_bounds__(kCrcCarryWords) void packet_carry_kernel(int n_blocks, const CaptureStage *__restrict__ stage, int stage_cap,
								       const uint2 *__restrict__ cnt, const uint4 *__restrict__ base, uint32_t max_runs,
								       unsigned long long max_samples, const uint32_t *__restrict__ track,
								       const uint32_t *__restrict__ match, uint32_t *__restrict__ carry,
								       uint32_t *__restrict__ hist)
{
	const int s = blockIdx.x, i = threadIdx.x;
	const int nr = (int)cnt[s].x;
	const int M = n_blocks * kBlockDec;
	const uint4 bs = base[s];
	const unsigned long long e0 = bs.x;
	const unsigned long long pool0 = (unsigned long long)bs.z | ((unsigned long long)bs.w << 32);
	uint32_t *xrow = carry + (size_t)s * kPacketCarryWords, *mrow = xrow + kCrcCarryWords;
	uint32_t x = 0u, m = 0u, h = 0u;
	bool open = false;
	if (nr) {
		const CaptureStage r = stage[(size_t)s * stage_cap + (nr - 1)];
		const unsigned long long dst0 = pool0 + r.rank;
		const int n = r.end - r.start;
		if (r.end == M && e0 + (unsigned)(nr - 1) < max_runs && dst0 + (unsigned)n <= max_samples) {
			const bool cont = r.flags & TFREC_AMD_RUN_CONTINUES;
			const long long total = (cont ? (long long)hist[s] : 0) + n;
			const size_t nw = (size_t)((max_samples + 31) >> 5);
			h = (uint32_t)(total < kCrcHist ? total : kCrcHist);
			x = crc_chain_word(n - kCrcCarryBits + 32 * i, cont, xrow, track, nw, dst0, n);
			m = crc_chain_word(n - kCrcCarryBits + 32 * i, cont, mrow, match, nw, dst0, n);
			open = true;
		}
	}
	__syncthreads();
	if (open) {
		xrow[i] = x;
		mrow[i] = m;
	}
	if (i == 0)
		hist[s] = h;
}

hipError_t launch_burst_packet(hipStream_t st, const FrontOut &o, const CaptureBufs &b, const PacketBufs &k)
{
	launch_run_records_init(st, b, k.recs, k.words);
	hipLaunchKernelGGL(packet_kernel, dim3(o.n_blocks, o.n_streams), dim3(kSyncThreads), 0, st, b.stage, b.stage_cap, b.cnt, b.base, b.max_runs,
			   b.max_samples, k.track, k.match, k.carry, k.hist, k.table, k.set, k.recs, k.words);
	hipLaunchKernelGGL(packet_carry_kernel, dim3(o.n_streams), dim3(kCrcCarryWords), 0, st, o.n_blocks, b.stage, b.stage_cap, b.cnt, b.base,
			   b.max_runs, b.max_samples, k.track, k.match, k.carry, k.hist);
	return hipGetLastError();
}
