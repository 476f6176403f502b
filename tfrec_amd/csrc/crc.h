// tfrec_amd/csrc/crc.h -- the frame check (tfrec_amd_enable_burst_crc, include/tfrec_amd.h: "Frame check"): an optional
// stage of the burst track, behind the line code and beside the sync.  Per captured sample of every run of the recorder's table one
// bit, 1 where the N bytes whose last bit sits at the sample -- read at the Framing's symbol centres -- carry their own CRC, packed
// where the track's bit lies; per run a 40-byte record.  A CRC is affine over GF(2) in the bits it covers, so the residue at a sample
// is r0 XORed with a fixed column for every set bit of a fixed-offset window of the track (crc_table.h builds the terms): the sync's
// own form, 32 samples a lane, bit-sliced into W residue planes, funnel-shifted LDS windows.  Three kernels (capture.h's
// run_records_init_kernel, crc_kernel, crc_carry_kernel) on the recorder's low-priority lane behind the code's (or the track's)
// carry kernel; they read the recorder's table and working set, the input bitmap of the same set -- complete: its kernels have
// ended -- and the 16384 input bits and H they carried themselves.  Integers only: the bits are joined by OR on a zeroed bitmap,
// n_ok is a sum and first_at a minimum, so the order of the atomics cannot matter.  The geometry and the run lookup are the sync's;
// the chain word and the carry are its siblings on 512 words.  Included by frontend.hip (inside namespace tfrec) behind linecode.h.
// tfrec_amd/crc.py restates the result.
#pragma once

static_assert(sizeof(tfrec_amd_burst_crc) == 40 && offsetof(tfrec_amd_burst_crc, bit_offset) == 24 && offsetof(tfrec_amd_burst_crc, n_ok) == 32 &&
		      offsetof(tfrec_amd_burst_crc, first_at) == 36,
	      "the init kernel copies a table entry's 32 bytes; crc_kernel adds into n_ok and takes a 32-bit minimum on first_at");
// run_records_init_kernel's rule -- the entry's 32 bytes (its first 24 and its pool_offset), n_ok = 0, first_at all ones: the
// minimum's start and "none" --; it zeroes the check bitmap too
template <>
__device__ inline uint32_t run_record_word<tfrec_amd_burst_crc>(const uint32_t *src, int w)
{
	return w < 8 ? src[w] : w == 8 ? 0u : 0xffffffffu;
}

constexpr int kCrcHist = 16383;      // the input bits ahead of a sample that a frame may need: the largest D
constexpr int kCrcCarryWords = 512;  // per stream: bit c of the carried words is t[c - 16384] of the piece that continues the chain
constexpr int kCrcCarryBits = 32 * kCrcCarryWords;
constexpr int kCrcLds = kCrcCarryWords + kSyncThreads + 1;  // the 16384 bits ahead of the block, the block's, and the funnel's second word
static_assert(kCrcHist < kCrcCarryBits && kCrcLds == 769, "a window begins at bit 1 .. 24544 of LDS: its two words are 0 .. 768");

// sync_chain_word on the 512 carried words: bits k0 .. k0 + 31 of a run's chain, run-relative: t[k] for 0 <= k < n out of the input
// bitmap, where the run's first bit is bit dst0 (the caller has seen that dst0 + n fits the bitmap); for k < 0 what the stream
// carried (bit 16384 + k), if the run CONTINUES; everything else 0.
__device__ inline uint32_t crc_chain_word(int k0, bool cont, const uint32_t *__restrict__ carry, const uint32_t *__restrict__ track, size_t nw,
					  unsigned long long dst0, int n)
{
	uint32_t v = 0;
	if (cont && k0 < 0 && k0 > -(kCrcCarryBits + 32)) {
		const int c = kCrcCarryBits + k0;  // (> -32)
		v = c >= 0 ? sync_fetch(carry, kCrcCarryWords, (unsigned long long)c) : carry[0] << -c;
	}
	if (k0 > -32 && k0 < n) {
		uint32_t g = k0 >= 0 ? sync_fetch(track, nw, dst0 + (unsigned)k0) : sync_fetch(track, nw, dst0) << -k0;
		if (n - k0 < 32)  // the bits behind the run are another run's
			g &= (1u << (n - k0)) - 1u;
		v |= g;
	}
	return v;
}

// Block blockIdx.x of stream blockIdx.y, with sync_kernel's geometry and capture_run_range's lookup: for every run of the stream
// that meets the block and fits the pool, the check track of the run's part of the block.  W: the CRC's width, the number of planes.
//   1. LDS word i holds the chain's input bits at the submit-relative samples b0 - 16384 + 32 i .. + 31 (crc_chain_word), as far as
//      a window of the run's part of the block can need them: those that reach behind a - D and begin before e; 769 words.
//   2. Lane t owns the samples [b0 + 32 t, b0 + 32 t + 32).  Plane p's bit i is bit p of the residue at the lane's sample i; the
//      planes start at the bits of r0.  For every term (off, col) of the table -- a uniform loop, the term read by a uniform index --
//      the lane's window is LDS at bit 16384 + 32 t - off, two words and a funnel shift (the bit index is 1 .. 24544, so the words
//      are 0 .. 768 of the 769), XORed into the planes whose bit is set in col.  The loop over the planes is unrolled and selects by col's uniform bits: the planes stay in
//      registers.
//   3. v = ~(the OR of the planes), masked to the run's part of the block and to the defined samples, k + H >= D; it goes to the
//      zeroed bitmap at the run's pool_offset with two integer ORs, as sync_kernel's: a bit's index is below pool_offset + n <=
//      max_samples.
//   4. n_ok and the first set k are reduced over each wave, then in LDS; one atomicAdd and one 32-bit atomicMin per (run, block).
// The run loop is uniform over the workgroup.
template <int W>
__global__ __launch_bounds__(kSyncThreads) void crc_kernel(const CaptureStage *__restrict__ stage, int stage_cap, const uint2 *__restrict__ cnt,
							    const uint4 *__restrict__ base, uint32_t max_runs, unsigned long long max_samples,
							    const uint32_t *__restrict__ track, const uint32_t *__restrict__ carry,
							    const uint32_t *__restrict__ hist, const uint2 *__restrict__ terms, int n_terms, int D,
							    uint32_t r0, tfrec_amd_burst_crc *__restrict__ out, uint32_t *__restrict__ words)
{
	const int b = blockIdx.x, s = blockIdx.y, t = threadIdx.x;
	const int nr = (int)cnt[s].x;  // (<= stage_cap)
	if (nr == 0)
		return;
	const CaptureStage *srow = stage + (size_t)s * stage_cap;
	const uint4 bs = base[s];
	const uint32_t e0 = bs.x;  // the stream's first table entry
	const unsigned long long pool0 = (unsigned long long)bs.z | ((unsigned long long)bs.w << 32);
	__shared__ uint32_t l_ok, l_first;
	__shared__ uint32_t l_t[kCrcLds];
	if (t == 0) {
		l_ok = 0;
		l_first = 0xffffffffu;
	}
	const int b0 = b * kBlockDec, b1 = b0 + kBlockDec;
	int lo, hi;
	capture_run_range(srow, nr, b0, b1, t, kSyncThreads, lo, hi);
	if (lo >= hi)
		return;
	const size_t nw = (size_t)((max_samples + 31) >> 5);
	const int H0 = (int)hist[s];  // (<= 16383)
	const uint32_t *crow = carry + (size_t)s * kCrcCarryWords;
	const int n0 = b0 + 32 * t;  // the lane's first sample
	for (int k = lo; k < hi; k++) {
		if ((unsigned long long)e0 + (unsigned)k >= max_runs)
			break;  // (and every later run of the stream: no record)
		const CaptureStage r = srow[k];
		const unsigned long long dst0 = pool0 + r.rank;  // the run's first bit
		const int n = r.end - r.start;  // (1 .. M)
		if (dst0 + (unsigned)n > max_samples)
			continue;  // (uniform) the input has no bits of it
		const bool cont = r.flags & TFREC_AMD_RUN_CONTINUES;
		const int H = cont ? H0 : 0;
		const int a = r.start > b0 ? r.start : b0, e = r.end < b1 ? r.end : b1;  // b0 <= a < e <= b1 <= M
		for (int i = t; i < kCrcLds; i += kSyncThreads) {
			const int m0 = b0 - kCrcCarryBits + 32 * i;  // the word's first sample
			l_t[i] = (m0 + 32 > a - D && m0 < e) ? crc_chain_word(m0 - r.start, cont, crow, track, nw, dst0, n) : 0u;
		}
		__syncthreads();
		// the lane's defined samples of the run: [n0 + j0, n0 + j1), with k + H >= D
		const int jd = D - H + r.start - n0;
		int j0 = a > n0 ? a - n0 : 0;
		const int j1 = e - n0 < 32 ? e - n0 : 32;
		j0 = jd > j0 ? jd : j0;
		uint32_t v = 0;
		if (j0 < j1) {
			uint32_t c[W];  // the residue's planes
#pragma unroll
			for (int p = 0; p < W; p++)
				c[p] = 0u - ((r0 >> p) & 1u);
			for (int i = 0; i < n_terms; i++) {
				const uint2 tm = terms[i];  // (off, col): off <= D <= 16383
				const int q = kCrcCarryBits + 32 * t - (int)tm.x;  // (>= 1: off < 16384; word 0 is filled like the others)
				const uint32_t wl = l_t[q >> 5], wh = l_t[(q >> 5) + 1];
				const int sh = q & 31;
				const uint32_t x = sh ? (wl >> sh) | (wh << (32 - sh)) : wl;
#pragma unroll
				for (int p = 0; p < W; p++)
					if ((tm.y >> p) & 1u)
						c[p] ^= x;
			}
			uint32_t any = 0;
#pragma unroll
			for (int p = 0; p < W; p++)
				any |= c[p];
			v = ~any & (j1 - j0 == 32 ? ~0u : ((1u << (j1 - j0)) - 1u) << j0);
			if (v) {
				const long long B = (long long)dst0 + (n0 - r.start);  // bit j of v is bit B + j of the bitmap (B > -32; B + j0 >= 0)
				const long long wi = B >> 5;
				const int sh = (int)(B & 31);
				const uint32_t vl = v << sh, vh = sh ? v >> (32 - sh) : 0u;
				if (vl)  // (B < 0: every set bit lies in vh)
					atomicOr(words + wi, vl);
				if (vh)
					atomicOr(words + wi + 1, vh);
			}
		}
		int ok = __popc(v);
		uint32_t first = v ? (uint32_t)(n0 + (__ffs((int)v) - 1) - r.start) : 0xffffffffu;
#pragma unroll
		for (int d = 32; d >= 1; d >>= 1) {
			ok += __shfl_xor(ok, d);
			const uint32_t of = __shfl_xor(first, d);
			first = of < first ? of : first;
		}
		if ((t & 63) == 0 && ok) {
			atomicAdd(&l_ok, (uint32_t)ok);
			atomicMin(&l_first, first);
		}
		__syncthreads();
		if (t == 0) {
			tfrec_amd_burst_crc *o = out + (e0 + (unsigned)k);
			if (l_ok) {
				atomicAdd(&o->n_ok, l_ok);
				atomicMin(&o->first_at, l_first);
			}
			l_ok = 0;
			l_first = 0xffffffffu;
		}
		__syncthreads();
	}
}

// What the next submit needs of this one, behind crc_kernel on the same stream -- so the kernel that reads carry and hist has ended
// before they are written, and the next submit's reads come behind these writes (DESIGN.md 6t's argument).  sync_carry_kernel's
// history half on 512 words: one workgroup of 512 lanes per stream; if the stream's last run reaches the submit's last sample, has
// a record and fits the pool, lane i builds word i of the chain's last 16384 input bits -- out of the old words and the run's bits,
// combined where the run is shorter than that (crc_chain_word) -- and H = min(16383, H' + n), H' = 0 unless it CONTINUES; every lane
// has read before any writes.  Otherwise H = 0 and the words stay.
__global__ __launch_bounds__(kCrcCarryWords) void crc_carry_kernel(int n_blocks, const CaptureStage *__restrict__ stage, int stage_cap,
								    const uint2 *__restrict__ cnt, const uint4 *__restrict__ base, uint32_t max_runs,
								    unsigned long long max_samples, const uint32_t *__restrict__ track,
								    uint32_t *__restrict__ carry, uint32_t *__restrict__ hist)
{
	const int s = blockIdx.x, i = threadIdx.x;
	const int nr = (int)cnt[s].x;
	const int M = n_blocks * kBlockDec;
	const uint4 bs = base[s];
	const unsigned long long e0 = bs.x;
	const unsigned long long pool0 = (unsigned long long)bs.z | ((unsigned long long)bs.w << 32);
	uint32_t v = 0u, h = 0u;
	bool open = false;
	if (nr) {
		const CaptureStage r = stage[(size_t)s * stage_cap + (nr - 1)];
		const unsigned long long dst0 = pool0 + r.rank;
		const int n = r.end - r.start;
		if (r.end == M && e0 + (unsigned)(nr - 1) < max_runs && dst0 + (unsigned)n <= max_samples) {
			const bool cont = r.flags & TFREC_AMD_RUN_CONTINUES;
			const long long total = (cont ? (long long)hist[s] : 0) + n;
			h = (uint32_t)(total < kCrcHist ? total : kCrcHist);
			v = crc_chain_word(n - kCrcCarryBits + 32 * i, cont, carry + (size_t)s * kCrcCarryWords, track, (size_t)((max_samples + 31) >> 5),
					   dst0, n);
			open = true;
		}
	}
	__syncthreads();
	if (open)
		carry[(size_t)s * kCrcCarryWords + i] = v;
	if (i == 0)
		hist[s] = h;
}

hipError_t launch_burst_crc(hipStream_t st, const FrontOut &o, const CaptureBufs &b, const CrcBufs &k)
{
	launch_run_records_init(st, b, k.recs, k.words);
	const dim3 grid(o.n_blocks, o.n_streams), lanes(kSyncThreads);
#define TFREC_CRC_LAUNCH(W)                                                                                                                       \
	hipLaunchKernelGGL(crc_kernel<W>, grid, lanes, 0, st, b.stage, b.stage_cap, b.cnt, b.base, b.max_runs, b.max_samples, k.track, k.carry, \
			   k.hist, k.terms, k.n_terms, k.reach, k.r0, k.recs, k.words)
	switch (k.width) {  // (the enable call admits these four)
	case 8: TFREC_CRC_LAUNCH(8); break;
	case 16: TFREC_CRC_LAUNCH(16); break;
	case 24: TFREC_CRC_LAUNCH(24); break;
	default: TFREC_CRC_LAUNCH(32); break;
	}
#undef TFREC_CRC_LAUNCH
	hipLaunchKernelGGL(crc_carry_kernel, dim3(o.n_streams), dim3(kCrcCarryWords), 0, st, o.n_blocks, b.stage, b.stage_cap, b.cnt, b.base,
			   b.max_runs, b.max_samples, k.track, k.carry, k.hist);
	return hipGetLastError();
}
