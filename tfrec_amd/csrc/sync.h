// tfrec_amd/csrc/sync.h -- the burst sync (tfrec_amd_enable_burst_sync, include/tfrec_amd.h: tfrec_amd_burst_sync): per
// captured sample of every run of the recorder's table one bit, 1 where the burst track read at P symbol centres that end at the
// sample is the sync word but for at most E places, packed where the track's bit lies; per run a 48-byte record.  Three kernels
// (capture.h's run_records_init_kernel, sync_kernel, sync_carry_kernel) behind the track's on the recorder's low-priority lane;
// they read the recorder's table and working set, the track's bitmap of the same set -- complete: track_kernel has ended -- and
// the 2048 track bits and H they carried themselves.  Integers only: the bits are joined by OR on a zeroed bitmap, n_hits is a sum
// and (best, best_at) one 64-bit minimum, so the order of the atomics cannot matter.  The distances are counted bit-sliced: 32
// samples a lane, eight planes (the form DESIGN.md 6u records).  Included by frontend.hip (inside namespace tfrec) behind track.h.
// tfrec_amd/sync.py restates the result.
#pragma once

static_assert(sizeof(tfrec_amd_burst_sync) == 48 && offsetof(tfrec_amd_burst_sync, bit_offset) == 24 && offsetof(tfrec_amd_burst_sync, n_hits) == 32 &&
		      offsetof(tfrec_amd_burst_sync, best) == 36 && offsetof(tfrec_amd_burst_sync, best_at) == 40 && offsetof(tfrec_amd_burst_sync, reserved) == 44,
	      "the init kernel copies a table entry's 32 bytes; sync_kernel keeps (best << 32) | best_at in the record's last 8 bytes");
// run_records_init_kernel's rule -- the entry's 32 bytes (its first 24 and its pool_offset), n_hits = 0, best = 0xffffffff and the
// 64-bit minimum's start, all ones, in the last 8 bytes (sync_carry_kernel turns them into best_at and the reserved 0) --; it zeroes
// the match bitmap too
template <>
__device__ inline uint32_t run_record_word<tfrec_amd_burst_sync>(const uint32_t *src, int w)
{
	return w < 8 ? src[w] : w == 8 ? 0u : 0xffffffffu;
}

constexpr int kSyncThreads = 256;  // sync_kernel: a workgroup per (stream, block), 32 consecutive samples -- one word -- per lane
constexpr int kSyncHist = 2047;       // the track bits ahead of a sample that a distance may need: the largest span
constexpr int kSyncCarryWords = 64;   // per stream: bit c of the carried words is t[c - 2048] of the piece that continues the chain
constexpr int kSyncCarryBits = 32 * kSyncCarryWords;
constexpr int kSyncLds = kSyncCarryWords + kSyncThreads + 1;  // the 2048 bits ahead of the block, the block's, and the funnel's second word
constexpr int kSyncPlanes = 8;        // a distance is at most 64, and the counter starts at 127 - E
static_assert(kBlockDec == 32 * kSyncThreads && kSyncHist < kSyncCarryBits, "a lane builds one word");

// 32 bits of a bitmap of nw words from bit p on; words behind the bitmap read 0
__device__ inline uint32_t sync_fetch(const uint32_t *__restrict__ w, size_t nw, unsigned long long p)
{
	const size_t i = (size_t)(p >> 5);
	const int sh = (int)(p & 31);
	const uint32_t lo = i < nw ? w[i] : 0u;
	if (!sh)
		return lo;
	const uint32_t hi = i + 1 < nw ? w[i + 1] : 0u;
	return (lo >> sh) | (hi << (32 - sh));
}

// Bits k0 .. k0 + 31 of a run's chain, run-relative: t[k] for 0 <= k < n out of the track's bitmap, where the run's first bit is
// bit dst0 (the caller has seen that dst0 + n fits the bitmap); for k < 0 what the stream carried (bit 2048 + k), if the run
// CONTINUES; everything else 0.
__device__ inline uint32_t sync_chain_word(int k0, bool cont, const uint32_t *__restrict__ carry, const uint32_t *__restrict__ track, size_t nw,
					   unsigned long long dst0, int n)
{
	uint32_t v = 0;
	if (cont && k0 < 0 && k0 > -(kSyncCarryBits + 32)) {
		const int c = kSyncCarryBits + k0;  // (> -32)
		v = c >= 0 ? sync_fetch(carry, kSyncCarryWords, (unsigned long long)c) : carry[0] << -c;
	}
	if (k0 > -32 && k0 < n) {
		uint32_t g = k0 >= 0 ? sync_fetch(track, nw, dst0 + (unsigned)k0) : sync_fetch(track, nw, dst0) << -k0;
		if (n - k0 < 32)  // the bits behind the run are another run's
			g &= (1u << (n - k0)) - 1u;
		v |= g;
	}
	return v;
}

// Block blockIdx.x of stream blockIdx.y, with track_kernel's geometry and capture_run_range's lookup: for every run of the stream
// that meets the block (the range [lo, hi) of the staged runs) and fits the pool, the match track of the run's part of the block.
//   1. LDS word i holds the chain's bits at the submit-relative samples b0 - 2048 + 32 i .. + 31 (sync_chain_word: the track's
//      bitmap where they lie in this submit -- a run's pool region is contiguous --, the carried words ahead of it), as far as a
//      distance of the block's part can need them; 321 words.
//   2. Lane t owns the samples [b0 + 32 t, b0 + 32 t + 32).  For pattern bit j its 32 comparisons are one unaligned window of LDS
//      at bit 2048 + 32 t - delta(j) -- two words and a funnel shift, XORed with 0 or ~0 --, added into eight bit planes by a ripple
//      of half adders: plane p's bit i is bit p of s = d + 127 - E at the lane's sample i.  delta() is computed once per workgroup.
//   3. d > E is plane 7 (s >= 128; s <= 191); d >= P - E is compared on the planes from the top; the undefined positions
//      (k + H < span) and the samples of no run are masked off.  The minimum of d (and with BOTH the maximum, for P - d) over the lane's defined samples is found
//      on the planes too, by narrowing a candidate set from the top plane down; the first candidate is best_at.
//   4. The lane's word goes to the bitmap at the run's pool_offset with two integer ORs, as track_kernel's does: a bit's index is
//      below pool_offset + n <= max_samples.  n_hits and the key (best << 32) | k are reduced over each wave, then in LDS; one
//      round of atomics per (run, block).
// The run loop is uniform over the workgroup.
__global__ __launch_bounds__(kSyncThreads) void sync_kernel(const CaptureStage *__restrict__ stage, int stage_cap, const uint2 *__restrict__ cnt,
							     const uint4 *__restrict__ base, uint32_t max_runs, unsigned long long max_samples,
							     const uint32_t *__restrict__ track, const uint32_t *__restrict__ carry,
							     const uint32_t *__restrict__ hist, int rate, int P, int E, uint32_t flags,
							     unsigned long long pattern, tfrec_amd_burst_sync *__restrict__ out, uint32_t *__restrict__ words)
{
	const int b = blockIdx.x, s = blockIdx.y, t = threadIdx.x;
	const int nr = (int)cnt[s].x;  // (<= stage_cap)
	if (nr == 0)
		return;
	const CaptureStage *srow = stage + (size_t)s * stage_cap;
	const uint4 bs = base[s];
	const uint32_t e0 = bs.x;  // the stream's first table entry
	const unsigned long long pool0 = (unsigned long long)bs.z | ((unsigned long long)bs.w << 32);
	__shared__ uint32_t l_hits;
	__shared__ unsigned long long l_best;
	__shared__ int l_delta[64];
	__shared__ uint32_t l_kb[kSyncPlanes], l_tb[kSyncPlanes];  // 0 or ~0 by the bits of K = 127 - E and of P - E + K: the planes' start,
								   // and what d >= P - E is compared with -- in LDS, so that sixteen
								   // loop-invariant masks do not sit in scalar registers
	__shared__ uint32_t l_t[kSyncLds];
	if (t == 0) {
		l_hits = 0;
		l_best = ~0ull;
	}
	const int K = 127 - E;  // (E <= 31)
	if (t < kSyncPlanes) {
		l_kb[t] = 0u - (uint32_t)((K >> t) & 1);
		l_tb[t] = 0u - (uint32_t)(((P - E + K) >> t) & 1);
	}
	if (t < P)
		l_delta[t] = (int)((768000u * (unsigned)t + (unsigned)rate) / (2u * (unsigned)rate));  // (below 2^26)
	const int b0 = b * kBlockDec, b1 = b0 + kBlockDec;
	int lo, hi;
	capture_run_range(srow, nr, b0, b1, t, kSyncThreads, lo, hi);
	if (lo >= hi)
		return;
	const size_t nw = (size_t)((max_samples + 31) >> 5);
	const int span = l_delta[P - 1];
	const int H0 = (int)hist[s];  // (<= 2047)
	const uint32_t *crow = carry + (size_t)s * kSyncCarryWords;
	const int n0 = b0 + 32 * t;   // the lane's first sample
	const bool both = flags & TFREC_AMD_SYNC_BOTH;
	for (int k = lo; k < hi; k++) {
		if ((unsigned long long)e0 + (unsigned)k >= max_runs)
			break;  // (and every later run of the stream: no record)
		const CaptureStage r = srow[k];
		const unsigned long long dst0 = pool0 + r.rank;  // the run's first bit
		const int n = r.end - r.start;  // (1 .. M)
		if (dst0 + (unsigned)n > max_samples)
			continue;  // (uniform) the track has no bits of it
		const bool cont = r.flags & TFREC_AMD_RUN_CONTINUES;
		const int H = cont ? H0 : 0;
		const int a = r.start > b0 ? r.start : b0, e = r.end < b1 ? r.end : b1;  // b0 <= a < e <= b1 <= M
		for (int i = t; i < kSyncLds; i += kSyncThreads) {
			const int m0 = b0 - kSyncCarryBits + 32 * i;  // the word's first sample
			l_t[i] = (m0 + 32 > a - kSyncHist && m0 < e)
					 ? sync_chain_word(m0 - r.start, cont, crow, track, nw, dst0, n)
					 : 0u;
		}
		__syncthreads();
		// the lane's defined samples of the run: [n0 + j0, n0 + j1), with k + H >= span
		const int jd = span - H + r.start - n0;
		int j0 = a > n0 ? a - n0 : 0;
		const int j1 = e - n0 < 32 ? e - n0 : 32;
		j0 = jd > j0 ? jd : j0;
		uint32_t m = 0;
		unsigned long long key = ~0ull;
		if (j0 < j1) {
			const uint32_t mask = (j1 - j0 == 32 ? ~0u : ((1u << (j1 - j0)) - 1u) << j0);
			uint32_t c[kSyncPlanes];  // the planes of s = d + K: bit 7 of s is d > E
#pragma unroll
			for (int p = 0; p < kSyncPlanes; p++)
				c[p] = l_kb[p];
			for (int j = 0; j < P; j++) {
				const int q = kSyncCarryBits + 32 * t - l_delta[j];  // (>= 1: delta <= 2047)
				const uint32_t wl = l_t[q >> 5], wh = l_t[(q >> 5) + 1];
				const int sh = q & 31;
				uint32_t x = sh ? (wl >> sh) | (wh << (32 - sh)) : wl;
				x ^= 0u - (uint32_t)((pattern >> j) & 1ull);  // 1 where the track differs from the pattern's bit
#pragma unroll
				for (int p = 0; p < kSyncPlanes; p++) {
					const uint32_t carry_out = c[p] & x;
					c[p] ^= x;
					x = carry_out;
				}
			}
			m = ~c[kSyncPlanes - 1];
			uint32_t cand = mask;
			uint32_t best = 0;  // the smallest s, then d
#pragma unroll
			for (int p = kSyncPlanes - 1; p >= 0; p--) {
				const uint32_t z = cand & ~c[p];
				cand = z ? z : cand;
				best |= z ? 0u : 1u << p;
			}
			best -= (uint32_t)K;
			if (both) {
				uint32_t lt = 0u, eq = ~0u;  // s < P - E + K: d < P - E
#pragma unroll
				for (int p = kSyncPlanes - 1; p >= 0; p--) {
					const uint32_t tb = l_tb[p];
					lt |= eq & ~c[p] & tb;
					eq &= ~(c[p] ^ tb);
				}
				m |= ~lt;
				uint32_t cmax = mask;
				uint32_t dmax = 0;
#pragma unroll
				for (int p = kSyncPlanes - 1; p >= 0; p--) {
					const uint32_t z = cmax & c[p];
					cmax = z ? z : cmax;
					dmax |= z ? 1u << p : 0u;
				}
				const uint32_t fold = (uint32_t)(P + K) - dmax;  // P - d of the largest d
				if (fold < best) {
					best = fold;
					cand = cmax;
				} else if (fold == best) {
					cand |= cmax;
				}
			}
			m &= mask;
			key = ((unsigned long long)best << 32) | (uint32_t)(n0 + (__ffs((int)cand) - 1) - r.start);
			if (m) {
				const long long D = (long long)dst0 + (n0 - r.start);  // bit j of m is bit D + j of the bitmap (D > -32; D + j0 >= 0)
				const long long wi = D >> 5;
				const int sh = (int)(D & 31);
				const uint32_t ml = m << sh, mh = sh ? m >> (32 - sh) : 0u;
				if (ml)  // (D < 0: every set bit lies in mh)
					atomicOr(words + wi, ml);
				if (mh)
					atomicOr(words + wi + 1, mh);
			}
		}
		int hits = __popc(m);
#pragma unroll
		for (int d = 32; d >= 1; d >>= 1) {
			hits += __shfl_xor(hits, d);
			const unsigned long long ok = __shfl_xor(key, d);
			key = ok < key ? ok : key;
		}
		if ((t & 63) == 0) {
			if (hits)
				atomicAdd(&l_hits, (uint32_t)hits);
			if (key != ~0ull)
				atomicMin(&l_best, key);
		}
		__syncthreads();
		if (t == 0) {
			tfrec_amd_burst_sync *o = out + (e0 + (unsigned)k);
			if (l_hits)
				atomicAdd(&o->n_hits, l_hits);
			if (l_best != ~0ull)
				atomicMin(reinterpret_cast<unsigned long long *>(&o->best_at), l_best);
			l_hits = 0;
			l_best = ~0ull;
		}
		__syncthreads();
	}
}

// What the next submit needs of this one, and the records' last words, behind sync_kernel on the same stream -- so the kernel that
// reads carry and hist has ended before they are written, and the next submit's reads come behind these writes.  One workgroup of
// 64 lanes per stream.  If the stream's last run reaches the submit's last sample, has a record and fits the pool, lane i builds
// word i of the chain's last 2048 bits -- out of the old words and the run's bits, combined where the run is shorter than that
// (sync_chain_word) --, and H = min(2047, H' + n), H' = 0 unless it CONTINUES; every lane has read before any writes.  Otherwise H
// = 0 and the words stay.  The stream's records get best = the minimum's high word, best_at = its low word (0 where there is
// none) and the reserved 0.
__global__ __launch_bounds__(kSyncCarryWords) void sync_carry_kernel(int n_blocks, const CaptureStage *__restrict__ stage, int stage_cap,
								      const uint2 *__restrict__ cnt, const uint4 *__restrict__ base, uint32_t max_runs,
								      unsigned long long max_samples, const uint32_t *__restrict__ track,
								      uint32_t *__restrict__ carry, uint32_t *__restrict__ hist,
								      tfrec_amd_burst_sync *__restrict__ out)
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
			h = (uint32_t)(total < kSyncHist ? total : kSyncHist);
			v = sync_chain_word(n - kSyncCarryBits + 32 * i, cont, carry + (size_t)s * kSyncCarryWords, track,
					    (size_t)((max_samples + 31) >> 5), dst0, n);
			open = true;
		}
	}
	for (int k = i; k < nr && e0 + (unsigned)k < max_runs; k += kSyncCarryWords) {
		uint32_t *w = reinterpret_cast<uint32_t *>(out + (e0 + (unsigned)k));
		const uint32_t best = w[11], at = w[10];
		w[9] = best;
		w[10] = best == 0xffffffffu ? 0u : at;
		w[11] = 0u;
	}
	__syncthreads();
	if (open)
		carry[(size_t)s * kSyncCarryWords + i] = v;
	if (i == 0)
		hist[s] = h;
}

hipError_t launch_burst_sync(hipStream_t st, const FrontOut &o, const CaptureBufs &b, const SyncBufs &k)
{
	launch_run_records_init(st, b, k.recs, k.words);
	hipLaunchKernelGGL(sync_kernel, dim3(o.n_blocks, o.n_streams), dim3(kSyncThreads), 0, st, b.stage, b.stage_cap, b.cnt, b.base, b.max_runs,
			   b.max_samples, k.track, k.carry, k.hist, k.rate, k.n_bits, k.max_errors, k.flags, k.pattern, k.recs, k.words);
	hipLaunchKernelGGL(sync_carry_kernel, dim3(o.n_streams), dim3(kSyncCarryWords), 0, st, o.n_blocks, b.stage, b.stage_cap, b.cnt, b.base,
			   b.max_runs, b.max_samples, k.track, k.carry, k.hist, k.recs);
	return hipGetLastError();
}
