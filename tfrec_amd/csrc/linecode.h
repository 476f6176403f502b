// tfrec_amd/csrc/linecode.h -- the line code (tfrec_amd_enable_burst_code, include/tfrec_amd.h: "Line code"): an optional
// stage of the burst track, between the track and the sync.  Per captured sample of every run of the recorder's table one bit, the
// track's bit XORed with the track's bits delta(j) samples ahead of it for every set tap j -- a self-synchronising descrambler, a
// differential decoder --, complemented under INVERT, packed where the track's bit lies; per run a tfrec_amd_track record.  Three
// kernels (capture.h's run_records_init_kernel<tfrec_amd_track>, linecode_kernel, linecode_carry_kernel) behind the track's on the
// recorder's low-priority lane and ahead of the sync's, which is then launched on the coded bitmap; they read the recorder's table
// and working set, the track's records and bitmap of the same set -- complete: the track's kernels have ended -- and the 2048 track
// bits and H they carried themselves.  Integers only: the bits are joined by OR on a zeroed bitmap and n_ones is a sum, so the order
// of the atomics cannot matter.  The geometry, the run lookup, the LDS fill (sync_chain_word) and the carry are the sync's.  Included
// by frontend.hip (inside namespace tfrec) behind sync.h.  tfrec_amd/linecode.py restates the result.
#pragma once

constexpr int kCodeTaps = 32;  // a tap per bit of the settings' word: bit j - 1 is a delay of j symbols

// sync_chain_word's bits k0 .. k0 + 31 with those ahead of the H available ones cleared: a chain shorter than 2047 samples has
// nothing ahead of its first one, whatever the carried words still hold of an earlier chain
__device__ inline uint32_t code_chain_word(int k0, int H, bool cont, const uint32_t *__restrict__ carry, const uint32_t *__restrict__ track, size_t nw,
					   unsigned long long dst0, int n)
{
	const uint32_t v = sync_chain_word(k0, cont, carry, track, nw, dst0, n);
	const int z = -H - k0;  // the word's bits below z lie ahead of the chain
	return z <= 0 ? v : z >= 32 ? 0u : v & (~0u << z);
}

// Block blockIdx.x of stream blockIdx.y, with sync_kernel's geometry and capture_run_range's lookup: for every run of the stream
// that meets the block and fits the pool, the coded track of the run's part of the block.
//   1. LDS word i holds the chain's track bits at the submit-relative samples b0 - 2048 + 32 i .. + 31, as sync_kernel's (321 words).
//   2. Lane t owns the samples [b0 + 32 t, b0 + 32 t + 32).  Its word is the window at bit 2048 + 32 t -- LDS word 64 + t -- XORed
//      with the window at 2048 + 32 t - delta(j) for every set tap j: two words and a funnel shift each.  delta() is computed once
//      per workgroup.  The loop over the taps is uniform.
//   3. The word is complemented under INVERT, masked to the run's part of the block and joined to the zeroed bitmap at the run's
//      pool_offset with two integer ORs, as track_kernel's: a bit's index is below pool_offset + n <= max_samples.
//   4. n_ones is reduced over each wave, then in LDS; one atomic per (run, block).  last_over is the track's record's, final since
//      the track's kernels have ended: the workgroup of the block the run starts in copies it, for a run that does not fit too.
__global__ __launch_bounds__(kSyncThreads) void linecode_kernel(const CaptureStage *__restrict__ stage, int stage_cap, const uint2 *__restrict__ cnt,
								 const uint4 *__restrict__ base, uint32_t max_runs, unsigned long long max_samples,
								 const uint32_t *__restrict__ track, const tfrec_amd_track *__restrict__ trecs,
								 const uint32_t *__restrict__ carry, const uint32_t *__restrict__ hist, int rate,
								 uint32_t taps, uint32_t flags, tfrec_amd_track *__restrict__ out,
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
	__shared__ uint32_t l_ones;
	__shared__ int l_delta[kCodeTaps];  // l_delta[j - 1] = delta(j)
	__shared__ uint32_t l_t[kSyncLds];
	if (t == 0)
		l_ones = 0;
	if (t < kCodeTaps)
		l_delta[t] = (int)((768000u * (unsigned)(t + 1) + (unsigned)rate) / (2u * (unsigned)rate));  // (below 2^26)
	const int b0 = b * kBlockDec, b1 = b0 + kBlockDec;
	int lo, hi;
	capture_run_range(srow, nr, b0, b1, t, kSyncThreads, lo, hi);
	if (lo >= hi)
		return;
	const size_t nw = (size_t)((max_samples + 31) >> 5);
	const int H0 = (int)hist[s];  // (<= 2047)
	const uint32_t *crow = carry + (size_t)s * kSyncCarryWords;
	const int n0 = b0 + 32 * t;  // the lane's first sample
	const uint32_t inv = (flags & TFREC_AMD_CODE_INVERT) ? ~0u : 0u;
	for (int k = lo; k < hi; k++) {
		if ((unsigned long long)e0 + (unsigned)k >= max_runs)
			break;  // (and every later run of the stream: no record)
		const CaptureStage r = srow[k];
		if (t == 0 && r.start >= b0)  // the run starts in this block
			out[e0 + (unsigned)k].last_over = trecs[e0 + (unsigned)k].last_over;
		const unsigned long long dst0 = pool0 + r.rank;  // the run's first bit
		const int n = r.end - r.start;  // (1 .. M)
		if (dst0 + (unsigned)n > max_samples)
			continue;  // (uniform) the track has no bits of it
		const bool cont = r.flags & TFREC_AMD_RUN_CONTINUES;
		const int H = cont ? H0 : 0;
		const int a = r.start > b0 ? r.start : b0, e = r.end < b1 ? r.end : b1;  // b0 <= a < e <= b1 <= M
		for (int i = t; i < kSyncLds; i += kSyncThreads) {
			const int m0 = b0 - kSyncCarryBits + 32 * i;  // the word's first sample
			l_t[i] = (m0 + 32 > a - kSyncHist && m0 < e) ? code_chain_word(m0 - r.start, H, cont, crow, track, nw, dst0, n) : 0u;
		}
		__syncthreads();
		const int j0 = a > n0 ? a - n0 : 0, j1 = e - n0 < 32 ? e - n0 : 32;  // the lane's samples of the run: [n0 + j0, n0 + j1)
		uint32_t w = 0;
		if (j0 < j1) {
			w = l_t[kSyncCarryWords + t] ^ inv;
			for (uint32_t rest = taps; rest; rest &= rest - 1u) {
				const int q = kSyncCarryBits + 32 * t - l_delta[__ffs((int)rest) - 1];  // (>= 1: delta <= 2047)
				const uint32_t wl = l_t[q >> 5], wh = l_t[(q >> 5) + 1];
				const int sh = q & 31;
				w ^= sh ? (wl >> sh) | (wh << (32 - sh)) : wl;
			}
			w &= (j1 - j0 == 32 ? ~0u : ((1u << (j1 - j0)) - 1u) << j0);
			if (w) {
				const long long D = (long long)dst0 + (n0 - r.start);  // bit j of w is bit D + j of the bitmap (D > -32; D + j0 >= 0)
				const long long wi = D >> 5;
				const int sh = (int)(D & 31);
				const uint32_t wl = w << sh, wh = sh ? w >> (32 - sh) : 0u;
				if (wl)  // (D < 0: every set bit lies in wh)
					atomicOr(words + wi, wl);
				if (wh)
					atomicOr(words + wi + 1, wh);
			}
		}
		int ones = __popc(w);
#pragma unroll
		for (int d = 32; d >= 1; d >>= 1)
			ones += __shfl_xor(ones, d);
		if ((t & 63) == 0 && ones)
			atomicAdd(&l_ones, (uint32_t)ones);
		__syncthreads();
		if (t == 0) {
			if (l_ones)
				atomicAdd(&out[e0 + (unsigned)k].n_ones, l_ones);
			l_ones = 0;
		}
		__syncthreads();
	}
}

// What the next submit needs of this one, behind linecode_kernel on the same stream -- so the kernel that reads carry and hist has
// ended before they are written, and the next submit's reads come behind these writes (DESIGN.md 6t's argument).  sync_carry_kernel's
// history half on the code's own words: one workgroup of 64 lanes per stream; if the stream's last run reaches the submit's last
// sample, has a record and fits the pool, lane i builds word i of the chain's last 2048 TRACK bits and H = min(2047, H' + n), H' = 0
// unless it CONTINUES; every lane has read before any writes.  Otherwise H = 0 and the words stay.
__global__ __launch_bounds__(kSyncCarryWords) void linecode_carry_kernel(int n_blocks, const CaptureStage *__restrict__ stage, int stage_cap,
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
			const int H = cont ? (int)hist[s] : 0;
			const long long total = (long long)H + n;
			h = (uint32_t)(total < kSyncHist ? total : kSyncHist);
			v = code_chain_word(n - kSyncCarryBits + 32 * i, H, cont, carry + (size_t)s * kSyncCarryWords, track,
					    (size_t)((max_samples + 31) >> 5), dst0, n);
			open = true;
		}
	}
	__syncthreads();
	if (open)
		carry[(size_t)s * kSyncCarryWords + i] = v;
	if (i == 0)
		hist[s] = h;
}

hipError_t launch_burst_code(hipStream_t st, const FrontOut &o, const CaptureBufs &b, const CodeBufs &k)
{
	launch_run_records_init(st, b, k.recs, k.words);
	hipLaunchKernelGGL(linecode_kernel, dim3(o.n_blocks, o.n_streams), dim3(kSyncThreads), 0, st, b.stage, b.stage_cap, b.cnt, b.base, b.max_runs,
			   b.max_samples, k.track, k.trecs, k.carry, k.hist, k.rate, k.taps, k.flags, k.recs, k.words);
	hipLaunchKernelGGL(linecode_carry_kernel, dim3(o.n_streams), dim3(kSyncCarryWords), 0, st, o.n_blocks, b.stage, b.stage_cap, b.cnt, b.base,
			   b.max_runs, b.max_samples, k.track, k.carry, k.hist);
	return hipGetLastError();
}
