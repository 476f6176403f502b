// tfrec_amd/csrc/track.h -- the burst track (tfrec_amd_enable_burst_track, include/tfrec_amd.h: tfrec_amd_track): per
// captured sample of every run of the recorder's table one bit, the sign of a quadrature discriminator about the stream's centre,
// boxcar-smoothed over L products, packed where the sample's pair lies in the pool; per run a 40-byte record.  Three kernels
// (capture.h's run_records_init_kernel, track_kernel, track_carry_kernel) behind the clock's on the recorder's low-priority lane;
// they read the recorder's table and working set, the decimated samples, the FINAL trigger mask and the 16 pairs and the chain
// position they carried themselves, and nothing a demodulator owns -- not even prevdec.  Exact integers only: the bits are joined
// by OR on a zeroed bitmap, n_ones is a sum and last_over a maximum, so the order of the atomics cannot matter.  Included by
// frontend.hip (inside namespace tfrec) behind clock.h.  tfrec_amd/track.py restates the result.
#pragma once

static_assert(sizeof(tfrec_amd_track) == 40 && offsetof(tfrec_amd_track, bit_offset) == 24 && offsetof(tfrec_amd_track, last_over) == 32 &&
		      offsetof(tfrec_amd_track, n_ones) == 36 && offsetof(tfrec_amd_run, pool_offset) == 24 && sizeof(tfrec_amd_run) == 32,
	      "the init kernel copies a table entry's 32 bytes: its first 24 and its pool_offset");
// run_records_init_kernel's rule -- the entry's 32 bytes (its first 24 and its pool_offset), last_over = -1, n_ones = 0 --; it zeroes
// the track's bitmap too
template <>
__device__ inline uint32_t run_record_word<tfrec_amd_track>(const uint32_t *src, int w)
{
	return w < 8 ? src[w] : w == 8 ? 0xffffffffu : 0u;
}

constexpr int kTrackThreads = 256;  // track_kernel: a workgroup per (stream, block), 32 consecutive samples -- one word -- per lane
constexpr int kTrackAhead = 16;  // the pairs kept ahead of a block: the largest L
constexpr int kTrackSlots = kBlockDec + kTrackAhead;
static_assert(kBlockDec == 32 * kTrackThreads && kTuneN == 4096, "a lane builds one word; the centre's index is one of 4096");

// Where slot q (the pair at block-relative sample q - 16) lies in LDS: a word of padding per 32, so that the lanes of a wave,
// whose slots lie 32 apart, read 33 apart -- every bank once
__device__ inline int track_slot(int q) { return q + (q >> 5); }
constexpr int kTrackLds = kTrackSlots + (kTrackSlots >> 5) + 1;

// Block blockIdx.x of stream blockIdx.y, with burst_accum_kernel's geometry and capture_run_range's lookup: for every run of the
// stream that meets the block (the range [lo, hi) of the staged runs) the track of the run's part of the block.
//   1. The block's 8192 pairs and the 16 ahead of it into LDS, coalesced: the 16 are the row's own, or for block 0 the stream's
//      carried ones (track_carry_kernel).  A block without a run ends before that.
//   2. Lane t owns the samples [b0 + 32 t, b0 + 32 t + 32).  With cf = the chain's first sample, submit-relative (the run's start,
//      less prior in a CONTINUES run: >= -16), v'(m) = crs C[r] - dot S[r] of the pairs at m and m - 1 for m > cf and 0 for m <= cf:
//      the sum over i < min(L, k + prior) of v[k - i] is then the sum of v'(m - i) over all i < L, which slides: + v'(m) - v'(m - L).
//      No pair ahead of cf is used and none ahead of slot 0 is addressed (m - L >= b0 - 15).  |v'| < 2^47, the sum < 2^51.
//   3. The lane's word goes to the bitmap at the run's pool_offset with two integer ORs (the word straddles two of the
//      bitmap's unless the offset is a multiple of 32) -- only where the run's pairs fit the pool, as capture_copy_kernel decides
//      it, which also keeps every word inside the bitmap: a bit's index is below pool_offset + n <= max_samples.
//   4. n_ones (popcounts) and last_over (the highest mask bit among the lane's samples of the run) are reduced over each wave,
//      then in LDS; one round of atomics per (run, block).
// The run loop is uniform over the workgroup.  No floating point.
__global__ __launch_bounds__(kTrackThreads) void track_kernel(const uint32_t *__restrict__ dec, size_t dec_stride,
							       const unsigned long long *__restrict__ mask, size_t mask_stride,
							       const CaptureStage *__restrict__ stage, int stage_cap,
							       const uint2 *__restrict__ cnt, const uint4 *__restrict__ base, uint32_t max_runs,
							       unsigned long long max_samples, const int32_t *__restrict__ centre,
							       const uint32_t *__restrict__ carry, const uint32_t *__restrict__ prior, int L,
							       tfrec_amd_track *__restrict__ out, uint32_t *__restrict__ words)
{
	const int b = blockIdx.x, s = blockIdx.y, t = threadIdx.x;
	const int nr = (int)cnt[s].x;  // (<= stage_cap)
	if (nr == 0)
		return;
	const CaptureStage *srow = stage + (size_t)s * stage_cap;
	const uint4 bs = base[s];
	const unsigned long long e0 = bs.x;  // the stream's first table entry
	const unsigned long long pool0 = (unsigned long long)bs.z | ((unsigned long long)bs.w << 32);
	__shared__ int l_last;
	__shared__ uint32_t l_ones;
	__shared__ uint32_t l_z[kTrackLds];
	if (t == 0) {
		l_last = -1;
		l_ones = 0;
	}
	const int b0 = b * kBlockDec, b1 = b0 + kBlockDec;
	int lo, hi;
	capture_run_range(srow, nr, b0, b1, t, kTrackThreads, lo, hi);
	if (lo >= hi)
		return;
	const uint32_t *row = dec + (size_t)s * dec_stride;
	for (int q = t; q < kTrackSlots; q += kTrackThreads) {
		const int m = b0 - kTrackAhead + q;  // (m < 0: block 0's first 16 slots)
		l_z[track_slot(q)] = m >= 0 ? row[m] : carry[(size_t)s * kTrackAhead + q];
	}
	__syncthreads();
	const int ri = centre[s] & (kTuneN - 1);
	const long long C = kTuneCos[ri], S = kTuneCos[(ri - kTuneN / 4) & (kTuneN - 1)];
	const int pr = (int)prior[s];  // (<= 16)
	const int n0 = b0 + 32 * t;    // the lane's first sample
	const unsigned long long *mrow = mask + (size_t)s * mask_stride;
	// v'(m) of step 2, m > cf: slots m - b0 + 16 and the one ahead of it
	auto vp = [&](int m) -> long long {
		const int q = m - b0 + kTrackAhead;
		const uint32_t w = l_z[track_slot(q)], wp = l_z[track_slot(q - 1)];
		const int I = (int16_t)(w & 0xffffu), Q = (int16_t)(w >> 16);
		const int Ip = (int16_t)(wp & 0xffffu), Qp = (int16_t)(wp >> 16);
		const long long dot = (long long)(I * Ip) + (long long)(Q * Qp), crs = (long long)(Q * Ip) - (long long)(I * Qp);
		return crs * C - dot * S;
	};
	for (int k = lo; k < hi; k++) {
		if (e0 + (unsigned)k >= max_runs)
			break;  // (and every later run of the stream: no record)
		const CaptureStage r = srow[k];
		const int cf = r.start - ((r.flags & TFREC_AMD_RUN_CONTINUES) ? pr : 0);
		const int a = r.start > b0 ? r.start : b0, e = r.end < b1 ? r.end : b1;  // b0 <= a < e <= b1 <= M
		const int j0 = a > n0 ? a - n0 : 0, j1 = e - n0 < 32 ? e - n0 : 32;  // the lane's samples of the run: [n0 + j0, n0 + j1)
		uint32_t w = 0;
		int last = -1;
		if (j0 < j1) {
			long long sum = 0;
			for (int i = 0; i < L; i++) {
				const int m = n0 + j0 - i;
				sum += m > cf ? vp(m) : 0;
			}
			w = (uint32_t)(sum > 0) << j0;
			for (int j = j0 + 1; j < j1; j++) {
				const int m = n0 + j;  // (> a >= cf)
				sum += vp(m) - (m - L > cf ? vp(m - L) : 0);
				w |= (uint32_t)(sum > 0) << j;
			}
			uint32_t mb = (uint32_t)(mrow[n0 >> 6] >> (n0 & 32));
			mb &= (j1 - j0 == 32 ? ~0u : ((1u << (j1 - j0)) - 1u) << j0);
			if (mb)
				last = n0 + 31 - __clz((int)mb) - r.start;
			const unsigned long long dst0 = pool0 + r.rank;  // the run's first bit
			if (w && dst0 + (unsigned)(r.end - r.start) <= max_samples) {
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
		for (int d = 32; d >= 1; d >>= 1) {
			ones += __shfl_xor(ones, d);
			const int ol = __shfl_xor(last, d);
			last = ol > last ? ol : last;
		}
		if ((t & 63) == 0) {
			if (ones)
				atomicAdd(&l_ones, (uint32_t)ones);
			if (last >= 0)
				atomicMax(&l_last, last);
		}
		__syncthreads();
		if (t == 0) {
			tfrec_amd_track *o = out + (e0 + (unsigned)k);
			if (l_ones)
				atomicAdd(&o->n_ones, l_ones);
			if (l_last >= 0)
				atomicMax(&o->last_over, l_last);
			l_ones = 0;
			l_last = -1;
		}
		__syncthreads();
	}
}

// What the next submit's block 0 needs of this one, behind track_kernel on the same stream -- so the kernel that reads carry and
// prior has ended before they are written, and the next submit's reads come behind these writes --: every stream's last 16 pairs,
// and prior = min(16, prior' + n) of the run that reaches the submit's last sample (prior' = 0 unless it CONTINUES), 0 without
// one.  16 lanes per stream.
__global__ __launch_bounds__(256) void track_carry_kernel(const uint32_t *__restrict__ dec, size_t dec_stride, int n_blocks, int n_streams,
							   const CaptureStage *__restrict__ stage, int stage_cap,
							   const uint2 *__restrict__ cnt, uint32_t *__restrict__ carry, uint32_t *__restrict__ prior)
{
	const int s = (int)blockIdx.x * (256 / kTrackAhead) + (int)threadIdx.x / kTrackAhead, i = threadIdx.x % kTrackAhead;
	if (s >= n_streams)
		return;
	const int M = n_blocks * kBlockDec;
	carry[(size_t)s * kTrackAhead + i] = dec[(size_t)s * dec_stride + (M - kTrackAhead + i)];
	if (i)
		return;
	const int nr = (int)cnt[s].x;
	uint32_t p = 0;
	if (nr) {
		const CaptureStage r = stage[(size_t)s * stage_cap + (nr - 1)];
		if (r.end == M) {
			p = ((r.flags & TFREC_AMD_RUN_CONTINUES) ? prior[s] : 0u) + (uint32_t)(r.end - r.start);
			p = p > (uint32_t)kTrackAhead ? (uint32_t)kTrackAhead : p;
		}
	}
	prior[s] = p;
}

hipError_t launch_burst_track(hipStream_t st, const FrontOut &o, const CaptureBufs &b, const TrackBufs &k)
{
	launch_run_records_init(st, b, k.recs, k.words);
	hipLaunchKernelGGL(track_kernel, dim3(o.n_blocks, o.n_streams), dim3(kTrackThreads), 0, st, o.dec, o.dec_stride, o.mask, o.mask_stride,
			   b.stage, b.stage_cap, b.cnt, b.base, b.max_runs, b.max_samples, k.centre, k.carry, k.prior, k.smooth, k.recs, k.words);
	hipLaunchKernelGGL(track_carry_kernel, dim3((o.n_streams + 256 / kTrackAhead - 1) / (256 / kTrackAhead)), dim3(256), 0, st, o.dec,
			   o.dec_stride, o.n_blocks, o.n_streams, b.stage, b.stage_cap, b.cnt, k.carry, k.prior);
	return hipGetLastError();
}
