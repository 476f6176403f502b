// tfrec_amd/csrc/amplitude.h -- the burst track's amplitude mode (tfrec_amd_enable_burst_track_amplitude, include/tfrec_amd.h: "Amplitude
// track"): per captured sample of every run of the recorder's table one bit, 1 where the boxcar sum of L powers
// p = |I| + |Q| lies above L times the stream's level -- an on-off keyed burst's track in the frequency track's own shape: the same
// records, bitmap, carry and readers, so the slicer, the merger and the sync work on it as they are.  One kernel, amplitude_kernel,
// in track_kernel's place between capture.h's run_records_init_kernel and track.h's track_carry_kernel, which are launched as they
// are.  Exact integers only, 32 bits throughout: p <= 2^16, a sum <= 2^20, L level < 2^20.  Included by frontend.hip (inside
// namespace tfrec) behind track.h.  tfrec_amd/track.py (amplitude_tracks) restates the result.
#pragma once

// Block blockIdx.x of stream blockIdx.y: track_kernel's geometry, run lookup, bitmap ORs and reductions (track.h); only the bit
// differs.
//   1. p of the block's 8192 pairs and of the 16 ahead of it into LDS, coalesced, in track_slot's padded layout: the 16 are the
//      row's own, or for block 0 the stream's carried ones (track_carry_kernel).  A block without a run ends before that.
//   2. Lane t owns the samples [b0 + 32 t, b0 + 32 t + 32).  With cf = the chain's first sample, submit-relative (the run's start,
//      less prior in a CONTINUES run: >= -16), p'(m) = p(m) for m >= cf and 0 for m < cf: the header's sum over the i < L with
//      k - i >= -prior is the sum of p'(m - i) over all i < L, which slides: + p'(m) - p'(m - L).  Nothing ahead of cf is used and
//      nothing ahead of slot 0 is addressed (m - L >= b0 - 16).  The bit is sum > L level; `level` is the stream's staged int32, the
//      one that carries the centre's index in frequency mode.
//   3., 4. as track_kernel's.
// The run loop is uniform over the workgroup.  No floating point, no 64-bit product.
__global__ __launch_bounds__(kTrackThreads) void amplitude_kernel(const uint32_t *__restrict__ dec, size_t dec_stride,
								   const unsigned long long *__restrict__ mask, size_t mask_stride,
								   const CaptureStage *__restrict__ stage, int stage_cap,
								   const uint2 *__restrict__ cnt, const uint4 *__restrict__ base, uint32_t max_runs,
								   unsigned long long max_samples, const int32_t *__restrict__ level,
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
	__shared__ uint32_t l_p[kTrackLds];
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
		const uint32_t w = m >= 0 ? row[m] : carry[(size_t)s * kTrackAhead + q];
		const int I = (int16_t)(w & 0xffffu), Q = (int16_t)(w >> 16);
		l_p[track_slot(q)] = (uint32_t)((I < 0 ? -I : I) + (Q < 0 ? -Q : Q));  // (<= 65536)
	}
	__syncthreads();
	const uint32_t thr = (uint32_t)L * (uint32_t)(level[s] & 0xffff);  // (< 2^20)
	const int pr = (int)prior[s];                                      // (<= 16)
	const int n0 = b0 + 32 * t;                                        // the lane's first sample
	const unsigned long long *mrow = mask + (size_t)s * mask_stride;
	auto pw = [&](int m) -> uint32_t { return l_p[track_slot(m - b0 + kTrackAhead)]; };
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
			uint32_t sum = 0;
			for (int i = 0; i < L; i++) {
				const int m = n0 + j0 - i;  // (>= b0 - 15: slot 1 or later)
				sum += m >= cf ? pw(m) : 0u;
			}
			w = (uint32_t)(sum > thr) << j0;
			for (int j = j0 + 1; j < j1; j++) {
				const int m = n0 + j;  // (> a >= cf)
				sum += pw(m) - (m - L >= cf ? pw(m - L) : 0u);
				w |= (uint32_t)(sum > thr) << j;
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

// The amplitude mode's three kernels: launch_burst_track's, with amplitude_kernel in track_kernel's place.  k.centre holds the levels.
hipError_t launch_burst_track_amplitude(hipStream_t st, const FrontOut &o, const CaptureBufs &b, const TrackBufs &k)
{
	launch_run_records_init(st, b, k.recs, k.words);
	hipLaunchKernelGGL(amplitude_kernel, dim3(o.n_blocks, o.n_streams), dim3(kTrackThreads), 0, st, o.dec, o.dec_stride, o.mask, o.mask_stride,
			   b.stage, b.stage_cap, b.cnt, b.base, b.max_runs, b.max_samples, k.centre, k.carry, k.prior, k.smooth, k.recs, k.words);
	hipLaunchKernelGGL(track_carry_kernel, dim3((o.n_streams + 256 / kTrackAhead - 1) / (256 / kTrackAhead)), dim3(256), 0, st, o.dec,
			   o.dec_stride, o.n_blocks, o.n_streams, b.stage, b.stage_cap, b.cnt, k.carry, k.prior);
	return hipGetLastError();
}
