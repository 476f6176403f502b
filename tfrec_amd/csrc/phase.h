// tfrec_amd/csrc/phase.h -- the burst track's phase mode (tfrec_amd_enable_burst_track_phase, include/tfrec_amd.h: "Phase track";
// DESIGN.md 6x), for phase-keyed bursts: every chain of the recorder's table is read by a differential phase detector at a lag of m
// samples about the carrier measured on its own first K samples, in the same submit.  Three kernels of its own --
// carrier_head_kernel ahead of the track (the sums A, B of the head's counted products and the zero of the cross term over the
// 4096 table directions), phase_kernel (track_kernel's geometry about u[k] = Re(z[k] conj(z[k - m])) turned back by r m) and
// phase_carry_kernel (the 80 carried pairs and prior) -- between capture.h's run_records_init_kernel and centre.h's
// centre_carry_kernel, which are launched as they are.  Exact integers only.  Included by frontend.hip (inside namespace tfrec)
// behind centre.h.  tfrec_amd/track.py (head_carriers, phase_tracks) restates the result.
#pragma once

constexpr int kPhaseLagMax = 64;                         // the largest m
constexpr int kPhaseAhead = kPhaseLagMax + kTrackAhead;  // the pairs kept ahead of a block: sample k - i - m, i < L <= 16, m <= 64
constexpr int kPhaseSlots = kBlockDec + kPhaseAhead;
constexpr int kPhaseLds = kPhaseSlots + (kPhaseSlots >> 5) + 1;  // (track_slot's padding)
constexpr int kCarrierPerLane = kTuneN / kCentreThreads;         // carrier_head_kernel: the candidates a lane tries
static_assert(kCarrierPerLane * kCentreThreads == kTuneN && kCentreThreads == 256, "the 4096 candidates are spread over four waves");

// (|cross|, r) of lane-local candidates, reduced to the smallest pair -- the smaller r on equal |cross| -- over a wave
__device__ inline void carrier_wave_min(long long &x, int &r)
{
#pragma unroll
	for (int d = 32; d >= 1; d >>= 1) {
		const long long ox = __shfl_xor(x, d);
		const int orr = __shfl_xor(r, d);
		if (ox < x || (ox == x && orr < r)) {
			x = ox;
			r = orr;
		}
	}
}

// Entry e of the submit's table, as centre_head_kernel walks it: a CONTINUES entry copies what the stream carried or falls back.
// Otherwise the lanes stride over the head's products k = 1 .. min(n, K) - 1 (start + k - 1 >= 0 and start + k < end <= M), test
// both samples' bits of the final trigger mask, and add dot and crs (each below 2^31 in size: at most 4095 of them, |A|, |B| <
// 2^43) and 1 to their own A, B and P, which are reduced over each wave and then through LDS.  With P >= 64 and (A, B) != (0, 0)
// lane t tries the candidates r = 16 t .. 16 t + 15: score = A C[r] + B S[r] and cross = B C[r] - A S[r] (below 2^59), keeps the
// smallest (|cross|, r) among those with score > 0 -- (2^63 - 1, 4096) stands for none --, and the pairs are reduced the same
// way; at least one candidate has a positive score, the one nearest the direction of (A, B).  Lane 0 writes the record's last 24
// bytes.  The entry loop and everything around the barriers are uniform over the workgroup.  No floating point.
__global__ __launch_bounds__(kCentreThreads) void carrier_head_kernel(const uint32_t *__restrict__ dec, size_t dec_stride,
								      const unsigned long long *__restrict__ mask, size_t mask_stride,
								      const CaptureStage *__restrict__ stage, int stage_cap,
								      const uint4 *__restrict__ base, const tfrec_amd_run *__restrict__ runs,
								      const CaptureHeader *__restrict__ hdr, uint32_t max_runs,
								      const int32_t *__restrict__ fallback, const int2 *__restrict__ carry, int K,
								      tfrec_amd_track_centre *__restrict__ out)
{
	const int t = threadIdx.x, wv = t >> 6;
	const unsigned long long total = hdr->n_runs;
	const uint32_t ne = total < max_runs ? (uint32_t)total : max_runs;
	__shared__ long long l_a[kCentreThreads / 64], l_b[kCentreThreads / 64], l_x[kCentreThreads / 64];
	__shared__ uint32_t l_p[kCentreThreads / 64];
	__shared__ int l_r[kCentreThreads / 64];
	for (uint32_t e = blockIdx.x; e < ne; e += gridDim.x) {
		const int s = (int)runs[e].stream;
		const CaptureStage r = stage[(size_t)s * stage_cap + (e - base[s].x)];  // (the stream's entries are base[s].x .. + cnt[s].x - 1)
		if (r.flags & TFREC_AMD_RUN_CONTINUES) {
			if (t == 0) {
				const int2 c = carry[s];
				tfrec_amd_track_centre *o = out + e;
				o->source = c.x >= 0 ? TFREC_AMD_CENTRE_INHERITED : TFREC_AMD_CENTRE_FALLBACK;
				o->centre_hz = c.x >= 0 ? c.y : fallback[s];
				o->index = c.x >= 0 ? c.x : centre_index(fallback[s]);
			}
			continue;
		}
		const int n = r.end - r.start, nh = n < K ? n : K;
		const uint32_t *row = dec + (size_t)s * dec_stride;
		const unsigned long long *mrow = mask + (size_t)s * mask_stride;
		long long A = 0, B = 0;
		uint32_t P = 0;
		for (int k = 1 + t; k < nh; k += kCentreThreads) {
			const int m = r.start + k;
			if (((mrow[m >> 6] >> (m & 63)) & (mrow[(m - 1) >> 6] >> ((m - 1) & 63)) & 1ull) == 0)
				continue;
			const uint32_t w = row[m], wp = row[m - 1];
			const int I = (int16_t)(w & 0xffffu), Q = (int16_t)(w >> 16);
			const int Ip = (int16_t)(wp & 0xffffu), Qp = (int16_t)(wp >> 16);
			A += (long long)(I * Ip) + (long long)(Q * Qp);
			B += (long long)(Q * Ip) - (long long)(I * Qp);
			P++;
		}
#pragma unroll
		for (int d = 32; d >= 1; d >>= 1) {
			A += __shfl_xor(A, d);
			B += __shfl_xor(B, d);
			P += __shfl_xor(P, d);
		}
		if ((t & 63) == 0) {
			l_a[wv] = A;
			l_b[wv] = B;
			l_p[wv] = P;
		}
		__syncthreads();
		A = l_a[0] + l_a[1] + l_a[2] + l_a[3];
		B = l_b[0] + l_b[1] + l_b[2] + l_b[3];
		P = l_p[0] + l_p[1] + l_p[2] + l_p[3];
		const bool measured = P >= (uint32_t)kCentreMinCount && (A != 0 || B != 0);  // (uniform)
		long long bx = 0x7fffffffffffffffll;
		int br = kTuneN;
		if (measured) {
#pragma unroll 4
			for (int j = 0; j < kCarrierPerLane; j++) {
				const int c = kCarrierPerLane * t + j;
				const long long C = kTuneCos[c], S = kTuneCos[(c - kTuneN / 4) & (kTuneN - 1)];
				const long long score = A * C + B * S, cross = B * C - A * S;
				const long long ax = cross < 0 ? -cross : cross;
				if (score > 0 && ax < bx) {  // (the candidates ascend: the first of equal ones stays)
					bx = ax;
					br = c;
				}
			}
			carrier_wave_min(bx, br);
			if ((t & 63) == 0) {
				l_x[wv] = bx;
				l_r[wv] = br;
			}
		}
		__syncthreads();  // (l_a, l_b, l_p are read before the next entry writes them; l_x, l_r are written)
		if (t == 0) {
			tfrec_amd_track_centre *o = out + e;
			int hz = fallback[s], idx;
			if (measured) {
				for (int i = 1; i < kCentreThreads / 64; i++)
					if (l_x[i] < bx || (l_x[i] == bx && l_r[i] < br)) {
						bx = l_x[i];
						br = l_r[i];
					}
				idx = br & (kTuneN - 1);
				const int rs = idx < kTuneN / 2 ? idx : idx - kTuneN;
				hz = (375 * rs) >> 2;  // floor(375 rs / 4)
			} else {
				idx = centre_index(hz);
			}
			o->n_counted = P;
			o->source = measured ? TFREC_AMD_CENTRE_MEASURED : TFREC_AMD_CENTRE_FALLBACK;
			o->centre_hz = hz;
			o->deviation_hz = 0;
			o->index = idx;
		}
		__syncthreads();  // (lane 0 has read l_x, l_r before the next entry's waves write them)
	}
}

// track_kernel's geometry, run lookup, sliding sum, bitmap ORs and reductions (track.h) about the differential product at lag m:
//   1. The block's 8192 pairs and the 80 ahead of it into LDS, coalesced, with track_slot's padding: the 80 are the row's own, or
//      for block 0 the stream's carried ones (phase_carry_kernel).  A block without a run ends before that.
//   2. Lane t owns the samples [b0 + 32 t, b0 + 32 t + 32).  With cf = the chain's first sample, submit-relative (the run's start,
//      less prior in a CONTINUES run, whose start is 0: cf >= -80), u'(k) = dm C[rm] + cm S[rm] of the pairs at k and k - m for
//      k - cf >= m and 0 otherwise: the track's sum is that of u'(k - i) over i < L, which slides: + u'(k) - u'(k - L).  A pair is
//      read only at k - m >= cf, and the lowest k asked for is the run's first sample in the block less 15 (>= b0 - 15), so
//      no slot below b0 - 79 is addressed and no pair ahead of the chain is used.  |u'| < 2^47, the sum < 2^51.
//   3. and 4. as track_kernel's.  C[rm], S[rm] are taken per run from the run's centre record, which carrier_head_kernel has written.
// The run loop is uniform over the workgroup.  No floating point.
__global__ __launch_bounds__(kTrackThreads) void phase_kernel(const uint32_t *__restrict__ dec, size_t dec_stride,
							       const unsigned long long *__restrict__ mask, size_t mask_stride,
							       const CaptureStage *__restrict__ stage, int stage_cap,
							       const uint2 *__restrict__ cnt, const uint4 *__restrict__ base, uint32_t max_runs,
							       unsigned long long max_samples, const tfrec_amd_track_centre *__restrict__ cen,
							       const uint32_t *__restrict__ carry, const uint32_t *__restrict__ prior, int L, int lag,
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
	__shared__ uint32_t l_z[kPhaseLds];
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
	for (int q = t; q < kPhaseSlots; q += kTrackThreads) {
		const int m = b0 - kPhaseAhead + q;  // (m < 0: block 0's first 80 slots)
		l_z[track_slot(q)] = m >= 0 ? row[m] : carry[(size_t)s * kPhaseAhead + q];
	}
	__syncthreads();
	long long C = 0, S = 0;        // the run's, set in the run loop
	int cf = 0;                    // ... and its chain's first sample
	const int pr = (int)prior[s];  // (<= 80)
	const int n0 = b0 + 32 * t;    // the lane's first sample
	const unsigned long long *mrow = mask + (size_t)s * mask_stride;
	auto up = [&](int k) -> long long {
		if (k - cf < lag)
			return 0;
		const int q = k - b0 + kPhaseAhead;  // (q - lag >= cf - b0 + 80 >= 0, and > 0 by step 2's bound)
		const uint32_t w = l_z[track_slot(q)], wp = l_z[track_slot(q - lag)];
		const int I = (int16_t)(w & 0xffffu), Q = (int16_t)(w >> 16);
		const int Ip = (int16_t)(wp & 0xffffu), Qp = (int16_t)(wp >> 16);
		const long long dm = (long long)(I * Ip) + (long long)(Q * Qp), cm = (long long)(Q * Ip) - (long long)(I * Qp);
		return dm * C + cm * S;
	};
	for (int k = lo; k < hi; k++) {
		if (e0 + (unsigned)k >= max_runs)
			break;  // (and every later run of the stream: no record)
		const CaptureStage r = srow[k];
		const int rm = ((cen[e0 + (unsigned)k].index & (kTuneN - 1)) * lag) & (kTuneN - 1);
		C = kTuneCos[rm];
		S = kTuneCos[(rm - kTuneN / 4) & (kTuneN - 1)];
		cf = r.start - ((r.flags & TFREC_AMD_RUN_CONTINUES) ? pr : 0);
		const int a = r.start > b0 ? r.start : b0, e = r.end < b1 ? r.end : b1;  // b0 <= a < e <= b1 <= M
		const int j0 = a > n0 ? a - n0 : 0, j1 = e - n0 < 32 ? e - n0 : 32;  // the lane's samples of the run: [n0 + j0, n0 + j1)
		uint32_t w = 0;
		int last = -1;
		if (j0 < j1) {
			long long sum = 0;
			for (int i = 0; i < L; i++)
				sum += up(n0 + j0 - i);
			w = (uint32_t)(sum > 0) << j0;
			for (int j = j0 + 1; j < j1; j++) {
				const int m = n0 + j;
				sum += up(m) - up(m - L);
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

// track_carry_kernel's work with 80 pairs: every stream's last 80 pairs, and prior = min(80, prior' + n) of the run that reaches
// the submit's last sample (prior' = 0 unless it CONTINUES), 0 without one.  Behind phase_kernel on the same stream.  80 lanes per
// stream, 3 streams per workgroup of 240.
constexpr int kPhaseCarryStreams = 3;
__global__ __launch_bounds__(kPhaseCarryStreams * kPhaseAhead) void phase_carry_kernel(const uint32_t *__restrict__ dec, size_t dec_stride, int n_blocks,
										       int n_streams, const CaptureStage *__restrict__ stage,
										       int stage_cap, const uint2 *__restrict__ cnt,
										       uint32_t *__restrict__ carry, uint32_t *__restrict__ prior)
{
	const int s = (int)blockIdx.x * kPhaseCarryStreams + (int)threadIdx.x / kPhaseAhead, i = threadIdx.x % kPhaseAhead;
	if (s >= n_streams)
		return;
	const int M = n_blocks * kBlockDec;
	carry[(size_t)s * kPhaseAhead + i] = dec[(size_t)s * dec_stride + (M - kPhaseAhead + i)];
	if (i)
		return;
	const int nr = (int)cnt[s].x;
	uint32_t p = 0;
	if (nr) {
		const CaptureStage r = stage[(size_t)s * stage_cap + (nr - 1)];
		if (r.end == M) {
			p = ((r.flags & TFREC_AMD_RUN_CONTINUES) ? prior[s] : 0u) + (uint32_t)(r.end - r.start);
			p = p > (uint32_t)kPhaseAhead ? (uint32_t)kPhaseAhead : p;
		}
	}
	prior[s] = p;
}

// The phase mode's kernels: both records' inits, the head's carrier, the track about the entries' indices, and the two carries.
// k.centre holds the set centres in Hz, the fallback; k.carry holds 80 pairs per stream.
hipError_t launch_burst_track_phase(hipStream_t st, const FrontOut &o, const CaptureBufs &b, const TrackBufs &k)
{
	launch_run_records_init(st, b, k.recs, k.words);
	launch_run_records_init(st, b, k.cen, (uint32_t *)nullptr);
	hipLaunchKernelGGL(carrier_head_kernel, dim3(std::max(1u, std::min(b.max_runs, kCentreGrid))), dim3(kCentreThreads), 0, st, o.dec, o.dec_stride,
			   o.mask, o.mask_stride, b.stage, b.stage_cap, b.base, b.runs, b.hdr, b.max_runs, k.centre, k.ccarry, k.head, k.cen);
	hipLaunchKernelGGL(phase_kernel, dim3(o.n_blocks, o.n_streams), dim3(kTrackThreads), 0, st, o.dec, o.dec_stride, o.mask, o.mask_stride,
			   b.stage, b.stage_cap, b.cnt, b.base, b.max_runs, b.max_samples, k.cen, k.carry, k.prior, k.smooth, k.lag, k.recs, k.words);
	hipLaunchKernelGGL(phase_carry_kernel, dim3((o.n_streams + kPhaseCarryStreams - 1) / kPhaseCarryStreams), dim3(kPhaseCarryStreams * kPhaseAhead), 0,
			   st, o.dec, o.dec_stride, o.n_blocks, o.n_streams, b.stage, b.stage_cap, b.cnt, k.carry, k.prior);
	hipLaunchKernelGGL(centre_carry_kernel, dim3((o.n_streams + 255) / 256), dim3(256), 0, st, o.n_blocks, o.n_streams, b.stage, b.stage_cap,
			   b.cnt, b.base, b.max_runs, k.cen, k.ccarry);
	return hipGetLastError();
}
