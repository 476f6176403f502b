// tfrec_amd/csrc/centre.h -- the burst track's auto-centre mode (tfrec_amd_enable_burst_track_auto, include/tfrec_amd.h: "Auto-centre
// track", tfrec_amd_track_centre): every chain of the recorder's table is tracked about a centre measured on its own
// first K samples, in the same submit.  Three kernels of its own -- centre_head_kernel ahead of the track (the head's histogram over
// the burst meter's 64 directions, restricted to products whose two samples are both in the final trigger mask, and its resolve to
// a table index), track_centre_kernel (track_kernel's work about the ENTRY's index) and centre_carry_kernel behind
// track_carry_kernel -- between capture.h's run_records_init_kernel and track.h's track_carry_kernel, which are launched as they
// are.  Exact integers only.  Included by frontend.hip (inside namespace tfrec) behind amplitude.h.  tfrec_amd/track.py
// (head_centres, auto_tracks) restates the result.
#pragma once

static_assert(sizeof(tfrec_amd_track_centre) == 48 && offsetof(tfrec_amd_track_centre, n_counted) == 24 &&
		      offsetof(tfrec_amd_track_centre, centre_hz) == 32 && offsetof(tfrec_amd_track_centre, index) == 40,
	      "the init kernel copies a table entry's first 24 bytes and zeroes the rest");
// run_records_init_kernel's rule: the entry's first 24 bytes, everything else zero (centre_head_kernel writes the rest)
template <>
__device__ inline uint32_t run_record_word<tfrec_amd_track_centre>(const uint32_t *src, int w)
{
	return w < 6 ? src[w] : 0u;
}

constexpr int kCentreThreads = 256;   // centre_head_kernel: a workgroup per table entry, a product per lane and step
constexpr int kCentreMinCount = 64;   // the counted products a measured centre needs
constexpr unsigned kCentreGrid = 2048;  // its workgroups at the most: each walks the entries blockIdx.x, blockIdx.x + gridDim.x, ...

// r = floor((8192 hz + 384000) / 768000) mod 4096 for |hz| <= 192000: the numerator stays below 2^31
__device__ inline int centre_index(int hz)
{
	const int a = 8192 * hz + 384000;
	const int q = a / 768000 - (a % 768000 < 0 ? 1 : 0);
	return q & (kTuneN - 1);
}

// Entry e of the submit's table, e below min(n_runs, max_runs): its stream s and its staged run (submit-relative start and end) come
// from the table capture_copy_kernel wrote and the recorder's working set.
//   An entry that CONTINUES copies what the stream carried (centre_carry_kernel: the index and centre of the OPEN entry that ended
//   the submit before, index -1 where that entry had no record) or falls back.
//   Otherwise the lanes stride over the head's products k = 1 .. min(n, K) - 1 -- the pairs at start + k and start + k - 1, read from
//   the row wherever its block boundaries lie; start + k - 1 >= start >= 0 and start + k < end <= M --, test both samples' bits of the
//   final trigger mask and count the product's direction (burst_bin) in 64 LDS counters, as burst_accum_kernel does.  Wave 0 then
//   resolves: P is the counters' sum, a 64-lane ballot of hist[j] >= (P + 15) / 16 (and P >= 64) is the occupancy mask, its
//   rotation by 32 puts the bins in signed order (bit i: index i - 32), and two bit scans give lo and hi.  Lane 0 writes the
//   record's last 24 bytes.
// The entry loop and everything in it are uniform over the workgroup.  No floating point.
__global__ __launch_bounds__(kCentreThreads) void centre_head_kernel(const uint32_t *__restrict__ dec, size_t dec_stride,
									     const unsigned long long *__restrict__ mask, size_t mask_stride,
									     const CaptureStage *__restrict__ stage, int stage_cap,
									     const uint4 *__restrict__ base, const tfrec_amd_run *__restrict__ runs,
									     const CaptureHeader *__restrict__ hdr, uint32_t max_runs,
									     const int32_t *__restrict__ fallback, const int2 *__restrict__ carry, int K,
									     tfrec_amd_track_centre *__restrict__ out)
{
	const int t = threadIdx.x;
	const unsigned long long total = hdr->n_runs;
	const uint32_t ne = total < max_runs ? (uint32_t)total : max_runs;
	__shared__ uint32_t l_hist[64];
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
		if (t < 64)
			l_hist[t] = 0;
		__syncthreads();
		const int n = r.end - r.start, nh = n < K ? n : K;
		const uint32_t *row = dec + (size_t)s * dec_stride;
		const unsigned long long *mrow = mask + (size_t)s * mask_stride;
		for (int k = 1 + t; k < nh; k += kCentreThreads) {
			const int m = r.start + k;
			if (((mrow[m >> 6] >> (m & 63)) & (mrow[(m - 1) >> 6] >> ((m - 1) & 63)) & 1ull) == 0)
				continue;
			const uint32_t w = row[m], wp = row[m - 1];
			const int I = (int16_t)(w & 0xffffu), Q = (int16_t)(w >> 16);
			const int Ip = (int16_t)(wp & 0xffffu), Qp = (int16_t)(wp >> 16);
			const long long dot = (long long)I * Ip + (long long)Q * Qp, crs = (long long)Q * Ip - (long long)I * Qp;
			atomicAdd(&l_hist[burst_bin(dot, crs)], 1u);  // (both pairs are over a threshold >= 0: the product is not (0, 0))
		}
		__syncthreads();
		if (t < 64) {  // wave 0, all of it
			const uint32_t h = l_hist[t];
			uint32_t P = h;
#pragma unroll
			for (int d = 32; d >= 1; d >>= 1)
				P += __shfl_xor(P, d);
			const unsigned long long occ = __ballot(P >= (uint32_t)kCentreMinCount && h >= ((P + 15u) >> 4));
			if (t == 0) {
				const unsigned long long rot = (occ << 32) | (occ >> 32);  // bit i: the bin of signed index i - 32
				tfrec_amd_track_centre *o = out + e;
				int hz = fallback[s], dev = 0;
				if (rot) {
					const int lo = __builtin_ctzll(rot) - 32, hi = 31 - __builtin_clzll(rot);
					hz = 3000 * (lo + hi);
					dev = 3000 * (hi - lo);
				}
				o->n_counted = P;
				o->source = rot ? TFREC_AMD_CENTRE_MEASURED : TFREC_AMD_CENTRE_FALLBACK;
				o->centre_hz = hz;
				o->deviation_hz = dev;
				o->index = centre_index(hz);
			}
		}
		__syncthreads();  // (the counters are read before the next entry zeroes them)
	}
}

// track_kernel (track.h) about the ENTRY's index: its geometry, LDS layout, run lookup, sliding sum, bitmap ORs and reductions, line
// for line; only C and S are taken per run, from the run's centre record, which centre_head_kernel has written.  A sibling, not a
// variant: track_kernel is compiled as it was.
__global__ __launch_bounds__(kTrackThreads) void track_centre_kernel(const uint32_t *__restrict__ dec, size_t dec_stride,
									     const unsigned long long *__restrict__ mask, size_t mask_stride,
									     const CaptureStage *__restrict__ stage, int stage_cap,
									     const uint2 *__restrict__ cnt, const uint4 *__restrict__ base, uint32_t max_runs,
									     unsigned long long max_samples, const tfrec_amd_track_centre *__restrict__ cen,
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
	long long C = 0, S = 0;        // the run's, set in the run loop
	const int pr = (int)prior[s];  // (<= 16)
	const int n0 = b0 + 32 * t;    // the lane's first sample
	const unsigned long long *mrow = mask + (size_t)s * mask_stride;
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
		const int ri = cen[e0 + (unsigned)k].index & (kTuneN - 1);
		C = kTuneCos[ri];
		S = kTuneCos[(ri - kTuneN / 4) & (kTuneN - 1)];
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

// What the next submit's CONTINUES entries need of this one: per stream the index and the centre of the run that reaches the
// submit's last sample, or index -1 where there is none or it has no record.  A kernel of its own behind track_carry_kernel on the
// same stream: centre_head_kernel, which reads the carried values, has ended before they are written -- a CONTINUES entry and a
// later OPEN entry of one stream are different workgroups of it --, and the next submit's reads come behind these writes.  A lane
// per stream.
__global__ __launch_bounds__(256) void centre_carry_kernel(int n_blocks, int n_streams, const CaptureStage *__restrict__ stage, int stage_cap,
							    const uint2 *__restrict__ cnt, const uint4 *__restrict__ base, uint32_t max_runs,
							    const tfrec_amd_track_centre *__restrict__ cen, int2 *__restrict__ carry)
{
	const int s = (int)blockIdx.x * 256 + (int)threadIdx.x;
	if (s >= n_streams)
		return;
	const int nr = (int)cnt[s].x;
	int2 v = make_int2(-1, 0);
	if (nr) {
		const CaptureStage r = stage[(size_t)s * stage_cap + (nr - 1)];
		const unsigned long long e = (unsigned long long)base[s].x + (unsigned)(nr - 1);
		if (r.end == n_blocks * kBlockDec && e < max_runs)
			v = make_int2(cen[e].index, cen[e].centre_hz);
	}
	carry[s] = v;
}

// The auto-centre mode's kernels: both records' inits, the head, the track about the entries' indices, and the two carries.
// k.centre holds the set centres in Hz, the fallback.
hipError_t launch_burst_track_auto(hipStream_t st, const FrontOut &o, const CaptureBufs &b, const TrackBufs &k)
{
	launch_run_records_init(st, b, k.recs, k.words);
	launch_run_records_init(st, b, k.cen, (uint32_t *)nullptr);
	hipLaunchKernelGGL(centre_head_kernel, dim3(std::max(1u, std::min(b.max_runs, kCentreGrid))), dim3(kCentreThreads), 0, st, o.dec, o.dec_stride,
			   o.mask, o.mask_stride, b.stage, b.stage_cap, b.base, b.runs, b.hdr, b.max_runs, k.centre, k.ccarry, k.head, k.cen);
	hipLaunchKernelGGL(track_centre_kernel, dim3(o.n_blocks, o.n_streams), dim3(kTrackThreads), 0, st, o.dec, o.dec_stride, o.mask, o.mask_stride,
			   b.stage, b.stage_cap, b.cnt, b.base, b.max_runs, b.max_samples, k.cen, k.carry, k.prior, k.smooth, k.recs, k.words);
	hipLaunchKernelGGL(track_carry_kernel, dim3((o.n_streams + 256 / kTrackAhead - 1) / (256 / kTrackAhead)), dim3(256), 0, st, o.dec,
			   o.dec_stride, o.n_blocks, o.n_streams, b.stage, b.stage_cap, b.cnt, k.carry, k.prior);
	hipLaunchKernelGGL(centre_carry_kernel, dim3((o.n_streams + 255) / 256), dim3(256), 0, st, o.n_blocks, o.n_streams, b.stage, b.stage_cap,
			   b.cnt, b.base, b.max_runs, k.cen, k.ccarry);
	return hipGetLastError();
}
