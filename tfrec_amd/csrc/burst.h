// tfrec_amd/csrc/burst.h -- the burst meter (tfrec_amd_enable_burst_meter, include/tfrec_amd.h: tfrec_amd_burst): per
// run of the recorder's table a histogram over 64 directions of the products z[k] conj(z[k-1]) of consecutive decimated samples,
// their sums, the run's energy and its peak.  Two kernels (capture.h's run_records_init_kernel and burst_accum_kernel) behind
// capture_copy_kernel on the recorder's low-priority lane; they read the recorder's table and working set, the decimated samples
// and prevdec, and nothing a demodulator owns.  Exact integers only: every quantity is an integer sum or maximum, so the order of
// the atomics that combine the pieces cannot matter.  Included by frontend.hip (inside namespace tfrec) behind capture.h.
// tfrec_amd/burst.py restates the result.
#pragma once

static_assert(sizeof(tfrec_amd_burst) == 320 && offsetof(tfrec_amd_burst, pwr_max) == 24 && offsetof(tfrec_amd_burst, hist) == 56 &&
		      offsetof(tfrec_amd_run, pool_offset) == 24,
	      "the init kernel copies a table entry's first 24 bytes and zeroes the rest");
// run_records_init_kernel's rule: the copied fields from the entry capture_copy_kernel wrote (its first 24 bytes are the record's),
// everything else zero
template <>
__device__ inline uint32_t run_record_word<tfrec_amd_burst>(const uint32_t *src, int w)
{
	return w < 6 ? src[w] : 0u;
}

constexpr int kBurstThreads = 256;  // burst_accum_kernel: a workgroup per (stream, block), a sample per lane and step

// The bin of a product: the j in 0..63 that maximises dot C[64 j] + crs S[64 j], the lowest on a tie.  Evaluated without the 64
// scores.  The table is exact under a quarter turn -- C[64 (j + 16)] = -S[64 j], S[64 (j + 16)] = C[64 j], from C[-k] = C[k] and
// C[2048 - k] = -C[k] --, so q quarter turns bring the product to x > 0, y >= 0 and score(16 q + j) of the product is score(j) of
// (x, y).  There direction k + 1 scores higher than k iff y (S[k+1] - S[k]) > x (C[k] - C[k+1]), both differences positive for k =
// 0..15, and their ratios increase strictly with k (asserted below): the comparisons are true up to the argmax and false from it
// on, the argmax is their count, and a tie (the one boundary the product lies on) keeps the lower direction.  The directions
// outside the quarter lose: 16 + m to 16 - m by 2 x S[m] > 0, -m to m by 2 y S[m] >= 0 (y == 0: direction 0 wins outright), the
// rest score <= 0.  Only a tie between 63 and 0 must go to the higher count: the last boundary of the last quarter.
// S[64 (k + 1)] - S[64 k], k = 0..15; C[64 k] - C[64 (k + 1)] is entry 15 - k (C[1024 - k] = S[k])
constexpr unsigned kBurstDS[16] = { 3212, 3181, 3119, 3027, 2907, 2758, 2583, 2383, 2159, 1916, 1653, 1375, 1083, 781, 472, 158 };
constexpr int16_t kBurstCos[1 << TFREC_TUNE_BITS] = { TFREC_TUNE_COS_TABLE };
constexpr bool burst_table_ok()
{
	for (int k = 0; k < 16; k++) {
		const int s0 = kBurstCos[(64 * k - 1024) & 4095], s1 = kBurstCos[(64 * (k + 1) - 1024) & 4095];
		if (s1 - s0 != (int)kBurstDS[k] || kBurstCos[64 * k] - kBurstCos[64 * (k + 1)] != (int)kBurstDS[15 - k])
			return false;
		// DC[k] / DS[k] < DC[k+1] / DS[k+1]
		if (k < 15 && (long long)kBurstDS[15 - k] * kBurstDS[k + 1] >= (long long)kBurstDS[14 - k] * kBurstDS[k])
			return false;
	}
	for (int k = 0; k < 4096; k++)
		if (kBurstCos[(4096 - k) & 4095] != kBurstCos[k] || kBurstCos[(2048 - k) & 4095] != -kBurstCos[k])
			return false;
	return true;
}
static_assert(burst_table_ok(), "burst_bin's boundaries are the tune table's, and the table has the symmetries it relies on");

// (dot, crs) != (0, 0), |dot|, |crs| <= 2^31
__device__ inline int burst_bin(long long dot, long long crs)
{
	int q;
	long long xs, ys;
	if (dot > 0 && crs >= 0) {
		q = 0, xs = dot, ys = crs;
	} else if (dot <= 0 && crs > 0) {
		q = 1, xs = crs, ys = -dot;
	} else if (dot < 0 && crs <= 0) {
		q = 2, xs = -dot, ys = -crs;
	} else {
		q = 3, xs = -crs, ys = dot;
	}
	const unsigned x = (unsigned)xs, y = (unsigned)ys;  // (<= 2^31; the products below stay under 2^43)
	int n = 0;
#pragma unroll
	for (int k = 0; k < 16; k++)
		n += (unsigned long long)y * kBurstDS[k] > (unsigned long long)x * kBurstDS[15 - k];
	if (q == 3 && n == 15 && (unsigned long long)y * kBurstDS[15] == (unsigned long long)x * kBurstDS[0])
		n = 16;
	return (16 * q + n) & 63;
}

// Block blockIdx.x of stream blockIdx.y: the part inside the block of every run of the stream that meets it -> added to the run's
// record.  The runs that meet the block are the index range [lo, hi) of the stream's staged runs, found by capture_run_range; a
// run's part is walked in steps of kBurstThreads samples, a sample per lane, so a short run costs one step and a stream that
// never leaves its window is spread over its blocks.  The product at sample n pairs it with sample n - 1: inside
// the row, or prevdec[s] at the submit's first sample; it is left out at a run's first sample unless the run CONTINUES (its
// start is then the submit's first sample).  Products are formed in 64 bits: |dot|, |crs| <= 2^31 for any int16 pairs.
// Per run and block: the histogram in LDS, sums and peak reduced over each wave and then in LDS; one round of integer atomics to
// the record -- the non-zero bins, the three 64-bit sums, the count and the peak.  The loops are uniform over the workgroup.
__global__ __launch_bounds__(kBurstThreads) void burst_accum_kernel(const uint32_t *__restrict__ dec, size_t dec_stride, int n_blocks,
								     const uint32_t *__restrict__ prevdec,
								     const CaptureStage *__restrict__ stage, int stage_cap,
								     const uint2 *__restrict__ cnt, const uint4 *__restrict__ base, uint32_t max_runs,
								     tfrec_amd_burst *__restrict__ out)
{
	const int b = blockIdx.x, s = blockIdx.y, t = threadIdx.x;
	const int nr = (int)cnt[s].x;  // (<= stage_cap)
	if (nr == 0)
		return;
	const CaptureStage *srow = stage + (size_t)s * stage_cap;
	const unsigned long long e0 = base[s].x;  // the stream's first table entry
	__shared__ int l_pmax;
	__shared__ uint32_t l_np, l_hist[64];
	__shared__ unsigned long long l_sum[3];
	if (t == 0)
		l_pmax = 0;
	if (t == 1)
		l_np = 0;
	if (t >= 2 && t < 5)
		l_sum[t - 2] = 0;
	if (t >= 64 && t < 128)
		l_hist[t - 64] = 0;
	const int b0 = b * kBlockDec, b1 = b0 + kBlockDec;
	int lo, hi;
	capture_run_range(srow, nr, b0, b1, t, kBurstThreads, lo, hi);
	const uint32_t *row = dec + (size_t)s * dec_stride;
	for (int k = lo; k < hi; k++) {
		if (e0 + (unsigned)k >= max_runs)
			break;  // (and every later run of the stream: no record)
		const CaptureStage r = srow[k];
		const bool cont = (r.flags & TFREC_AMD_RUN_CONTINUES) != 0;
		const int a = r.start > b0 ? r.start : b0, e = r.end < b1 ? r.end : b1;  // b0 <= a < e <= b1 <= M
		int pmax = 0;
		long long np = 0, sd = 0, sc = 0, en = 0;
		for (int n = a + t; n < e; n += kBurstThreads) {
			const uint32_t w = row[n];
			const int I = (int16_t)(w & 0xffffu), Q = (int16_t)(w >> 16);
			const int p = abs(I) + abs(Q);
			pmax = p > pmax ? p : pmax;
			en += (long long)((unsigned)(I * I) + (unsigned)(Q * Q));  // (<= 2^31)
			if (n > r.start || cont) {
				const uint32_t wp = n > 0 ? row[n - 1] : prevdec[s];
				const int Ip = (int16_t)(wp & 0xffffu), Qp = (int16_t)(wp >> 16);
				const long long dot = (long long)I * Ip + (long long)Q * Qp, crs = (long long)Q * Ip - (long long)I * Qp;
				if (dot | crs) {
					atomicAdd(&l_hist[burst_bin(dot, crs)], 1u);
					np++;
					sd += dot;
					sc += crs;
				}
			}
		}
#pragma unroll
		for (int d = 32; d >= 1; d >>= 1) {
			const int o = __shfl_xor(pmax, d);
			pmax = o > pmax ? o : pmax;
		}
		np = burst_wave_sum(np);
		sd = burst_wave_sum(sd);
		sc = burst_wave_sum(sc);
		en = burst_wave_sum(en);
		if ((t & 63) == 0) {
			atomicMax(&l_pmax, pmax);
			atomicAdd(&l_np, (uint32_t)np);
			atomicAdd(&l_sum[0], (unsigned long long)sd);
			atomicAdd(&l_sum[1], (unsigned long long)sc);
			atomicAdd(&l_sum[2], (unsigned long long)en);
		}
		__syncthreads();
		tfrec_amd_burst *o = out + (e0 + (unsigned)k);
		if (t < 64) {
			const uint32_t h = l_hist[t];
			if (h) {
				atomicAdd(&o->hist[t], h);
				l_hist[t] = 0;
			}
		} else if (t == 64) {
			atomicMax(&o->pwr_max, l_pmax);
			l_pmax = 0;
		} else if (t == 65) {
			if (l_np)
				atomicAdd(&o->n_products, l_np);
			l_np = 0;
		} else if (t >= 66 && t < 69) {  // sum_dot, sum_crs, energy: three consecutive 64-bit fields
			unsigned long long *f = reinterpret_cast<unsigned long long *>(&o->sum_dot) + (t - 66);
			if (l_sum[t - 66])
				atomicAdd(f, l_sum[t - 66]);
			l_sum[t - 66] = 0;
		}
		__syncthreads();
	}
}

hipError_t launch_burst_meter(hipStream_t st, const FrontOut &o, const CaptureBufs &b, tfrec_amd_burst *out)
{
	launch_run_records_init(st, b, out, nullptr);
	hipLaunchKernelGGL(burst_accum_kernel, dim3(o.n_blocks, o.n_streams), dim3(kBurstThreads), 0, st, o.dec, o.dec_stride, o.n_blocks,
			   o.prevdec, b.stage, b.stage_cap, b.cnt, b.base, b.max_runs, out);
	return hipGetLastError();
}
