// tfrec_amd/csrc/clock.h -- the burst clock (tfrec_amd_enable_burst_clock, include/tfrec_amd.h: tfrec_amd_clock): per
// run of the recorder's table the power spectrum, 128 bins of 375 Hz, of the second-order product of the decimated samples, summed
// over the 1024-sample segments that lie wholly inside the run: it peaks at the symbol rate.  Two kernels (capture.h's
// run_records_init_kernel and clock_accum_kernel) behind the envelope's on the recorder's low-priority lane; they read the
// recorder's table and working set and the decimated samples, and nothing a demodulator owns -- not even prevdec: a segment reads
// its own 1024 pairs only.  Exact integers only: every combined quantity is an integer sum, so the order of the atomics that
// combine the blocks cannot matter.  Included by frontend.hip (inside namespace tfrec) behind envelope.h.  tfrec_amd/clock.py
// restates the result.
#pragma once

static_assert(sizeof(tfrec_amd_clock) == 1056 && offsetof(tfrec_amd_clock, n_segments) == 24 && offsetof(tfrec_amd_clock, spec) == 32 &&
		      offsetof(tfrec_amd_run, pool_offset) == 24,
	      "the init kernel copies a table entry's first 24 bytes and zeroes the rest");
// run_records_init_kernel's rule: the copied fields from the entry capture_copy_kernel wrote (its first 24 bytes are the record's),
// everything else zero
template <>
__device__ inline uint32_t run_record_word<tfrec_amd_clock>(const uint32_t *src, int w)
{
	return w < 6 ? src[w] : 0u;
}

constexpr int kClockThreads = 256;  // clock_accum_kernel: a workgroup per (stream, block); two lanes per bin
constexpr int kClockSeg = 1024;  // samples per segment
constexpr int kClockBins = 128;  // bins j = kClockBin0 .. kClockBin0 + 127
constexpr int kClockBin0 = 4;
static_assert(kBlockDec % kClockSeg == 0 && kClockSeg == 4 * kClockThreads && kClockThreads == 2 * kClockBins && kTuneN == 4096,
	      "a block is 8 whole segments, a lane forms 4 products, and bin j steps 4 j entries of the 4096-entry table per sample");

// Block blockIdx.x of stream blockIdx.y: for every run of the stream that meets the block (capture_run_range's [lo, hi) of the
// staged runs), each of the block's 8 segments that lies wholly inside the run -> its spectrum, summed over the segments in
// registers (lane t < 128 owns bin 4 + t) and added to the run's record in one round of 64-bit atomics.  Per segment:
//   1. the 1024 pairs into LDS, 4 per lane (m' = t, t + 256, ...);
//   2. dot, crs of m' >= 1 in 64 bits (|.| <= 2^31), their largest magnitude over the wave by shuffles and over the workgroup in LDS;
//      mx == 0: silent, next segment;  else sh = max(0, bitlength(mx) - 15) and (d, c) = (dot, crs) >> sh as int16 halves into LDS;
//   3. g16 = min((d d' + c c') >> 16, 32767) of m' >= 2 as int16 into LDS, 0 for m' < 2 (the sum in 64 bits: it reaches 2^31);
//   4. the DFT: lane t sums bin j = 4 + (t & 127) over the samples [512 h, 512 h + 512), h = t >> 7 -- a wave lies in one half, so
//      the g16 reads are broadcasts --, the table index stepping j from (512 j h) mod 1024 in a packed (C, S) table in LDS as the
//      mixer keeps one, thinned to the 1024 entries that (4 j m') mod 4096 reaches.  Two products fit int32 (|g16| <= 2^15, |C| <
//      2^15: each < 2^30): a pair of samples is summed in 32 bits, the pairs in 64;
//   5. the halves meet in LDS; lane t < 128: P = (X_re >> 16)^2 + (X_im >> 16)^2 (< 2^49), added to its register.
// Every loop and branch is uniform over the workgroup.  No floating point.
__global__ __launch_bounds__(kClockThreads) void clock_accum_kernel(const uint32_t *__restrict__ dec, size_t dec_stride, int n_blocks,
								     const CaptureStage *__restrict__ stage, int stage_cap,
								     const uint2 *__restrict__ cnt, const uint4 *__restrict__ base, uint32_t max_runs,
								     tfrec_amd_clock *__restrict__ out)
{
	const int b = blockIdx.x, s = blockIdx.y, t = threadIdx.x;
	const int nr = (int)cnt[s].x;  // (<= stage_cap)
	if (nr == 0)
		return;
	const CaptureStage *srow = stage + (size_t)s * stage_cap;
	const unsigned long long e0 = base[s].x;  // the stream's first table entry
	__shared__ uint32_t l_mx;
	__shared__ uint32_t l_tab[kClockSeg];   // (C[4 k], S[4 k]) as int16 halves: the entries (4 j m') mod 4096 can reach
	__shared__ uint32_t l_z[kClockSeg];     // the segment's pairs
	__shared__ uint32_t l_dc[kClockSeg];    // (d, c) as int16 halves
	__shared__ __attribute__((aligned(4))) int16_t l_g[kClockSeg];
	__shared__ long long l_part[2][kClockBins][2];
	const int b0 = b * kBlockDec, b1 = b0 + kBlockDec;
	int lo, hi;
	capture_run_range(srow, nr, b0, b1, t, kClockThreads, lo, hi);
	if (lo >= hi)
		return;
	for (int i = t; i < kClockSeg; i += kClockThreads)
		l_tab[i] = (uint32_t)(uint16_t)kTuneCos[4 * i] | ((uint32_t)(uint16_t)kTuneCos[(4 * i - kTuneN / 4) & (kTuneN - 1)] << 16);
	const uint32_t *row = dec + (size_t)s * dec_stride;
	const int bin = t & (kClockBins - 1), half = t >> 7;
	const uint32_t step = (uint32_t)(kClockBin0 + bin);  // in entries of l_tab
	for (int k = lo; k < hi; k++) {
		if (e0 + (unsigned)k >= max_runs)
			break;  // (and every later run of the stream: no record)
		const CaptureStage r = srow[k];
		uint32_t nseg = 0, nsil = 0;
		unsigned long long pacc = 0;  // t < 128: bin 4 + t over this run's segments of the block
		for (int q = 0; q < kBlockDec / kClockSeg; q++) {
			const int s0 = b0 + q * kClockSeg;  // b0 <= s0, s0 + 1024 <= b1 <= M
			if (s0 < r.start || s0 + kClockSeg > r.end)
				continue;
			__syncthreads();  // (the segment before, and the table, are done with)
			if (t == 0)
				l_mx = 0;
#pragma unroll
			for (int i = 0; i < 4; i++)
				l_z[t + i * kClockThreads] = row[s0 + t + i * kClockThreads];
			__syncthreads();
			long long dot[4], crs[4];
			uint32_t mx = 0;
#pragma unroll
			for (int i = 0; i < 4; i++) {
				const int m = t + i * kClockThreads;
				dot[i] = crs[i] = 0;
				if (m >= 1) {
					const uint32_t w = l_z[m], wp = l_z[m - 1];
					const int I = (int16_t)(w & 0xffffu), Q = (int16_t)(w >> 16);
					const int Ip = (int16_t)(wp & 0xffffu), Qp = (int16_t)(wp >> 16);
					dot[i] = (long long)I * Ip + (long long)Q * Qp;
					crs[i] = (long long)Q * Ip - (long long)I * Qp;
					const uint32_t ad = (uint32_t)(dot[i] < 0 ? -dot[i] : dot[i]), ac = (uint32_t)(crs[i] < 0 ? -crs[i] : crs[i]);
					mx = ad > mx ? ad : mx;
					mx = ac > mx ? ac : mx;
				}
			}
#pragma unroll
			for (int d = 32; d >= 1; d >>= 1) {
				const uint32_t o = (uint32_t)__shfl_xor((int)mx, d);
				mx = o > mx ? o : mx;
			}
			if ((t & 63) == 0 && mx)
				atomicMax(&l_mx, mx);
			__syncthreads();
			mx = l_mx;
			if (mx == 0) {
				nsil++;
				continue;
			}
			nseg++;
			const int bits = 32 - __clz((int)mx);
			const int sh = bits > 15 ? bits - 15 : 0;
#pragma unroll
			for (int i = 0; i < 4; i++)  // (m' = 0: (0, 0), never read)
				l_dc[t + i * kClockThreads] = (uint32_t)(uint16_t)(int16_t)(dot[i] >> sh) | ((uint32_t)(uint16_t)(int16_t)(crs[i] >> sh) << 16);
			__syncthreads();
#pragma unroll
			for (int i = 0; i < 4; i++) {
				const int m = t + i * kClockThreads;
				int g16 = 0;
				if (m >= 2) {
					const uint32_t w = l_dc[m], wp = l_dc[m - 1];
					const long long g = (long long)((int16_t)(w & 0xffffu) * (int16_t)(wp & 0xffffu)) +
							    (long long)((int16_t)(w >> 16) * (int16_t)(wp >> 16));  // (each product <= 2^30)
					g16 = (int)(g >> 16);
					g16 = g16 > 32767 ? 32767 : g16;
				}
				l_g[m] = (int16_t)g16;
			}
			__syncthreads();
			long long xr = 0, xi = 0;
			uint32_t idx = (step * (uint32_t)(half * (kClockSeg / 2))) & (kClockSeg - 1);
			const uint32_t *g2 = reinterpret_cast<const uint32_t *>(l_g) + half * (kClockSeg / 4);
#pragma unroll 4
			for (int i = 0; i < kClockSeg / 4; i++) {
				const uint32_t gg = g2[i];
				const int ga = (int16_t)(gg & 0xffffu), gb = (int16_t)(gg >> 16);
				const uint32_t ca = l_tab[idx], cb = l_tab[(idx + step) & (kClockSeg - 1)];
				idx = (idx + 2 * step) & (kClockSeg - 1);
				xr += (long long)(ga * (int16_t)(ca & 0xffffu) + gb * (int16_t)(cb & 0xffffu));
				xi += (long long)(ga * (int16_t)(ca >> 16) + gb * (int16_t)(cb >> 16));
			}
			l_part[half][bin][0] = xr;
			l_part[half][bin][1] = xi;
			__syncthreads();
			if (t < kClockBins) {
				const long long re = (l_part[0][t][0] + l_part[1][t][0]) >> 16, im = (l_part[0][t][1] + l_part[1][t][1]) >> 16;  // (|.| < 2^24)
				pacc += (unsigned long long)(re * re) + (unsigned long long)(im * im);
			}
		}
		tfrec_amd_clock *o = out + (e0 + (unsigned)k);
		if (t < kClockBins) {
			if (pacc)
				atomicAdd(reinterpret_cast<unsigned long long *>(&o->spec[t]), pacc);
		} else if (t == kClockBins) {
			if (nseg)
				atomicAdd(&o->n_segments, nseg);
		} else if (t == kClockBins + 1) {
			if (nsil)
				atomicAdd(&o->n_silent, nsil);
		}
	}
}

hipError_t launch_burst_clock(hipStream_t st, const FrontOut &o, const CaptureBufs &b, tfrec_amd_clock *out)
{
	launch_run_records_init(st, b, out, nullptr);
	hipLaunchKernelGGL(clock_accum_kernel, dim3(o.n_blocks, o.n_streams), dim3(kClockThreads), 0, st, o.dec, o.dec_stride, o.n_blocks,
			   b.stage, b.stage_cap, b.cnt, b.base, b.max_runs, out);
	return hipGetLastError();
}
