// tfrec_amd/csrc/envelope.h -- the burst envelope (tfrec_amd_enable_burst_envelope, include/tfrec_amd.h: tfrec_amd_envelope; DESIGN.md
// 6r): per run of the recorder's table the over samples' count and last index, the gaps between them, and the energy and product
// sums split at the last over sample.  Three kernels (capture.h's run_records_init_kernel and the two passes) behind
// capture_copy_kernel (and the burst meter's) on the recorder's low-priority lane; they read the recorder's table and working set,
// the decimated samples, prevdec and the FINAL trigger mask, and nothing a demodulator owns.  Exact integers only: every combined
// quantity is an integer sum, count, maximum or minimum, so the order of the atomics cannot matter.  Included by frontend.hip
// (inside namespace tfrec) behind burst.h.  tfrec_amd/envelope.py restates the result.
#pragma once

static_assert(sizeof(tfrec_amd_envelope) == 128 && offsetof(tfrec_amd_envelope, n_over) == 24 && offsetof(tfrec_amd_envelope, last_over) == 28 &&
		      offsetof(tfrec_amd_envelope, energy_head) == 32 && offsetof(tfrec_amd_envelope, lead_not_over) == 56 &&
		      offsetof(tfrec_amd_envelope, dot_head) == 64 && offsetof(tfrec_amd_envelope, nprod_tail) == 96,
	      "the init kernel writes the record by dwords; envelope_accum_kernel takes the four product sums as one array");
// run_records_init_kernel's rule: the copied fields from the entry capture_copy_kernel wrote (its first 24 bytes are the record's),
// last_over = -1, lead_not_over = n_samples -- what a piece without an over sample keeps --, everything else zero
template <>
__device__ inline uint32_t run_record_word<tfrec_amd_envelope>(const uint32_t *src, int w)
{
	return w < 6 ? src[w] : w == 7 ? 0xffffffffu : w == 14 ? src[4] : 0u;
}

constexpr int kEnvMaskThreads = kCapMaskWords;  // envelope_mask_kernel: a workgroup per (stream, block), a mask word per lane
constexpr int kEnvThreads = 256;                // envelope_accum_kernel: a sample per lane and step

// Pass A.  Block blockIdx.x of stream blockIdx.y, from the mask words alone: for every run of the stream that meets the block
// (the index range [lo, hi) of the staged runs, found by capture_run_range) the words of the run's part of the block,
// a word per lane, cut to the run's samples ->
//   n_over         the words' popcounts, added;
//   last_over      the run-relative index of the part's highest bit, an atomic maximum;
//   per rising edge (an over sample whose predecessor inside the run is not over, or which is the run's first sample) the stretch
//   of not-over samples ahead of it, back to the last over sample before it: inside the lane's word, or in the nearest earlier
//   non-zero word at or behind the run's start.  Those words lie in the stream's mask row whichever block they belong to, so a
//   stretch that crosses a block boundary is measured whole by the one lane that holds its end, and a stretch counts once.
//   Found: a gap -- n_gaps + 1, max_gap an atomic maximum.  Not found: the edge is the run's first over sample and the stretch
//   is lead_not_over (an atomic minimum; one edge of a run at most).
// Inside a run two over samples lie fewer than wmax samples apart, and so do a CONTINUES piece's start and its first over
// sample: the search backwards reads wmax / 64 + 1 words at the most, and never one ahead of the word of the run's start.
// Sums and maxima are reduced over each wave; one round of integer atomics per wave that has something to add.
__global__ __launch_bounds__(kEnvMaskThreads) void envelope_mask_kernel(const unsigned long long *__restrict__ mask, size_t mask_stride,
									 const CaptureStage *__restrict__ stage, int stage_cap,
									 const uint2 *__restrict__ cnt, const uint4 *__restrict__ base,
									 uint32_t max_runs, tfrec_amd_envelope *__restrict__ out)
{
	const int b = blockIdx.x, s = blockIdx.y, t = threadIdx.x;
	const int nr = (int)cnt[s].x;  // (<= stage_cap)
	if (nr == 0)
		return;
	const CaptureStage *srow = stage + (size_t)s * stage_cap;
	const unsigned long long e0 = base[s].x;  // the stream's first table entry
	const int b0 = b * kBlockDec, b1 = b0 + kBlockDec;
	int lo, hi;
	capture_run_range(srow, nr, b0, b1, t, kEnvMaskThreads, lo, hi);
	const unsigned long long *mrow = mask + (size_t)s * mask_stride;
	for (int k = lo; k < hi; k++) {
		if (e0 + (unsigned)k >= max_runs)
			break;  // (and every later run of the stream: no record)
		const CaptureStage r = srow[k];
		const int a = r.start > b0 ? r.start : b0, e = r.end < b1 ? r.end : b1;  // b0 <= a < e <= b1 <= M
		const int w = (b0 >> 6) + t;  // this lane's word: samples [g0, g0 + 64) of the block
		const int g0 = w << 6;
		unsigned long long m = 0;
		if (g0 < e && g0 + 64 > a) {
			m = mrow[w];
			if (a > g0)
				m &= ~0ull << (a - g0);
			if (e < g0 + 64)
				m &= ~0ull >> (g0 + 64 - e);
		}
		int n_over = __popcll(m);
		int last = m ? g0 + 63 - __builtin_clzll(m) - r.start : -1;
		int gaps = 0, gmax = 0;
		// the sample ahead of the word, where it belongs to the run (then w >= 1)
		const unsigned long long prev = (m && g0 > r.start) ? mrow[w - 1] >> 63 : 0ull;
		unsigned long long rise = m & ~((m << 1) | prev);
		while (rise) {
			const int i = __builtin_ctzll(rise);
			rise &= rise - 1;
			const unsigned long long below = i ? m & (~0ull >> (64 - i)) : 0ull;
			int j = -1;  // the last over sample ahead of g0 + i, submit-relative
			if (below) {
				j = g0 + 63 - __builtin_clzll(below);
			} else {
				for (int v = w - 1; v >= (r.start >> 6); v--) {
					unsigned long long x = mrow[v];
					if ((v << 6) < r.start)
						x &= ~0ull << (r.start - (v << 6));
					if (x) {
						j = (v << 6) + 63 - __builtin_clzll(x);
						break;
					}
				}
			}
			if (j >= 0) {
				const int g = g0 + i - 1 - j;  // (> 0: the predecessor is not over)
				gaps++;
				gmax = g > gmax ? g : gmax;
			} else {
				atomicMin(&out[e0 + (unsigned)k].lead_not_over, (uint32_t)(g0 + i - r.start));
			}
		}
#pragma unroll
		for (int d = 32; d >= 1; d >>= 1) {
			n_over += __shfl_xor(n_over, d);
			gaps += __shfl_xor(gaps, d);
			const int ol = __shfl_xor(last, d), og = __shfl_xor(gmax, d);
			last = ol > last ? ol : last;
			gmax = og > gmax ? og : gmax;
		}
		if ((t & 63) == 0 && n_over) {
			tfrec_amd_envelope *o = out + (e0 + (unsigned)k);
			atomicAdd(&o->n_over, (uint32_t)n_over);
			atomicMax(&o->last_over, last);
			if (gaps) {
				atomicAdd(&o->n_gaps, (uint32_t)gaps);
				atomicMax(&o->max_gap, (uint32_t)gmax);
			}
		}
	}
}

// Pass B, behind pass A (the record's last_over is final).  Block blockIdx.x of stream blockIdx.y, with burst_accum_kernel's
// geometry and its products (the product at sample n pairs it with sample n - 1: inside the row, or prevdec[s] at the submit's
// first sample; left out at a run's first sample unless the run CONTINUES; skipped when dot == crs == 0): the energy, the
// product sums and the counts of the run's part of the block, each split by whether the sample's run-relative index is <=
// last_over.  Reduced over each wave, then in LDS; one round of integer atomics per (run, block).  The loops are uniform over the
// workgroup.
__global__ __launch_bounds__(kEnvThreads) void envelope_accum_kernel(const uint32_t *__restrict__ dec, size_t dec_stride,
								      const uint32_t *__restrict__ prevdec,
								      const CaptureStage *__restrict__ stage, int stage_cap,
								      const uint2 *__restrict__ cnt, const uint4 *__restrict__ base, uint32_t max_runs,
								      tfrec_amd_envelope *__restrict__ out)
{
	const int b = blockIdx.x, s = blockIdx.y, t = threadIdx.x;
	const int nr = (int)cnt[s].x;  // (<= stage_cap)
	if (nr == 0)
		return;
	const CaptureStage *srow = stage + (size_t)s * stage_cap;
	const unsigned long long e0 = base[s].x;
	__shared__ uint32_t l_np[2];
	__shared__ unsigned long long l_sum[6];  // energy head, tail; dot head, crs head, dot tail, crs tail
	if (t >= 2 && t < 4)
		l_np[t - 2] = 0;
	if (t >= 4 && t < 10)
		l_sum[t - 4] = 0;
	const int b0 = b * kBlockDec, b1 = b0 + kBlockDec;
	int lo, hi;
	capture_run_range(srow, nr, b0, b1, t, kEnvThreads, lo, hi);
	const uint32_t *row = dec + (size_t)s * dec_stride;
	for (int k = lo; k < hi; k++) {
		if (e0 + (unsigned)k >= max_runs)
			break;  // (and every later run of the stream: no record)
		tfrec_amd_envelope *o = out + (e0 + (unsigned)k);
		const CaptureStage r = srow[k];
		const bool cont = (r.flags & TFREC_AMD_RUN_CONTINUES) != 0;
		const int split = r.start + o->last_over;  // the last head sample, submit-relative (r.start - 1: none)
		const int a = r.start > b0 ? r.start : b0, e = r.end < b1 ? r.end : b1;  // b0 <= a < e <= b1 <= M
		long long eh = 0, et = 0, dh = 0, ch = 0, dt = 0, ct = 0, nh = 0, nt = 0;
		for (int n = a + t; n < e; n += kEnvThreads) {
			const uint32_t w = row[n];
			const int I = (int16_t)(w & 0xffffu), Q = (int16_t)(w >> 16);
			const bool head = n <= split;
			const long long en = (long long)((unsigned)(I * I) + (unsigned)(Q * Q));  // (<= 2^31)
			eh += head ? en : 0;
			et += head ? 0 : en;
			if (n > r.start || cont) {
				const uint32_t wp = n > 0 ? row[n - 1] : prevdec[s];
				const int Ip = (int16_t)(wp & 0xffffu), Qp = (int16_t)(wp >> 16);
				const long long dot = (long long)I * Ip + (long long)Q * Qp, crs = (long long)Q * Ip - (long long)I * Qp;
				if (dot | crs) {
					dh += head ? dot : 0;
					ch += head ? crs : 0;
					dt += head ? 0 : dot;
					ct += head ? 0 : crs;
					nh += head;
					nt += !head;
				}
			}
		}
		const long long v[8] = { burst_wave_sum(eh), burst_wave_sum(et), burst_wave_sum(dh), burst_wave_sum(ch),
					 burst_wave_sum(dt), burst_wave_sum(ct), burst_wave_sum(nh), burst_wave_sum(nt) };
		if ((t & 63) == 0) {
#pragma unroll
			for (int i = 0; i < 6; i++)
				if (v[i])
					atomicAdd(&l_sum[i], (unsigned long long)v[i]);
			if (v[6])
				atomicAdd(&l_np[0], (uint32_t)v[6]);
			if (v[7])
				atomicAdd(&l_np[1], (uint32_t)v[7]);
		}
		__syncthreads();
		if (t < 2) {  // energy_head, energy_tail: two consecutive 64-bit fields
			if (l_sum[t])
				atomicAdd(reinterpret_cast<unsigned long long *>(&o->energy_head) + t, l_sum[t]);
			l_sum[t] = 0;
		} else if (t < 6) {  // dot_head, crs_head, dot_tail, crs_tail: four more
			if (l_sum[t])
				atomicAdd(reinterpret_cast<unsigned long long *>(&o->dot_head) + (t - 2), l_sum[t]);
			l_sum[t] = 0;
		} else if (t < 8) {
			if (l_np[t - 6])
				atomicAdd(t == 6 ? &o->nprod_head : &o->nprod_tail, l_np[t - 6]);
			l_np[t - 6] = 0;
		}
		__syncthreads();
	}
}

hipError_t launch_burst_envelope(hipStream_t st, const FrontOut &o, const CaptureBufs &b, tfrec_amd_envelope *out)
{
	launch_run_records_init(st, b, out, nullptr);
	hipLaunchKernelGGL(envelope_mask_kernel, dim3(o.n_blocks, o.n_streams), dim3(kEnvMaskThreads), 0, st, o.mask, o.mask_stride, b.stage,
			   b.stage_cap, b.cnt, b.base, b.max_runs, out);
	hipLaunchKernelGGL(envelope_accum_kernel, dim3(o.n_blocks, o.n_streams), dim3(kEnvThreads), 0, st, o.dec, o.dec_stride, o.prevdec, b.stage,
			   b.stage_cap, b.cnt, b.base, b.max_runs, out);
	return hipGetLastError();
}
