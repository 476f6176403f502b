// tfrec_amd/csrc/decin.h -- the channel-rate front end (tfrec_amd_create_decimated, tfrec_amd_submit_runs): input rows
// that already hold the decimated int16 (I, Q) pairs at 384 kS/s -> dec, the trigger mask and prevdec, the three things everything
// behind the front end reads.  No filter: per component v' = max(v, -32767), dec[n] = (I', Q'), mask bit n = |I'| + |Q'| > thresh.
// Plus the recorder's gather of the sample ahead of every run (tfrec_amd_enable_capture_pre).  Included by frontend.hip (inside
// namespace tfrec).  tfrec_amd/decin.py restates the results.
//
// Both kernels share one body.  A lane owns four consecutive samples (16 bytes in, 16 bytes out), a wave 256 samples = four mask
// words, a workgroup of 256 lanes 1024 samples per step and eight steps per block.  The mask words come from four ballots (ballot
// j: the lanes' sample j): word w of the wave's four interleaves bits [16 w, 16 w + 16) of the four, and lane w < 4 writes it --
// one writer per word, no atomics.
//
// Grid: kDecinPersist persistent workgroups that take the (stream, block) pairs in turn, as the front end does (kFrontPersist,
// and for its reason: the kernel runs on the context's highest-priority stream, where a grid of one workgroup per tile held the
// dispatcher for the whole kernel and nothing of another stream started beside it).  A block is 32 KiB in and 32 KiB + 1 KiB out,
// so a workgroup per 1024-sample step would be 8 x as many workgroups with nothing to amortise; 2048 workgroups of 256 lanes are
// one round of 8 per CU.  Not measured against the alternative: profiles/decin_cost.txt says what was.
//
// The carried pair: prevdec[s] of a submit is the stream's last pair of the submit before, (0, 0) at a start or restart
// (stream_reset_kernel clears last[s]).  ONE lane reads last[s] and then writes it -- lane 0 of the workgroup that has the stream's
// block 0, which fetches the submit's last pair itself --, so no two workgroups meet on it.
#pragma once

constexpr int kDecinThreads = 256;
constexpr int kDecinStep = 4 * kDecinThreads;  // samples per step
constexpr int kDecinPersist = 2048;
static_assert(kBlockDec % kDecinStep == 0, "decin kernels: a block is a whole number of steps");

typedef short decin_s16x2 __attribute__((ext_vector_type(2)));

// v' = max(v, -32767) per int16 half: I * I + Q * Q and every product downstream stays inside int32
__device__ inline uint32_t decin_clamp(uint32_t w)
{
	decin_s16x2 v;
	__builtin_memcpy(&v, &w, 4);
	v = __builtin_elementwise_max(v, decin_s16x2{ -32767, -32767 });
	__builtin_memcpy(&w, &v, 4);
	return w;
}

__device__ inline bool decin_over(uint32_t w, int thresh)
{
	const int i = (int16_t)(w & 0xffffu), q = (int16_t)(w >> 16);
	return abs(i) + abs(q) > thresh;
}

// bit k of a 16-bit value -> bit 4 k
__device__ inline unsigned long long decin_spread4(unsigned long long x)
{
	x = (x | (x << 24)) & 0x000000ff000000ffull;
	x = (x | (x << 12)) & 0x000f000f000f000full;
	x = (x | (x << 6)) & 0x0303030303030303ull;
	x = (x | (x << 3)) & 0x1111111111111111ull;
	return x;
}

// A sparse submit's view of one row (tfrec_amd_submit_runs): its runs are tab[r0 .. r1), ordered by start, at least one sample
// apart; tab[k] = { start, end (exclusive), pool offset low, high }; pre[k] goes at start - 1 when start > 0.
struct DecinRuns {
	const uint4 *tab;
	const uint32_t *pool, *pre;
	int r0, r1;
};

// the first run of the row that ends behind sample n (r1: none)
__device__ inline int decin_find(const DecinRuns &R, int n)
{
	int lo = R.r0, hi = R.r1;
	while (lo < hi) {
		const int mid = (lo + hi) >> 1;
		if ((int)R.tab[mid].y > n)
			hi = mid;
		else
			lo = mid + 1;
	}
	return lo;
}

// sample n of the expanded row, k = decin_find(n): a run's pair, the pair ahead of a run, or zero -- written without a load
__device__ inline uint32_t decin_fetch(const DecinRuns &R, int n, int k)
{
	if (k >= R.r1)
		return 0u;
	const uint4 r = R.tab[k];
	if (n >= (int)r.x) {
		const unsigned long long off = (unsigned long long)r.z | ((unsigned long long)r.w << 32);
		return R.pool[off + (unsigned)(n - (int)r.x)];
	}
	return n == (int)r.x - 1 ? R.pre[k] : 0u;
}

// SPARSE = false: row chan[s].z (chan == nullptr: row s) of `in`, int16 pairs.  SPARSE = true: the rows are given by the run table
// (first[s] .. first[s + 1]), the pool and pre; ov[s] = { 1, pair } replaces the carried pair as this submit's prevdec[s] (a run at
// the submit's first sample brings its own predecessor; the host leaves it out for a stream that restarts here).
// scfg != nullptr: the stream's own threshold.
template <bool SPARSE>
__global__ __launch_bounds__(kDecinThreads) void decin_kernel(const uint8_t *__restrict__ in, size_t stride, int n_blocks, int n_streams,
							       const uint4 *__restrict__ chan, const uint4 *__restrict__ tab,
							       const uint32_t *__restrict__ pool, const uint32_t *__restrict__ pre,
							       const int32_t *__restrict__ first, const uint2 *__restrict__ ov,
							       uint32_t *__restrict__ dec, size_t dec_stride,
							       unsigned long long *__restrict__ mask, size_t mask_stride,
							       uint32_t *__restrict__ prevdec, uint32_t *__restrict__ last, int thresh,
							       const StreamCfg *__restrict__ scfg)
{
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const int M = n_blocks * kBlockDec;
	const int n_work = n_blocks * n_streams;
	for (int w = blockIdx.x; w < n_work; w += gridDim.x) {
		const int s = w / n_blocks, b = w - s * n_blocks;
		const int th = scfg ? scfg[s].thresh : thresh;
		const uint32_t *row = nullptr;
		DecinRuns R = { tab, pool, pre, 0, 0 };
		if constexpr (SPARSE) {
			R.r0 = first[s];
			R.r1 = first[s + 1];
		} else {
			row = reinterpret_cast<const uint32_t *>(in + (size_t)(chan ? chan[s].z : (uint32_t)s) * stride);
		}
		uint32_t *drow = dec + (size_t)s * dec_stride;
		unsigned long long *mrow = mask + (size_t)s * mask_stride;
#pragma unroll 2
		for (int it = 0; it < kBlockDec / kDecinStep; it++) {
			const int n = b * kBlockDec + it * kDecinStep + 4 * tid;  // (a multiple of 4 below M: 16 bytes inside the row)
			uint32_t v[4];
			if constexpr (SPARSE) {
				int k = decin_find(R, n);
#pragma unroll
				for (int j = 0; j < 4; j++) {
					// (runs are not empty and a sample apart: one step passes at most one run's end)
					if (j && k < R.r1 && n + j >= (int)R.tab[k].y)
						k++;
					v[j] = decin_fetch(R, n + j, k);
				}
			} else {
				const uint4 x = *reinterpret_cast<const uint4 *>(row + n);
				v[0] = x.x;
				v[1] = x.y;
				v[2] = x.z;
				v[3] = x.w;
			}
			unsigned long long word = 0;
#pragma unroll
			for (int j = 0; j < 4; j++) {
				v[j] = decin_clamp(v[j]);
				const unsigned long long bal = __ballot(decin_over(v[j], th));
				// lane w < 4: bits [16 w, 16 w + 16) of ballot j are samples 64 w + 4 i + j of the wave's 256
				word |= decin_spread4((bal >> (16 * (lane & 3))) & 0xffffull) << j;
			}
			*reinterpret_cast<uint4 *>(drow + n) = make_uint4(v[0], v[1], v[2], v[3]);
			if (lane < 4)
				mrow[((b * kBlockDec + it * kDecinStep) >> 6) + 4 * wave + lane] = word;
		}
		if (b == 0 && tid == 0) {  // the carried pair: read, then written, by this lane alone
			uint32_t p = last[s];
			uint32_t e;
			if constexpr (SPARSE) {
				const uint2 o = ov[s];
				if (o.x)
					p = decin_clamp(o.y);
				e = decin_fetch(R, M - 1, decin_find(R, M - 1));
			} else {
				e = row[M - 1];
			}
			prevdec[s] = p;
			last[s] = decin_clamp(e);
		}
	}
}

static unsigned decin_grid(int n_streams, int n_blocks)
{
	return (unsigned)std::min<long>(kDecinPersist, (long)n_streams * n_blocks);
}

// chan != nullptr: a mapped context, stream s reads row chan[s].z
hipError_t launch_decin(hipStream_t st, const uint8_t *in, size_t stride, const uint4 *chan, const FrontOut &o, uint32_t *last, int thresh,
			const StreamCfg *scfg)
{
	hipLaunchKernelGGL(decin_kernel<false>, dim3(decin_grid(o.n_streams, o.n_blocks)), dim3(kDecinThreads), 0, st, in, stride, o.n_blocks,
			   o.n_streams, chan, nullptr, nullptr, nullptr, nullptr, nullptr, o.dec, o.dec_stride, o.mask, o.mask_stride, o.prevdec,
			   last, thresh, scfg);
	return hipGetLastError();
}

hipError_t launch_decin_runs(hipStream_t st, const RunsTables &r, const FrontOut &o, uint32_t *last, int thresh, const StreamCfg *scfg)
{
	hipLaunchKernelGGL(decin_kernel<true>, dim3(decin_grid(o.n_streams, o.n_blocks)), dim3(kDecinThreads), 0, st, nullptr, 0, o.n_blocks,
			   o.n_streams, nullptr, r.tab, r.pool, r.pre, r.first, r.ov, o.dec, o.dec_stride, o.mask, o.mask_stride, o.prevdec,
			   last, thresh, scfg);
	return hipGetLastError();
}

// tfrec_amd_enable_capture_pre: pre[e] = the decimated pair just ahead of run e of the submit's table -- dec[start - 1] inside the
// submit, the set's prevdec[s] for a run at its first sample ((0, 0) at a stream's start or restart).  Behind capture_copy_kernel
// on the recorder's lane: it reads the table entries that kernel wrote (those below max_runs), start_sample still counted from
// sample_base.
__global__ __launch_bounds__(256) void capture_pre_kernel(const tfrec_amd_run *__restrict__ runs, const CaptureHeader *__restrict__ hdr,
							   uint32_t max_runs, long long sample_base, const uint32_t *__restrict__ dec,
							   size_t dec_stride, const uint32_t *__restrict__ prevdec, uint32_t *__restrict__ pre)
{
	const unsigned long long total = hdr->n_runs;
	const uint32_t n = total < max_runs ? (uint32_t)total : max_runs;
	for (uint32_t e = blockIdx.x * 256u + threadIdx.x; e < n; e += gridDim.x * 256u) {
		const tfrec_amd_run r = runs[e];
		const long long rel = r.start_sample - sample_base;  // within [0, M)
		pre[e] = rel > 0 ? dec[(size_t)r.stream * dec_stride + (size_t)(rel - 1)] : prevdec[r.stream];
	}
}

hipError_t launch_capture_pre(hipStream_t st, const FrontOut &o, long long sample_base, const CaptureBufs &b, uint32_t *pre)
{
	const unsigned blocks = std::max(1u, std::min(256u, (b.max_runs + 255u) / 256u));
	hipLaunchKernelGGL(capture_pre_kernel, dim3(blocks), dim3(256), 0, st, b.runs, b.hdr, b.max_runs, sample_base, o.dec, o.dec_stride,
			   o.prevdec, pre);
	return hipGetLastError();
}
