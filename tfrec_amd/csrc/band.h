// tfrec_amd/csrc/band.h -- the burst band (tfrec_amd_enable_burst_band, include/tfrec_amd.h: tfrec_amd_band): per run of
// the recorder's table the power spectrum of the burst's own IQ, 256 bins of 750 Hz over -96 .. +95.25 kHz, Hann-windowed, summed over
// the 512-sample segments that lie wholly inside the run.  capture.h's run_records_init_kernel, band_list_kernel and
// band_product_kernel, on the recorder's low-priority lane behind the envelope clock's kernels; once, at enable, band_planes_kernel.
// They read the recorder's table and working set and the decimated samples.  Exact integers only: every combined quantity is an
// integer sum, so neither the order of the atomics nor the grouping of the matrix instruction's sums can matter.  Included by
// frontend.hip (inside namespace tfrec) behind keying.h.  tfrec_amd/band.py restates the result.
//
// With I and Q stacked along k the complex DFT of a segment is ONE real product, segments as rows:
//   X[32 x 512] = w[32 x 1024] B[1024 x 512],   w = (wI[0 .. 511], wQ[0 .. 511]),   column pairs (re_j, im_j),
//   B[m'][re_j] = C[t]   B[m'][im_j] = -S[t]     (the wI rows)          t = (8 j m') & 4095, S[i] = C[(i - 1024) & 4095]
//   B[512 + m'][re_j] = S[t]   B[512 + m'][im_j] = C[t]     (the wQ rows)
// on __builtin_amdgcn_mfma_i32_16x16x64_i8.  The split into int8 planes:
//   w = 128 wh + wl,       wh = w >> 7 (arithmetic), wl = w & 127:  -64 <= wh <= 63, 0 <= wl <= 127 (-2^13 <= w < 2^13);
//   T = 256 th + tl + 128, th = T >> 8 (arithmetic), tl = (T & 255) - 128:  -128 <= th, tl <= 127.  |C| <= 32767 (the table is
//                          round(32767 cos)), so -S never reaches 32768 and th of -S never 128; the offset comes back as a rank-one
//                          term, 128 (sum wI + sum wQ) on every column;
//   sum w T = 2^15 sum wh th + 2^7 sum wh tl + 2^8 sum wl th + sum wl tl + 128 sum w.
// A plane product is at most 127 * 128 < 2^14 in magnitude and a sum has 1024 terms: every int32 accumulator stays below 2^24, with
// nothing rounded or saturated; the five terms meet in int64 (|X| < 2^38).
#pragma once

static_assert(sizeof(tfrec_amd_band) == 2080 && offsetof(tfrec_amd_band, n_segments) == 24 && offsetof(tfrec_amd_band, spec) == 32,
	      "the init kernel copies a table entry's first 24 bytes and zeroes the rest");
// run_records_init_kernel's rule: the clock's
template <>
__device__ inline uint32_t run_record_word<tfrec_amd_band>(const uint32_t *src, int w)
{
	return w < 6 ? src[w] : 0u;
}

constexpr int kBandSeg = 512;      // samples per segment
constexpr int kBandBins = 256;     // bins j = -128 .. 127, spec[j + 128]
constexpr int kBandShift = 14;     // P = (X_re >> 14)^2 + (X_im >> 14)^2
constexpr int kBandK = 2 * kBandSeg;       // the product's depth: the 512 wI, then the 512 wQ
constexpr int kBandCols = 2 * kBandBins;   // the product's columns: column tile 2 g is X_re of the bins 16 g - 128 .. 16 g - 113, tile 2 g + 1 their X_im
constexpr int kBandTile = 32;      // H: segments per workgroup, two row tiles of the instruction
constexpr int kBandThreads = 512;  // band_product_kernel: 8 waves, wave w = row tile w >> 2 x the column tiles [8 (w & 3), + 8)
constexpr int kBandChunk = 64;     // k per step: one instruction's depth
constexpr int kBandChunks = kBandK / kBandChunk;
// One plane's operand block of a chunk and a 16-row or 16-column tile: 64 lanes x 16 bytes, lane l = row or column (l & 15), k = 16 (l >> 4) + byte
constexpr int kBandOperand = 64 * 16;
constexpr int kBandChunkB = 2 * (kBandCols / 16) * kBandOperand;  // a chunk of B: [plane th, tl][32 column tiles][operand], 64 KB
constexpr int kBandPlaneA = (kBandTile / 16) * kBandChunks * kBandOperand;  // a plane of the tile's w: [2 row tiles][16 chunks][operand], 32 KB
static_assert(kBandPlaneBytes == (size_t)kBandChunks * kBandChunkB, "1 MB: both planes of the 1024 x 512 matrix (launch.h)");
static_assert(kBlockDec == 16 * kBandSeg && kTuneN == 8 * kBandSeg, "a block is 16 whole segments; the window and bin j step 8 and 8 j entries of the 4096-entry table per sample");
static_assert(kBandChunkB == 8 * kBandThreads * 16 && kBandTile * kBandSeg == 4 * kBandThreads * 8, "a lane stages 8 x 16 bytes of B a chunk, and 8 samples of 4 rows once");
static_assert(2 * kBandPlaneA + kBandChunkB + 3 * kBandTile * 4 <= 160 * 1024, "the resident tile and a chunk of B fit the 160 KB of LDS");

typedef int band_v4i __attribute__((ext_vector_type(4)));
typedef uint32_t band_v4u __attribute__((ext_vector_type(4)));

// B's planes, once: 16 bytes of either plane per lane, in the layout band_product_kernel reads
__global__ __launch_bounds__(256) void band_planes_kernel(int8_t *__restrict__ planes)
{
	const uint32_t u = blockIdx.x * 256 + threadIdx.x;  // (chunk, column tile, lane)
	if (u >= (uint32_t)(kBandChunks * (kBandCols / 16) * 64))
		return;
	const uint32_t l = u & 63, n = (u >> 6) & 31, kc = u >> 11;
	const int j = (int)((n >> 1) * 16 + (l & 15)) - kBandBins / 2;
	const bool im = n & 1;
	uint32_t hi[4] = {}, lo[4] = {};
	for (uint32_t b = 0; b < 16; b++) {
		const uint32_t k = kc * kBandChunk + 16 * (l >> 4) + b;
		const int m = (int)(k & (kBandSeg - 1));
		const bool q_row = k >= (uint32_t)kBandSeg;
		const int t = 8 * j * m;            // (masked below: two's complement)
		const bool sine = q_row != im;      // re_j takes S from the wQ rows, im_j -S from the wI rows
		int T = kTuneCos[(t - (sine ? kTuneN / 4 : 0)) & (kTuneN - 1)];  // S[i] = C[i - 1024]
		if (im && !q_row)
			T = -T;  // (|T| <= 32767)
		hi[b >> 2] |= (uint32_t)(uint8_t)(T >> 8) << (8 * (b & 3));
		lo[b >> 2] |= (uint32_t)(uint8_t)((T & 255) - 128) << (8 * (b & 3));
	}
	uint4 *dst = reinterpret_cast<uint4 *>(planes + (size_t)kc * kBandChunkB) + n * 64 + l;
	dst[0] = make_uint4(hi[0], hi[1], hi[2], hi[3]);
	dst[(kBandCols / 16) * 64] = make_uint4(lo[0], lo[1], lo[2], lo[3]);
}

// The whole segments of a stream's runs that have a record
__device__ inline uint32_t band_stream_segments(const CaptureStage *__restrict__ srow, int nr, unsigned long long e0, uint32_t max_runs)
{
	uint32_t c = 0;
	for (int k = 0; k < nr && e0 + (unsigned)k < max_runs; k++) {
		const int q0 = (srow[k].start + kBandSeg - 1) / kBandSeg, q1 = srow[k].end / kBandSeg;
		c += q1 > q0 ? (uint32_t)(q1 - q0) : 0u;
	}
	return c;
}

// The work list: { table entry, submit-relative first sample } of every whole segment of every run below max_runs, by stream, run
// and segment -- the order of the table --, and its length.  A stream's runs are disjoint, so the list holds at most 16 n_blocks
// entries a stream: `cap`, eight times the envelope clock's, and writing it is what takes the time.  So not one workgroup: a wave per
// 64 streams, a stream per lane, each on a compute unit of its own.  Where its part of the list begins the wave finds by counting
// the streams ahead of its own once more, a strided share per lane -- at most n_streams / 64 more streams a lane, against the 16
// n_blocks entries it may write --: no second kernel, no atomic, and the list's order stays the table's.  Shuffles only; no LDS.
__global__ __launch_bounds__(64) void band_list_kernel(const CaptureStage *__restrict__ stage, int stage_cap, const uint2 *__restrict__ cnt,
						       const uint4 *__restrict__ base, int n_streams, uint32_t max_runs, uint2 *__restrict__ work,
						       uint32_t cap, uint32_t *__restrict__ n_work)
{
	const int lane = threadIdx.x, s_first = blockIdx.x * 64;
	uint32_t before = 0;  // the segments of the streams ahead of this wave's
	for (int s = lane; s < s_first; s += 64)
		before += band_stream_segments(stage + (size_t)s * stage_cap, (int)cnt[s].x, base[s].x, max_runs);
	before = (uint32_t)burst_wave_sum((long long)before);
	const int s = s_first + lane;
	const CaptureStage *srow = stage + (size_t)(s < n_streams ? s : 0) * stage_cap;
	const int nr = s < n_streams ? (int)cnt[s].x : 0;
	const unsigned long long e0 = s < n_streams ? base[s].x : 0;
	const uint32_t c = band_stream_segments(srow, nr, e0, max_runs);
	uint32_t at = before + (uint32_t)cap_prefix_excl((int)c, lane);
	if (blockIdx.x == gridDim.x - 1 && lane == 63)
		*n_work = at + c < cap ? at + c : cap;
	for (int k = 0; k < nr && e0 + (unsigned)k < max_runs; k++) {
		const int q0 = (srow[k].start + kBandSeg - 1) / kBandSeg, q1 = srow[k].end / kBandSeg;
		for (int q = q0; q < q1; q++, at++)
			if (at < cap)
				work[at] = make_uint2((uint32_t)(e0 + (unsigned)k), (uint32_t)(q * kBandSeg));
	}
}

// Tile blockIdx.x of the work list: its H = 32 segments are the rows of one matrix product against B.  Unlike the envelope clock's
// tile, whose 32 x 4096 samples are streamed, this one's 32 x 1024 operand bytes a plane fit LDS: the tile is staged ONCE and stays.
//   1. Wave w stages the rows 4 w .. 4 w + 3, lane l the samples 8 l .. 8 l + 7 of each, from two 16-byte loads a row that are all
//      issued before the first is used -- the samples are read once and never leave the registers: mx over the wave by shuffles, sh,
//      x = (I, Q) >> sh, w = (x Wn) >> 16 with the lane's 8 window values, the split into wh and wl written to the A operand's
//      place in LDS (plane, row tile, chunk, lane = row & 15 + 16 (k >> 4), byte k & 15; wI at k = m', wQ at k = 512 + m'), and the
//      row's sum of w by shuffles.  A row behind the list's end, and a silent segment, is staged as zeros.
//   2. 16 steps of k = 64.  The step's chunk of B's planes is laid out as the B operand wants it: a plain copy, global memory to
//      LDS, 8 x 16 bytes a lane, and one contiguous 16-byte read per lane and operand in the product loop.  All 8 waves read it
//      from LDS: the workgroup streams B once, in one pass over all 512 columns.  The next step's chunk is loaded into registers
//      ahead of this step's 32 instructions.  Wave w keeps 32 accumulators: its row tile x 8 column tiles x the four plane products.
//   3. lane (column c, rows 4 g .. 4 g + 3) holds X_re and X_im of bin 64 (w & 3) + 16 u + c - 128 for u = 0 .. 3 in the same
//      registers' places: the five terms in int64, P = (X_re >> 14)^2 + (X_im >> 14)^2, one 64-bit atomic per (segment, bin) where P
//      != 0, and one 32-bit atomic per segment for its count.
// Every loop and barrier is uniform over the workgroup.  No floating point.
__global__ __launch_bounds__(kBandThreads) void band_product_kernel(const uint32_t *__restrict__ dec, size_t dec_stride,
								    const uint2 *__restrict__ work, const uint32_t *__restrict__ n_work,
								    const int8_t *__restrict__ planes, tfrec_amd_band *__restrict__ out)
{
	const uint32_t nw = *n_work, w0 = blockIdx.x * kBandTile;
	if (w0 >= nw)
		return;
	const int t = threadIdx.x, lane = t & 63, w = t >> 6;
	__shared__ __attribute__((aligned(16))) int8_t l_a[2 * kBandPlaneA];
	__shared__ __attribute__((aligned(16))) int8_t l_b[kBandChunkB];
	__shared__ uint32_t l_ent[kBandTile], l_mx[kBandTile];  // (l_mx 0: an empty or silent row)
	__shared__ int l_sum[kBandTile];
	band_v4u pb[8];  // the first chunk of B, in flight behind the staging
	const band_v4u *gb = reinterpret_cast<const band_v4u *>(planes) + t;
#pragma unroll
	for (int i = 0; i < 8; i++)
		pb[i] = gb[i * kBandThreads];
	{
		uint4 z[4][2];
		uint32_t ent[4];
#pragma unroll
		for (int i = 0; i < 4; i++) {
			const int r = 4 * w + i;  // (wave-uniform)
			ent[i] = 0;
			z[i][0] = z[i][1] = make_uint4(0, 0, 0, 0);
			if (w0 + r < nw) {
				const uint2 we = work[w0 + r];
				ent[i] = we.x;
				const uint4 *src = reinterpret_cast<const uint4 *>(dec + (size_t)out[we.x].stream * dec_stride + we.y);  // (the init kernel copied the entry's stream)
				z[i][0] = src[2 * lane];
				z[i][1] = src[2 * lane + 1];
			}
		}
		int wn[8];  // Wn[8 lane + p]
#pragma unroll
		for (int p = 0; p < 8; p++)
			wn[p] = 32767 - kTuneCos[8 * (8 * lane + p)];
		// samples 8 lane .. 8 lane + 7: chunk lane >> 3 (wQ: + 8), operand lane (row & 15) + 16 ((lane & 7) >> 1), bytes 8 (lane & 1) ..
		const int a_at = ((lane >> 3) * 64 + 16 * ((lane & 7) >> 1)) * 16 + 8 * (lane & 1);
#pragma unroll
		for (int i = 0; i < 4; i++) {
			const int r = 4 * w + i;
			const uint32_t zz[8] = { z[i][0].x, z[i][0].y, z[i][0].z, z[i][0].w, z[i][1].x, z[i][1].y, z[i][1].z, z[i][1].w };
			uint32_t mx = 0;
#pragma unroll
			for (int p = 0; p < 8; p++) {
				const int I = (int16_t)(zz[p] & 0xffffu), Q = (int16_t)(zz[p] >> 16);
				const uint32_t aI = (uint32_t)(I < 0 ? -I : I), aQ = (uint32_t)(Q < 0 ? -Q : Q);  // (|-32768| = 32768)
				mx = aI > mx ? aI : mx;
				mx = aQ > mx ? aQ : mx;
			}
#pragma unroll
			for (int d = 32; d >= 1; d >>= 1) {
				const uint32_t o = (uint32_t)__shfl_xor((int)mx, d);
				mx = o > mx ? o : mx;
			}
			const int bits = 32 - __clz((int)mx);
			const int sh = bits > 13 ? bits - 13 : 0;
			uint32_t hI[2] = {}, lI[2] = {}, hQ[2] = {}, lQ[2] = {};
			int sum = 0;
#pragma unroll
			for (int p = 0; p < 8; p++) {
				const int I = (int16_t)(zz[p] & 0xffffu), Q = (int16_t)(zz[p] >> 16);
				const int wI = ((I >> sh) * wn[p]) >> 16, wQ = ((Q >> sh) * wn[p]) >> 16;  // (|x Wn| < 2^13 * 2^16)
				sum += wI + wQ;
				hI[p >> 2] |= (uint32_t)(uint8_t)(wI >> 7) << (8 * (p & 3));
				lI[p >> 2] |= (uint32_t)(wI & 127) << (8 * (p & 3));
				hQ[p >> 2] |= (uint32_t)(uint8_t)(wQ >> 7) << (8 * (p & 3));
				lQ[p >> 2] |= (uint32_t)(wQ & 127) << (8 * (p & 3));
			}
			int8_t *a = l_a + (r >> 4) * (kBandChunks * kBandOperand) + (r & 15) * 16 + a_at;
			*reinterpret_cast<uint2 *>(a) = make_uint2(hI[0], hI[1]);
			*reinterpret_cast<uint2 *>(a + kBandPlaneA) = make_uint2(lI[0], lI[1]);
			*reinterpret_cast<uint2 *>(a + (kBandChunks / 2) * kBandOperand) = make_uint2(hQ[0], hQ[1]);
			*reinterpret_cast<uint2 *>(a + (kBandChunks / 2) * kBandOperand + kBandPlaneA) = make_uint2(lQ[0], lQ[1]);
			sum = (int)burst_wave_sum((long long)sum);
			if (lane == 0) {
				l_ent[r] = ent[i];
				l_mx[r] = mx;
				l_sum[r] = sum;
			}
		}
	}
	const int wm = w >> 2, wc = w & 3;
	band_v4i acc[8][4];  // [column tile][wh th, wh tl, wl th, wl tl]
#pragma unroll
	for (int n = 0; n < 8; n++)
#pragma unroll
		for (int p = 0; p < 4; p++)
			acc[n][p] = band_v4i{ 0, 0, 0, 0 };
	for (int kc = 0; kc < kBandChunks; kc++) {
		__syncthreads();  // (the step before has read l_b; ahead of the first step: the tile is staged)
#pragma unroll
		for (int i = 0; i < 8; i++)
			reinterpret_cast<band_v4u *>(l_b)[t + i * kBandThreads] = pb[i];
		__syncthreads();
		{  // the next step's, in flight behind this step's products (the last step loads its own again)
			const int kn = kc + 1 < kBandChunks ? kc + 1 : kc;
			const band_v4u *nb = gb + (size_t)kn * (kBandChunkB / 16);
#pragma unroll
			for (int i = 0; i < 8; i++)
				pb[i] = nb[i * kBandThreads];
		}
		const band_v4i ah = reinterpret_cast<const band_v4i *>(l_a)[(wm * kBandChunks + kc) * 64 + lane];
		const band_v4i al = reinterpret_cast<const band_v4i *>(l_a + kBandPlaneA)[(wm * kBandChunks + kc) * 64 + lane];
#pragma unroll
		for (int n = 0; n < 8; n++) {
			const band_v4i bh = reinterpret_cast<const band_v4i *>(l_b)[(wc * 8 + n) * 64 + lane];
			const band_v4i bl = reinterpret_cast<const band_v4i *>(l_b + kBandChunkB / 2)[(wc * 8 + n) * 64 + lane];
			acc[n][0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ah, bh, acc[n][0], 0, 0, 0);
			acc[n][1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ah, bl, acc[n][1], 0, 0, 0);
			acc[n][2] = __builtin_amdgcn_mfma_i32_16x16x64_i8(al, bh, acc[n][2], 0, 0, 0);
			acc[n][3] = __builtin_amdgcn_mfma_i32_16x16x64_i8(al, bl, acc[n][3], 0, 0, 0);
		}
	}
	// the instruction's result: register i of lane l is row 4 (l >> 4) + i, column l & 15 of the 16 x 16 tile
	const int col = lane & 15;
#pragma unroll
	for (int i = 0; i < 4; i++) {
		const int r = wm * 16 + 4 * (lane >> 4) + i;
		if (!l_mx[r])
			continue;  // empty or silent: nothing to add
		tfrec_amd_band *o = out + l_ent[r];
		const long long rank1 = 128LL * l_sum[r];
#pragma unroll
		for (int u = 0; u < 4; u++) {
			long long X[2];
#pragma unroll
			for (int part = 0; part < 2; part++) {
				const int n = 2 * u + part;
				X[part] = (long long)acc[n][0][i] * 32768 + (long long)acc[n][1][i] * 128 + (long long)acc[n][2][i] * 256 + (long long)acc[n][3][i] + rank1;
			}
			const long long re = X[0] >> kBandShift, im = X[1] >> kBandShift;  // (|.| < 2^24)
			const unsigned long long P = (unsigned long long)(re * re) + (unsigned long long)(im * im);
			if (P)
				atomicAdd(reinterpret_cast<unsigned long long *>(&o->spec[(wc * 4 + u) * 16 + col]), P);
		}
	}
	if (t < kBandTile && w0 + t < nw)  // the counts: a lane per row of the tile
		atomicAdd(l_mx[t] ? &out[l_ent[t]].n_segments : &out[l_ent[t]].n_silent, 1u);
}

hipError_t launch_band_planes(hipStream_t st, int8_t *planes)
{
	hipLaunchKernelGGL(band_planes_kernel, dim3(kBandChunks * (kBandCols / 16) * 64 / 256), dim3(256), 0, st, planes);
	return hipGetLastError();
}

hipError_t launch_burst_band(hipStream_t st, const FrontOut &o, const CaptureBufs &b, const BandBufs &k)
{
	const uint32_t cap = 16u * (uint32_t)o.n_blocks * (uint32_t)o.n_streams;  // (<= the buffer's: the context's largest submit)
	launch_run_records_init(st, b, k.recs, nullptr);
	hipLaunchKernelGGL(band_list_kernel, dim3((o.n_streams + 63) / 64), dim3(64), 0, st, b.stage, b.stage_cap, b.cnt, b.base, o.n_streams, b.max_runs,
			   k.work, cap, k.n_work);
	hipLaunchKernelGGL(band_product_kernel, dim3((cap + kBandTile - 1) / kBandTile), dim3(kBandThreads), 0, st, o.dec, o.dec_stride, k.work, k.n_work,
			   k.planes, k.recs);
	return hipGetLastError();
}
