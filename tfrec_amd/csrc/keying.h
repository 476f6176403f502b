// tfrec_amd/csrc/keying.h -- the envelope clock (tfrec_amd_enable_burst_keying, include/tfrec_amd.h: "Envelope clock"):
// per run of the recorder's table the power spectrum, 128 bins of 93.75 Hz, of the burst's amplitude |I| + |Q|, summed over the
// 4096-sample segments that lie wholly inside the run: it peaks at the rate an on-off keyed burst is keyed at.  The record is the
// burst clock's (tfrec_amd_clock), so capture.h's run_records_init_kernel instance of clock.h serves; behind it keying_list_kernel
// and keying_product_kernel, on the recorder's low-priority lane behind the clock's kernels; once, at enable, keying_planes_kernel.
// They read the recorder's table and working set and the decimated samples.  Exact integers only: every combined quantity is an
// integer sum, so neither the order of the atomics nor the grouping of the matrix instruction's sums can matter.  Included by
// frontend.hip (inside namespace tfrec) behind clock.h.  tfrec_amd/clock.py (keyings) restates the result.
//
// The DFT of a segment is a 4096-term integer dot product per bin and part: with the segments as rows it is the matrix product
// X[32 x 256] = x[32 x 4096] T[4096 x 256], T[k][col] = C or S at (j k) mod 4096, on __builtin_amdgcn_mfma_i32_16x16x64_i8.
// The split into int8 planes:
//   x = 128 xh + xl,       xh = x >> 7, xl = x & 127:  0 <= xh, xl <= 127 (0 <= x < 2^14): seven-bit planes, no correction;
//   T = 256 th + tl + 128, th = T >> 8 (arithmetic), tl = (T & 255) - 128:  -128 <= th, tl <= 127 (|T| <= 32767; a balanced byte
//                          split of 32767 would need a high byte of 128), the offset back in as a rank-one term;
//   sum x T = 2^15 sum xh th + 2^7 sum xh tl + 2^8 sum xl th + sum xl tl + 128 sum x.
// A plane product is at most 127 * 128 < 2^14 in magnitude and a sum has 4096 terms: below 2^26, inside the int32 accumulator with
// nothing rounded or saturated; the five terms meet in int64 (|X| < 2^41).
#pragma once

constexpr int kKeySeg = 4096;     // samples per segment
constexpr int kKeyBins = 128;     // bins j = 1 .. 128, spec[j - 1]
constexpr int kKeyShift = 17;     // P = (X_re >> 17)^2 + (X_im >> 17)^2
constexpr int kKeyCols = 2 * kKeyBins;  // the product's columns: column tile 2 u is X_re of bins 16 u + 1 .. 16 u + 16, tile 2 u + 1 their X_im
constexpr int kKeyTile = 32;      // H: segments per workgroup, two row tiles of the instruction
constexpr int kKeyThreads = 256;  // keying_product_kernel: 4 waves, wave w = row tile w >> 1 x the column tiles [8 (w & 1), + 8)
constexpr int kKeyChunk = 64;     // k per step: one instruction's depth
constexpr int kKeyChunks = kKeySeg / kKeyChunk;
// One plane's operand block of a chunk and a 16-column tile: 64 lanes x 16 bytes, lane l = column (l & 15), k = 16 (l >> 4) + byte
constexpr int kKeyOperand = 64 * 16;
constexpr int kKeyChunkB = 2 * (kKeyCols / 16) * kKeyOperand;  // a chunk of the twiddle planes: [plane th, tl][16 column tiles][operand], 32 KB
constexpr int kKeyChunkA = 2 * (kKeyTile / 16) * kKeyOperand;  // a chunk of the tile's x: [plane xh, xl][2 row tiles][operand], 4 KB
static_assert(kKeyingPlaneBytes == (size_t)kKeyChunks * kKeyChunkB, "2 MB: both planes of the 4096 x 256 matrix (launch.h)");
static_assert(kBlockDec == 2 * kKeySeg && kTuneN == kKeySeg, "a block is two whole segments; bin j steps j entries of the 4096-entry table per sample");
static_assert(kKeyChunkB == 8 * kKeyThreads * 16 && kKeyTile * kKeyChunk == 8 * kKeyThreads, "a lane stages 8 x 16 bytes of the planes and 8 samples a chunk");

typedef int key_v4i __attribute__((ext_vector_type(4)));
typedef uint32_t key_v4u __attribute__((ext_vector_type(4)));

// The twiddle planes, once: 16 bytes of either plane per lane, in the layout keying_product_kernel reads
__global__ __launch_bounds__(256) void keying_planes_kernel(int8_t *__restrict__ planes)
{
	const uint32_t u = blockIdx.x * 256 + threadIdx.x;  // (chunk, column tile, lane)
	if (u >= (uint32_t)(kKeyChunks * (kKeyCols / 16) * 64))
		return;
	const uint32_t l = u & 63, n = (u >> 6) & 15, kc = u >> 10;
	const uint32_t j = (n >> 1) * 16 + (l & 15) + 1;
	const uint32_t quarter = (n & 1) ? kTuneN / 4 : 0;  // S[i] = C[i - 1024]
	uint32_t hi[4] = {}, lo[4] = {};
	for (uint32_t b = 0; b < 16; b++) {
		const uint32_t k = kc * kKeyChunk + 16 * (l >> 4) + b;
		const int T = kTuneCos[(j * k - quarter) & (kTuneN - 1)];
		hi[b >> 2] |= (uint32_t)(uint8_t)(T >> 8) << (8 * (b & 3));
		lo[b >> 2] |= (uint32_t)(uint8_t)((T & 255) - 128) << (8 * (b & 3));
	}
	uint4 *dst = reinterpret_cast<uint4 *>(planes + (size_t)kc * kKeyChunkB) + n * 64 + l;
	dst[0] = make_uint4(hi[0], hi[1], hi[2], hi[3]);
	dst[(kKeyCols / 16) * 64] = make_uint4(lo[0], lo[1], lo[2], lo[3]);
}

// The work list: { table entry, submit-relative first sample } of every whole segment of every run below max_runs, by stream, run
// and segment -- the order of the table --, and its length.  A stream's runs are disjoint, so the list holds at most 2 n_blocks
// entries a stream: `cap`.  One workgroup, a stream per lane and 256 streams a step: the lane counts its stream's segments, an
// exclusive prefix sum over the workgroup (wave shuffles, then LDS) places them.
__global__ __launch_bounds__(256) void keying_list_kernel(const CaptureStage *__restrict__ stage, int stage_cap, const uint2 *__restrict__ cnt,
							  const uint4 *__restrict__ base, int n_streams, uint32_t max_runs, uint2 *__restrict__ work,
							  uint32_t cap, uint32_t *__restrict__ n_work)
{
	__shared__ uint32_t l_wave[4];
	const int t = threadIdx.x, lane = t & 63, w = t >> 6;
	uint32_t placed = 0;  // of the streams before this step
	for (int s0 = 0; s0 < n_streams; s0 += 256) {
		const int s = s0 + t;
		const CaptureStage *srow = stage + (size_t)(s < n_streams ? s : 0) * stage_cap;
		const int nr = s < n_streams ? (int)cnt[s].x : 0;
		const unsigned long long e0 = s < n_streams ? base[s].x : 0;
		uint32_t c = 0;
		for (int k = 0; k < nr && e0 + (unsigned)k < max_runs; k++) {
			const int q0 = (srow[k].start + kKeySeg - 1) / kKeySeg, q1 = srow[k].end / kKeySeg;
			c += q1 > q0 ? (uint32_t)(q1 - q0) : 0u;
		}
		uint32_t x = c;
#pragma unroll
		for (int d = 1; d < 64; d <<= 1) {
			const uint32_t o = (uint32_t)__shfl_up((int)x, d);
			if (lane >= d)
				x += o;
		}
		__syncthreads();  // (the step before has read l_wave)
		if (lane == 63)
			l_wave[w] = x;
		__syncthreads();
		uint32_t at = placed + x - c;
		for (int i = 0; i < 4; i++) {
			at += i < w ? l_wave[i] : 0u;
			placed += l_wave[i];
		}
		for (int k = 0; k < nr && e0 + (unsigned)k < max_runs; k++) {
			const int q0 = (srow[k].start + kKeySeg - 1) / kKeySeg, q1 = srow[k].end / kKeySeg;
			for (int q = q0; q < q1; q++, at++)
				if (at < cap)
					work[at] = make_uint2((uint32_t)(e0 + (unsigned)k), (uint32_t)(q * kKeySeg));
		}
	}
	if (t == 0)
		*n_work = placed < cap ? placed : cap;
}

// Tile blockIdx.x of the work list: its H = 32 segments are the rows of one matrix product against the twiddle planes.
//   1. mx of every segment: a wave per segment, 8 segments a wave, 16 samples per lane and step, the maximum over the wave by shuffles
//      and into LDS with sh and the row's source.  A row behind the list's end, and a silent segment, is staged as zeros.
//   2. 64 steps of 64 samples.  Lane t stages 8 samples of row t >> 3: x = amp >> sh, split into xh and xl at the A operand's place in
//      LDS (row tile, lane = row & 15 + 16 (k >> 4), byte k & 15), and sums x; and 8 x 16 bytes of the planes' chunk, which is laid
//      out as the B operand wants it: a plain copy, global memory to LDS, and one contiguous 16-byte read per lane and operand in the
//      product loop.  All four waves read the chunk from LDS: the workgroup streams the planes once.  What the next step stages is
//      loaded into registers ahead of this step's 32 instructions.  Wave w keeps 32 accumulators: its row tile x 8 column tiles x the
//      four plane products.
//   3. lane (column c, rows 4 g .. 4 g + 3) holds X_re and X_im of bin 64 (w & 1) + 16 u + c + 1 for u = 0 .. 3 in the same registers'
//      places: the five terms in int64, P = (X_re >> 17)^2 + (X_im >> 17)^2, one 64-bit atomic per (segment, bin) where P != 0, and
//      one 32-bit atomic per segment for its count.
// Every loop and barrier is uniform over the workgroup.  No floating point.
__global__ __launch_bounds__(kKeyThreads) void keying_product_kernel(const uint32_t *__restrict__ dec, size_t dec_stride,
								      const uint2 *__restrict__ work, const uint32_t *__restrict__ n_work,
								      const int8_t *__restrict__ planes, tfrec_amd_clock *__restrict__ out)
{
	const uint32_t nw = *n_work, w0 = blockIdx.x * kKeyTile;
	if (w0 >= nw)
		return;
	const int t = threadIdx.x, lane = t & 63, w = t >> 6;
	__shared__ __attribute__((aligned(16))) int8_t l_b[kKeyChunkB];
	__shared__ __attribute__((aligned(16))) int8_t l_a[kKeyChunkA];
	__shared__ const uint32_t *l_src[kKeyTile];  // the segment's first pair; null: an empty row
	__shared__ uint32_t l_ent[kKeyTile], l_mx[kKeyTile];
	__shared__ int l_sum[kKeyTile];
	for (int i = 0; i < kKeyTile / 4; i++) {
		const int r = w + 4 * i;  // (wave-uniform)
		const uint32_t *src = nullptr;
		uint32_t e = 0, mx = 0;
		if (w0 + r < nw) {
			const uint2 we = work[w0 + r];
			e = we.x;
			src = dec + (size_t)out[e].stream * dec_stride + we.y;  // (the init kernel copied the entry's stream)
#pragma unroll 4
			for (int v = 0; v < kKeySeg / 256; v++) {
				const uint4 z = reinterpret_cast<const uint4 *>(src)[v * 64 + lane];
				const uint32_t zz[4] = { z.x, z.y, z.z, z.w };
#pragma unroll
				for (int p = 0; p < 4; p++) {
					const int I = (int16_t)(zz[p] & 0xffffu), Q = (int16_t)(zz[p] >> 16);
					const uint32_t amp = (uint32_t)(I < 0 ? -I : I) + (uint32_t)(Q < 0 ? -Q : Q);
					mx = amp > mx ? amp : mx;
				}
			}
#pragma unroll
			for (int d = 32; d >= 1; d >>= 1) {
				const uint32_t o = (uint32_t)__shfl_xor((int)mx, d);
				mx = o > mx ? o : mx;
			}
		}
		if (lane == 0) {
			l_src[r] = mx ? src : nullptr;
			l_ent[r] = e;
			l_mx[r] = mx;
		}
	}
	__syncthreads();
	const int row = t >> 3, sub = t & 7;  // this lane stages the samples [8 sub, 8 sub + 8) of every chunk of row `row`
	// (an empty or silent row reads the submit's first segment instead, which every submit has, and shifts it away: no branch in the loop)
	const uint32_t *src = l_src[row] ? l_src[row] : dec;
	const int bits = 32 - __clz((int)l_mx[row]);
	const int sh = !l_src[row] ? 31 : bits > 14 ? bits - 14 : 0;
	const int a_at = ((row >> 4) * 64 + (row & 15) + 16 * (sub >> 1)) * 16 + 8 * (sub & 1);  // in plane xh; xl: + kKeyChunkA / 2
	const int wm = w >> 1, wn = w & 1;
	key_v4i acc[8][4];  // [column tile][xh th, xh tl, xl th, xl tl]
#pragma unroll
	for (int n = 0; n < 8; n++)
#pragma unroll
		for (int p = 0; p < 4; p++)
			acc[n][p] = key_v4i{ 0, 0, 0, 0 };
	int sumx = 0;
	key_v4u pb[8], pa[2];
	const key_v4u *gb = reinterpret_cast<const key_v4u *>(planes) + t;
#pragma unroll
	for (int i = 0; i < 8; i++)
		pb[i] = gb[i * kKeyThreads];
	pa[0] = reinterpret_cast<const key_v4u *>(src + 8 * sub)[0];
	pa[1] = reinterpret_cast<const key_v4u *>(src + 8 * sub)[1];
	for (int kc = 0; kc < kKeyChunks; kc++) {
		__syncthreads();  // (the step before has read l_a and l_b)
#pragma unroll
		for (int i = 0; i < 8; i++)
			reinterpret_cast<key_v4u *>(l_b)[t + i * kKeyThreads] = pb[i];
		{
			const uint32_t z[8] = { pa[0].x, pa[0].y, pa[0].z, pa[0].w, pa[1].x, pa[1].y, pa[1].z, pa[1].w };
			uint32_t xh[2] = {}, xl[2] = {};
#pragma unroll
			for (int i = 0; i < 8; i++) {
				const int I = (int16_t)(z[i] & 0xffffu), Q = (int16_t)(z[i] >> 16);
				const uint32_t x = ((uint32_t)(I < 0 ? -I : I) + (uint32_t)(Q < 0 ? -Q : Q)) >> sh;  // (< 2^14)
				sumx += (int)x;
				xh[i >> 2] |= (x >> 7) << (8 * (i & 3));
				xl[i >> 2] |= (x & 127u) << (8 * (i & 3));
			}
			*reinterpret_cast<uint2 *>(l_a + a_at) = make_uint2(xh[0], xh[1]);
			*reinterpret_cast<uint2 *>(l_a + kKeyChunkA / 2 + a_at) = make_uint2(xl[0], xl[1]);
		}
		__syncthreads();
		{  // the next step's, in flight behind this step's products (the last step loads its own again)
			const int kn = kc + 1 < kKeyChunks ? kc + 1 : kc;
			const key_v4u *nb = gb + (size_t)kn * (kKeyChunkB / 16);
#pragma unroll
			for (int i = 0; i < 8; i++)
				pb[i] = nb[i * kKeyThreads];
			const key_v4u *na = reinterpret_cast<const key_v4u *>(src + kn * kKeyChunk + 8 * sub);
			pa[0] = na[0];
			pa[1] = na[1];
		}
		const key_v4i ah = reinterpret_cast<const key_v4i *>(l_a)[wm * 64 + lane];
		const key_v4i al = reinterpret_cast<const key_v4i *>(l_a + kKeyChunkA / 2)[wm * 64 + lane];
#pragma unroll
		for (int n = 0; n < 8; n++) {
			const key_v4i bh = reinterpret_cast<const key_v4i *>(l_b)[(wn * 8 + n) * 64 + lane];
			const key_v4i bl = reinterpret_cast<const key_v4i *>(l_b + kKeyChunkB / 2)[(wn * 8 + n) * 64 + lane];
			acc[n][0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ah, bh, acc[n][0], 0, 0, 0);
			acc[n][1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ah, bl, acc[n][1], 0, 0, 0);
			acc[n][2] = __builtin_amdgcn_mfma_i32_16x16x64_i8(al, bh, acc[n][2], 0, 0, 0);
			acc[n][3] = __builtin_amdgcn_mfma_i32_16x16x64_i8(al, bl, acc[n][3], 0, 0, 0);
		}
	}
	sumx += __shfl_xor(sumx, 1);  // the row's 8 lanes
	sumx += __shfl_xor(sumx, 2);
	sumx += __shfl_xor(sumx, 4);
	if (sub == 0)
		l_sum[row] = sumx;
	__syncthreads();
	// the instruction's result: register i of lane l is row 4 (l >> 4) + i, column l & 15 of the 16 x 16 tile
	const int col = lane & 15;
#pragma unroll
	for (int i = 0; i < 4; i++) {
		const int r = wm * 16 + 4 * (lane >> 4) + i;
		if (!l_src[r])
			continue;  // empty or silent: nothing to add
		tfrec_amd_clock *o = out + l_ent[r];
		const long long rank1 = 128LL * l_sum[r];
#pragma unroll
		for (int u = 0; u < 4; u++) {
			long long X[2];
#pragma unroll
			for (int part = 0; part < 2; part++) {
				const int n = 2 * u + part;
				X[part] = (long long)acc[n][0][i] * 32768 + (long long)acc[n][1][i] * 128 + (long long)acc[n][2][i] * 256 + (long long)acc[n][3][i] + rank1;
			}
			const long long re = X[0] >> kKeyShift, im = X[1] >> kKeyShift;  // (|.| < 2^24)
			const unsigned long long P = (unsigned long long)(re * re) + (unsigned long long)(im * im);
			if (P)
				atomicAdd(reinterpret_cast<unsigned long long *>(&o->spec[wn * 64 + u * 16 + col]), P);
		}
	}
	if (t < kKeyTile && w0 + t < nw)  // the counts: a lane per row of the tile
		atomicAdd(l_mx[t] ? &out[l_ent[t]].n_segments : &out[l_ent[t]].n_silent, 1u);
}

hipError_t launch_keying_planes(hipStream_t st, int8_t *planes)
{
	hipLaunchKernelGGL(keying_planes_kernel, dim3(kKeyChunks * (kKeyCols / 16) * 64 / 256), dim3(256), 0, st, planes);
	return hipGetLastError();
}

hipError_t launch_burst_keying(hipStream_t st, const FrontOut &o, const CaptureBufs &b, const KeyingBufs &k)
{
	const uint32_t cap = 2u * (uint32_t)o.n_blocks * (uint32_t)o.n_streams;  // (<= the buffer's: the context's largest submit)
	launch_run_records_init(st, b, k.recs, nullptr);
	hipLaunchKernelGGL(keying_list_kernel, dim3(1), dim3(256), 0, st, b.stage, b.stage_cap, b.cnt, b.base, o.n_streams, b.max_runs, k.work, cap,
			   k.n_work);
	hipLaunchKernelGGL(keying_product_kernel, dim3((cap + kKeyTile - 1) / kKeyTile), dim3(kKeyThreads), 0, st, o.dec, o.dec_stride, k.work, k.n_work,
			   k.planes, k.recs);
	return hipGetLastError();
}
