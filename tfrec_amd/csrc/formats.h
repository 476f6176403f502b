// tfrec_amd/csrc/formats.h -- sample formats of rate contexts and of the base rate, included by frontend.hip behind
// resample.h inside namespace tfrec.
//
// A format maps one stored component (I or Q; little-endian, interleaved I, Q) to x, the int16 value every stage is defined on,
// -8192 <= x <= 8191 (include/tfrec_amd.h: tfrec_amd_create_format the normative text, tfrec_amd/formats.py the CPU restatement):
//   S8   x = s8 << 6                      S16  x = s16 >> 2 (arithmetic)
//   F32  v = f * 8192 in fp32, x = clamp(rint(v), -8192, 8191), ties to even, NaN -> 0
// U8 never comes here: a U8 context is tfrec_amd_create_rate's or tfrec_amd_create's, with the kernels those launch.
//   * resample_fmt_kernel<FMT> is resample_kernel<true> (resample.h) with the chunk load and the conversion to x in front: the
//     tile is staged into LDS as the int16 (I, Q) image, one dword per complex sample; a chunk of 8 complex samples is 16, 32 or
//     64 bytes of input; a tuned stream's samples are rotated once while they are staged (4 x as the int16 halves, two
//     v_dot2_i32_i16, + 2^16 >> 17: |4 x| <= 32768, and |C| + |S| < 2^15.6 keeps the dot product in int32); the taps run as
//     fma(x', h / 65536, acc) on the 2^23 + 2^22 accumulator in round-toward-minus-infinity mode.  The history is 64 complex
//     samples per stream of canonical x (256 bytes; x = 0 after a start or restart), so one kernel reads the history of every
//     format alike.  The cosine table is staged, and its 8 KB of LDS asked for, only by a launch with a tuned stream.
//   * ingest_kernel<FMT> (base rate, 1/1) converts each stream's row into the stage-0 buffer frontend_kernel<true, ...> reads.
constexpr int kFmtU8 = 0, kFmtS8 = 1, kFmtS16 = 2, kFmtF32 = 3;
constexpr int kFmtTailDw = 64;  // history per stream: 64 complex samples of x, one dword each (T - 1 <= 59 needed)
__host__ __device__ constexpr int fmt_sample_bytes(int fmt) { return fmt == kFmtF32 ? 8 : fmt == kFmtS16 ? 4 : 2; }

// One fp32 component -> x in the low 16 bits.  None of this depends on the fp32 rounding mode the tap loop sets: a product with a
// power of two is exact (where it overflows, every mode gives a value beyond the clamp), v_rndne_f32 rounds to the nearest
// even whatever the mode field says, and max, min, the comparison and the conversion of an integer value below 2^14 are exact.
__device__ __forceinline__ uint32_t fmt_f32_x(float f)
{
	const float v = f * 8192.0f;
	const float r = fminf(fmaxf(__builtin_rintf(v), -8192.0f), 8191.0f);
	return (uint32_t)(v != v ? 0 : (int)r) & 0xffffu;
}

// 8 complex samples at src (16-byte aligned) -> x as 8 dwords, I in the low half and Q in the high one
template <int FMT>
__device__ __forceinline__ void fmt_load8(const uint8_t *__restrict__ src, uint32_t (&o)[8])
{
	const uint4 *p = reinterpret_cast<const uint4 *>(src);
	if constexpr (FMT == kFmtS8) {
		const uint4 v = p[0];
		const uint32_t w[4] = { v.x, v.y, v.z, v.w };
#pragma unroll
		for (int i = 0; i < 8; i++) {  // (b << 8) >> 2 per half = b << 6
			const uint32_t x4 = __builtin_amdgcn_perm(0u, w[i / 2], (i & 1) ? 0x030c020cu : 0x010c000cu);
			o[i] = ((uint32_t)((int)(int16_t)(x4 & 0xffffu) >> 2) & 0xffffu) | ((uint32_t)((int)x4 >> 18) << 16);
		}
	} else if constexpr (FMT == kFmtS16) {
		const uint4 a = p[0], b = p[1];
		const uint32_t w[8] = { a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w };
#pragma unroll
		for (int i = 0; i < 8; i++)
			o[i] = ((uint32_t)((int)(int16_t)(w[i] & 0xffffu) >> 2) & 0xffffu) | ((uint32_t)((int)w[i] >> 18) << 16);
	} else {
		static_assert(FMT == kFmtF32, "U8 has kernels of its own");
#pragma unroll
		for (int k = 0; k < 4; k++) {
			const uint4 v = p[k];
			o[2 * k] = fmt_f32_x(__uint_as_float(v.x)) | (fmt_f32_x(__uint_as_float(v.y)) << 16);
			o[2 * k + 1] = fmt_f32_x(__uint_as_float(v.z)) | (fmt_f32_x(__uint_as_float(v.w)) << 16);
		}
	}
}

// `chan` (nullptr: stream s reads row s, nothing is tuned): {inc_in, phase of the submit's first input sample, input row, 0} per
// stream, as resample_kernel<true> reads it; `tuned`: a stream of the launch has inc_in != 0 and the launch's LDS holds the table.
template <int FMT>
__global__ __launch_bounds__(kRsThreads) void resample_fmt_kernel(const uint8_t *__restrict__ iq, size_t stride, long n_in, int p, int q,
								  int t, const float *__restrict__ taps, const uint32_t *__restrict__ tail_in,
								  uint32_t *__restrict__ tail_out, uint32_t *__restrict__ out, size_t out_stride,
								  const uint4 *__restrict__ chan, int tuned)
{
	constexpr int kBps = fmt_sample_bytes(FMT);
	extern __shared__ __attribute__((aligned(16))) uint32_t fmt_lds[];
	float *htab = reinterpret_cast<float *>(fmt_lds);
	uint32_t *raw = fmt_lds + rs_taps_dw(q, t);
	typedef float f32x2 __attribute__((ext_vector_type(2)));
	typedef short s16x2 __attribute__((ext_vector_type(2)));
	const int s = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x;
	const int nthreads = (int)blockDim.x, tile_n = kRsOut * (int)blockDim.x;
	__builtin_amdgcn_s_setreg(1 | (0 << 6) | (1 << 11), 2);  // fp32 rounding toward -inf (see frontend_kernel, stage 1)
	const long m0 = (long)tile * tile_n;
	const uint8_t *src = iq + (size_t)(chan ? chan[s].z : (uint32_t)s) * stride;
	for (int i = tid; i < q * t; i += nthreads)
		htab[i] = taps[i] * (1.0f / 64.0f);  // (h / 1024 -> h / 65536: exact)
	// ---- the tile's first output: a = m0 P in 64 bits
	const unsigned long long a0 = (unsigned long long)m0 * (unsigned)p;
	const long i00 = (long)(a0 / (unsigned)q);
	const unsigned phi0 = (unsigned)(a0 % (unsigned)q);
	const long lo = i00 - (t - 1);  // the first sample the tile reads (negative: history)
	const long b0 = lo & ~7L;       // ... and the chunk boundary at or below it
	const long hi = i00 + (long)((phi0 + (unsigned)(tile_n - 1) * (unsigned)p) / (unsigned)q);  // its last sample: i0(m0 + tile_n - 1) < n_in
	const int nchunks = min((int)((hi + 1 - b0 + 7) >> 3), rs_raw_chunks(p, q, t, tile_n));
	const uint32_t tinc = (tuned && chan) ? chan[s].x : 0u, tph = chan ? chan[s].y : 0u;
	int16_t *ctab = reinterpret_cast<int16_t *>(raw + 8 * rs_raw_chunks(p, q, t, tile_n));
	if (tinc != 0) {  // (uniform for the workgroup)
		for (int i = tid; i < kTuneN / 2; i += nthreads)
			reinterpret_cast<uint32_t *>(ctab)[i] = (uint32_t)(uint16_t)kTuneCos[2 * i] | ((uint32_t)(uint16_t)kTuneCos[2 * i + 1] << 16);
		__syncthreads();
	}
	for (int c = tid; c < nchunks; c += nthreads) {
		const long so = b0 + 8L * c;  // a chunk lies wholly in the history or wholly in the submit (both are multiples of 8 samples)
		uint32_t o8[8] = { 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u };
		if (so >= 0 && so + 8 <= n_in) {
			fmt_load8<FMT>(src + (size_t)so * kBps, o8);
		} else if (so < 0 && so >= -kFmtTailDw) {
			const uint4 *h = reinterpret_cast<const uint4 *>(tail_in + (size_t)s * kFmtTailDw + (kFmtTailDw + so));
			const uint4 a = h[0], b = h[1];
			o8[0] = a.x, o8[1] = a.y, o8[2] = a.z, o8[3] = a.w, o8[4] = b.x, o8[5] = b.y, o8[6] = b.z, o8[7] = b.w;
		}
		if (tinc != 0) {  // the chunk's first sample is input sample so of the submit
			const uint32_t p0 = tph + (uint32_t)(int)so * tinc;
#pragma unroll
			for (int i = 0; i < 8; i++) {
				const uint32_t ph = p0 + (uint32_t)i * tinc;
				const uint32_t k = ph >> (32 - TFREC_TUNE_BITS);
				const int C = ctab[k], S = ctab[(k - kTuneN / 4) & (kTuneN - 1)];
				const uint32_t cs = ((uint32_t)C & 0xffffu) | ((uint32_t)S << 16);   // (C, S)
				const uint32_t sc = ((uint32_t)-S & 0xffffu) | ((uint32_t)C << 16);  // (-S, C)
				const uint32_t x4 = (o8[i] << 2) & 0xfffcfffcu;                      // (4 I, 4 Q)
				const int vi = __builtin_amdgcn_sdot2(__builtin_bit_cast(s16x2, x4), __builtin_bit_cast(s16x2, cs), 1 << 16, false) >> 17;
				const int vq = __builtin_amdgcn_sdot2(__builtin_bit_cast(s16x2, x4), __builtin_bit_cast(s16x2, sc), 1 << 16, false) >> 17;
				o8[i] = ((uint32_t)vi & 0xffffu) | ((uint32_t)vq << 16);
			}
		}
		uint32_t *d = raw + 8 * c;
		reinterpret_cast<uint4 *>(d)[0] = make_uint4(o8[0], o8[1], o8[2], o8[3]);
		reinterpret_cast<uint4 *>(d)[1] = make_uint4(o8[4], o8[5], o8[6], o8[7]);
	}
	// history for the next submit: the last 64 complex samples of this one as x, unrotated (n_in >= 32768, a multiple of 8)
	if (tile == (int)gridDim.x - 1 && tid < kFmtTailDw / 8) {
		uint32_t o8[8];
		fmt_load8<FMT>(src + (size_t)(n_in - kFmtTailDw + 8 * tid) * kBps, o8);
		uint4 *d = reinterpret_cast<uint4 *>(tail_out + (size_t)s * kFmtTailDw + 8 * tid);
		d[0] = make_uint4(o8[0], o8[1], o8[2], o8[3]);
		d[1] = make_uint4(o8[4], o8[5], o8[6], o8[7]);
	}
	__syncthreads();
	// ---- the lane's outputs m0 + 8 tid + o: sample i0 - (T-1) + n is dword sh + (i0 - i00) + n of the image
	const int sh = (int)(lo - b0);
	const unsigned ar = phi0 + (unsigned)(kRsOut * tid) * (unsigned)p;  // a - i00 Q of the lane's first output, < 2^20
	unsigned di = ar / (unsigned)q, phi = ar % (unsigned)q;
	const unsigned pq = (unsigned)p / (unsigned)q, pr = (unsigned)p % (unsigned)q;
	const float kMagic = 12582912.0f;  // 2^23 + 2^22
	const uint32_t *xp[kRsOut];
	const float *hp[kRsOut];
	f32x2 acc[kRsOut];
#pragma unroll
	for (int o = 0; o < kRsOut; o++) {
		xp[o] = raw + sh + di;
		hp[o] = htab + phi * (unsigned)t;
		acc[o] = f32x2{ kMagic, kMagic };
		phi += pr;
		di += pq;
		if (phi >= (unsigned)q) {
			phi -= (unsigned)q;
			di++;
		}
	}
#pragma unroll 2
	for (int n = 0; n < t; n++) {  // (T is even)
#pragma unroll
		for (int o = 0; o < kRsOut; o++) {
			const uint32_t w = xp[o][n];
			const f32x2 d = f32x2{ (float)(int)(int16_t)(w & 0xffffu), (float)((int)w >> 16) };  // exact
			const float hs = hp[o][n];
			acc[o] = __builtin_elementwise_fma(d, f32x2{ hs, hs }, acc[o]);
		}
	}
	uint32_t ow[kRsOut];
#pragma unroll
	for (int o = 0; o < kRsOut; o++)  // the int16 store: the low half of the accumulator's mantissa
		ow[o] = (__float_as_uint(acc[o].x) & 0xffffu) | (__float_as_uint(acc[o].y) << 16);
	uint4 *dst = reinterpret_cast<uint4 *>(out + (size_t)s * out_stride + m0 + kRsOut * tid);
#pragma unroll
	for (int k = 0; k < kRsOut / 4; k++)
		dst[k] = make_uint4(ow[4 * k], ow[4 * k + 1], ow[4 * k + 2], ow[4 * k + 3]);
}

// Base rate: chunk c (8 complex samples) of stream s's row -> dwords 8c .. 8c + 7 of the stream's stage-0 row.  `chan` as above
// (only the row is read: a 1/1 context has no input-rate tune).
constexpr int kIngestThreads = 256;
template <int FMT>
__global__ __launch_bounds__(kIngestThreads) void ingest_kernel(const uint8_t *__restrict__ iq, size_t stride, long n_chunks,
								uint32_t *__restrict__ out, size_t out_stride, const uint4 *__restrict__ chan)
{
	const int s = blockIdx.y;
	const long c = (long)blockIdx.x * kIngestThreads + threadIdx.x;
	if (c >= n_chunks)
		return;
	const uint8_t *src = iq + (size_t)(chan ? chan[s].z : (uint32_t)s) * stride;
	uint32_t o8[8];
	fmt_load8<FMT>(src + (size_t)c * (8 * fmt_sample_bytes(FMT)), o8);
	uint4 *d = reinterpret_cast<uint4 *>(out + (size_t)s * out_stride + 8 * c);
	d[0] = make_uint4(o8[0], o8[1], o8[2], o8[3]);
	d[1] = make_uint4(o8[4], o8[5], o8[6], o8[7]);
}

// fmt: kFmtS8, kFmtS16 or kFmtF32; the rest as launch_resample, with the history in dwords of x.  One geometry per rate, tuned
// or not: half the tile where the image of a whole one and the cosine table exceed the LDS limit (resample.h).
hipError_t launch_resample_fmt(hipStream_t st, int fmt, const uint8_t *iq, size_t stride, int n_streams, int n_blocks, int p, int q, int t,
			       const float *taps, const uint32_t *tail_in, uint32_t *tail_out, uint32_t *out, size_t out_stride,
			       const uint4 *chan, bool tuned)
{
	const long n_out = (long)n_blocks * (TFREC_AMD_BLOCK_BYTES / 2);  // complex samples at 1.536 MS/s
	const long n_in = n_out * p / q;
	if (tuned && !chan)
		return hipErrorInvalidValue;
	const int tile = rs_tuned_lds(p, q, t, kRsTile) <= kRsLdsMax ? kRsTile : kRsTile / 2;
	const size_t lds = (size_t)rs_tuned_lds(p, q, t, tile) - (tuned ? 0 : 2 * kTuneN);
	const dim3 grid((unsigned)(n_out / tile), n_streams), block(tile / kRsOut);
	const int tn = tuned ? 1 : 0;
	switch (fmt) {
	case kFmtS8:
		hipLaunchKernelGGL(resample_fmt_kernel<kFmtS8>, grid, block, lds, st, iq, stride, n_in, p, q, t, taps, tail_in, tail_out, out, out_stride, chan, tn);
		break;
	case kFmtS16:
		hipLaunchKernelGGL(resample_fmt_kernel<kFmtS16>, grid, block, lds, st, iq, stride, n_in, p, q, t, taps, tail_in, tail_out, out, out_stride, chan, tn);
		break;
	case kFmtF32:
		hipLaunchKernelGGL(resample_fmt_kernel<kFmtF32>, grid, block, lds, st, iq, stride, n_in, p, q, t, taps, tail_in, tail_out, out, out_stride, chan, tn);
		break;
	default:
		return hipErrorInvalidValue;
	}
	return hipGetLastError();
}

hipError_t launch_ingest(hipStream_t st, int fmt, const uint8_t *iq, size_t stride, int n_streams, int n_blocks, uint32_t *out,
			 size_t out_stride, const uint4 *chan)
{
	const long n_chunks = (long)n_blocks * (TFREC_AMD_BLOCK_BYTES / 2) / 8;
	const dim3 grid((unsigned)((n_chunks + kIngestThreads - 1) / kIngestThreads), n_streams), block(kIngestThreads);
	switch (fmt) {
	case kFmtS8:
		hipLaunchKernelGGL(ingest_kernel<kFmtS8>, grid, block, 0, st, iq, stride, n_chunks, out, out_stride, chan);
		break;
	case kFmtS16:
		hipLaunchKernelGGL(ingest_kernel<kFmtS16>, grid, block, 0, st, iq, stride, n_chunks, out, out_stride, chan);
		break;
	case kFmtF32:
		hipLaunchKernelGGL(ingest_kernel<kFmtF32>, grid, block, 0, st, iq, stride, n_chunks, out, out_stride, chan);
		break;
	default:
		return hipErrorInvalidValue;
	}
	return hipGetLastError();
}
