// tfrec_amd/csrc/formats.h -- sample formats of rate contexts and of the base rate, included by frontend.hip behind
// resample.h inside namespace tfrec.
//
// A format maps one stored component (I or Q; little-endian, interleaved I, Q) to x, the int16 value every stage is defined on,
// -8192 <= x <= 8191 (include/tfrec_amd.h: tfrec_amd_create_format the normative text, tfrec_amd/formats.py the CPU restatement):
//   U8   x = (u8 - 128) << 6              S8   x = s8 << 6
//   S16  x = s16 >> 2 (arithmetic)        F32  v = f * 8192 in fp32, x = clamp(rint(v), -8192, 8191), ties to even, NaN -> 0
//   * resample_fmt_kernel<FMT> is the resampling stage (resample.h) with the chunk load and the conversion to x in front: the
//     tile is staged into LDS as the int16 (I, Q) image, one dword per complex sample; a chunk of 8 complex samples is 16, 32 or
//     64 bytes of input; a tuned stream's samples (6g: chan[s].x = inc_in != 0) are rotated once while they are staged (mixer.h),
//     with the phase of their own n -- negative for a history sample -- and the history keeps the unrotated input; an untuned
//     stream of the launch comes out as an untuned launch makes it.  The taps run as fma(x', h / 65536, acc) on the 2^23 + 2^22
//     accumulator in round-toward-minus-infinity mode: |h| < 2^17, so h / 65536 is exact in fp32; the FMA rounds once after the
//     exact product and the accumulator is integer-valued, so each tap floors its own term; and every partial sum is at most
//     max_phi sum |h| * 11585 >> 16 <= 19137 (108260 at 769/768 and 1537/1536 is the largest sum |h| of any accepted rate, 108112
//     at 65/64 the largest with Q <= 64; the tune is refused where the bound reaches 32768), which keeps the accumulator in
//     [2^23, 2^24) and the int16 store from wrapping.
//     The history is 64 complex samples per stream: of canonical x (256 bytes; x = 0 after a start or restart) for S8, S16 and
//     F32, so one loop reads the history of those formats alike -- and the RAW 128 bytes (0x80 after a start or restart) for U8,
//     read through the format's own loader.  A U8 context runs this kernel only while a stream is tuned and resample_kernel
//     otherwise: both read and write that one history, so an untuned stream's survives the change in both directions.
//     The cosine table is staged, and its 8 KB of LDS asked for, only by a launch with a tuned stream.
//   * resample_stream_kernel<FMT> is the same stage for a rate whose table does not fit (rs_streamed: Q T > 3840, up to 360 KB at
//     15359/1536): the image is staged by the same code (rs_stage_tile), the taps stay in global memory.  Its table is uploaded in
//     VISIT ORDER and tap-major, as h / 65536: entry n Q + j holds tap n of the phase (j P) mod Q.  P is invertible mod Q, so that is
//     a permutation of the phases, and output m of a stream uses column m mod Q.  Lane `tid` of a workgroup of N makes the outputs
//     m0 + o N + tid, o < 8: for one tap and one o the lanes of a wave read 64 consecutive floats (wrapping once at Q at most)
//     -- a coalesced 256-byte load that the XCD's L2 (4 MiB) serves -- and write 64 consecutive outputs.  The FMAs, their order
//     and the accumulator are resample_fmt_kernel's, so the outputs are the same bits.
//   * ingest_kernel<FMT> (base rate, 1/1; never U8, whose rows the front end reads as they are) converts each stream's row into
//     the stage-0 buffer frontend_kernel<true, ...> reads.
constexpr int kFmtTailDw = 64;  // history per stream: 64 complex samples of x, one dword each (T - 1 <= 59 needed)
static_assert(kRsTail == 2 * kFmtTailDw, "the raw u8 history holds the same 64 samples");

// One fp32 component -> x in the low 16 bits.  None of this depends on the fp32 rounding mode the tap loop sets: a product with a
// power of two is exact (where it overflows, every mode gives a value beyond the clamp), v_rndne_f32 rounds to the nearest
// even whatever the mode field says, and max, min, the comparison and the conversion of an integer value below 2^14 are exact.
__device__ __forceinline__ uint32_t fmt_f32_x(float f)
{
	const float v = f * 8192.0f;
	const float r = fminf(fmaxf(__builtin_rintf(v), -8192.0f), 8191.0f);
	return (uint32_t)(v != v ? 0 : (int)r) & 0xffffu;
}

// 8 complex samples at src (16-byte aligned) -> x as 8 dwords, I in the low half and Q in the high one; X4: 4 x instead, the form
// mixer_rotate takes (what the 8-bit formats' permute makes anyway)
template <int FMT, bool X4 = false>
__device__ __forceinline__ void fmt_load8(const uint8_t *__restrict__ src, uint32_t (&o)[8])
{
	const uint4 *p = reinterpret_cast<const uint4 *>(src);
	if constexpr (FMT == kFmtU8 || FMT == kFmtS8) {
		constexpr uint32_t kFlip = FMT == kFmtU8 ? 0x80808080u : 0u;  // u8 - 128 as two's complement
		const uint4 v = p[0];
		const uint32_t w[4] = { v.x ^ kFlip, v.y ^ kFlip, v.z ^ kFlip, v.w ^ kFlip };
#pragma unroll
		for (int i = 0; i < 8; i++)  // (b << 8) >> 2 per half = b << 6
			o[i] = X4 ? mixer_b8(w[i / 2], i & 1) : mixer_x(mixer_b8(w[i / 2], i & 1));
	} else if constexpr (FMT == kFmtS16) {
		const uint4 a = p[0], b = p[1];
		const uint32_t w[8] = { a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w };
#pragma unroll
		for (int i = 0; i < 8; i++)
			o[i] = X4 ? w[i] & 0xfffcfffcu : mixer_x(w[i]);
	} else {
		static_assert(FMT == kFmtF32, "four formats");
#pragma unroll
		for (int k = 0; k < 4; k++) {
			const uint4 v = p[k];
			const uint32_t x0 = fmt_f32_x(__uint_as_float(v.x)) | (fmt_f32_x(__uint_as_float(v.y)) << 16);
			const uint32_t x1 = fmt_f32_x(__uint_as_float(v.z)) | (fmt_f32_x(__uint_as_float(v.w)) << 16);
			o[2 * k] = X4 ? mixer_x4(x0) : x0;
			o[2 * k + 1] = X4 ? mixer_x4(x1) : x1;
		}
	}
}

// `chan` (nullptr: stream s reads row s, nothing is tuned): {inc_in, phase of the submit's first input sample, input row, 0} per
// stream; `tuned`: a stream of the launch has inc_in != 0 and the launch's LDS holds the table.  The history: kFmtTailDw dwords of
// x per stream, or -- U8 -- kRsTail raw bytes.
//
// What a tile of tile_n = 8 blockDim.x outputs starts from: its first output m0, that output's phase, and the dword of the image
// at which sample i0(m0) - (T-1) sits
struct RsTile {
	long m0;
	unsigned phi0;
	int sh;
};

// Stages the tile's int16 image into `raw` (8 rs_raw_chunks(p, q, t, tile_n) dwords, the cosine table behind it), writes the
// stream's history for the next submit from the last tile, and ends in the workgroup's barrier.
template <int FMT>
__device__ __forceinline__ RsTile rs_stage_tile(uint32_t *raw, const uint8_t *__restrict__ iq, size_t stride, long n_in, int p, int q, int t,
						const uint8_t *__restrict__ tail_in, uint8_t *__restrict__ tail_out,
						const uint4 *__restrict__ chan, int tuned)
{
	constexpr int kBps = fmt_sample_bytes(FMT);
	constexpr bool kRawHist = FMT == kFmtU8;
	constexpr int kHistBps = kRawHist ? kBps : 4;  // bytes per complex sample of the history
	const int s = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x;
	const int nthreads = (int)blockDim.x, tile_n = kRsOut * (int)blockDim.x;
	const long m0 = (long)tile * tile_n;
	const uint8_t *src = iq + (size_t)(chan ? chan[s].z : (uint32_t)s) * stride;
	const uint8_t *hist = tail_in + (size_t)s * (kFmtTailDw * kHistBps);
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
		mixer_stage_table(ctab, tid, nthreads);
		__syncthreads();
	}
	// the chunk at sample `so` of the submit as x (or 4 x): it lies wholly in the history or wholly in the submit (both are multiples
	// of 8 samples); silence elsewhere
	auto chunk = [&](auto x4, long so, uint32_t (&o8)[8]) {
		constexpr bool kX4 = decltype(x4)::value;
		if (so >= 0 && so + 8 <= n_in) {
			fmt_load8<FMT, kX4>(src + (size_t)so * kBps, o8);
		} else if (so < 0 && so >= -kFmtTailDw) {
			const uint8_t *h = hist + (kFmtTailDw + so) * kHistBps;
			if constexpr (kRawHist) {
				fmt_load8<FMT, kX4>(h, o8);
			} else {
				const uint4 a = reinterpret_cast<const uint4 *>(h)[0], b = reinterpret_cast<const uint4 *>(h)[1];
				const uint32_t w[8] = { a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w };
#pragma unroll
				for (int i = 0; i < 8; i++)
					o8[i] = kX4 ? mixer_x4(w[i]) : w[i];
			}
		} else {
#pragma unroll
			for (int i = 0; i < 8; i++)
				o8[i] = 0u;
		}
	};
	for (int c = tid; c < nchunks; c += nthreads) {
		const long so = b0 + 8L * c;
		uint32_t o8[8];
		if (tinc != 0) {  // the chunk's first sample is input sample so of the submit
			chunk(std::true_type{}, so, o8);
			const uint32_t p0 = tph + (uint32_t)(int)so * tinc;
#pragma unroll
			for (int i = 0; i < 8; i++)
				o8[i] = mixer_rotate(ctab, o8[i], p0 + (uint32_t)i * tinc);
		} else {
			chunk(std::false_type{}, so, o8);
		}
		uint32_t *d = raw + 8 * c;
		reinterpret_cast<uint4 *>(d)[0] = make_uint4(o8[0], o8[1], o8[2], o8[3]);
		reinterpret_cast<uint4 *>(d)[1] = make_uint4(o8[4], o8[5], o8[6], o8[7]);
	}
	// history for the next submit: the last 64 complex samples of this one, unrotated (n_in >= 32768, a multiple of 8)
	if (tile == (int)gridDim.x - 1 && tid < kFmtTailDw / 8) {
		const uint8_t *last = src + (size_t)(n_in - kFmtTailDw + 8 * tid) * kBps;
		uint4 *d = reinterpret_cast<uint4 *>(tail_out + (size_t)s * (kFmtTailDw * kHistBps) + 8 * kHistBps * tid);
		if constexpr (kRawHist) {
			d[0] = *reinterpret_cast<const uint4 *>(last);
		} else {
			uint32_t o8[8];
			fmt_load8<FMT>(last, o8);
			d[0] = make_uint4(o8[0], o8[1], o8[2], o8[3]);
			d[1] = make_uint4(o8[4], o8[5], o8[6], o8[7]);
		}
	}
	__syncthreads();
	return RsTile{ m0, phi0, (int)(lo - b0) };
}

template <int FMT>
__global__ __launch_bounds__(kRsThreads) void resample_fmt_kernel(const uint8_t *__restrict__ iq, size_t stride, long n_in, int p, int q,
								  int t, const float *__restrict__ taps, const uint8_t *__restrict__ tail_in,
								  uint8_t *__restrict__ tail_out, uint32_t *__restrict__ out, size_t out_stride,
								  const uint4 *__restrict__ chan, int tuned)
{
	extern __shared__ __attribute__((aligned(16))) uint32_t fmt_lds[];
	float *htab = reinterpret_cast<float *>(fmt_lds);
	uint32_t *raw = fmt_lds + rs_taps_dw(q, t);
	typedef float f32x2 __attribute__((ext_vector_type(2)));
	const int s = blockIdx.y, tid = threadIdx.x;
	const int nthreads = (int)blockDim.x;
	__builtin_amdgcn_s_setreg(1 | (0 << 6) | (1 << 11), 2);  // fp32 rounding toward -inf (see frontend_kernel, stage 1)
	for (int i = tid; i < q * t; i += nthreads)
		htab[i] = taps[i] * (1.0f / 64.0f);  // (h / 1024 -> h / 65536: exact)
	const RsTile g = rs_stage_tile<FMT>(raw, iq, stride, n_in, p, q, t, tail_in, tail_out, chan, tuned);
	const long m0 = g.m0;
	const unsigned phi0 = g.phi0;
	// ---- the lane's outputs m0 + 8 tid + o: sample i0 - (T-1) + n is dword sh + (i0 - i00) + n of the image
	const int sh = g.sh;
	const unsigned ar = phi0 + (unsigned)(kRsOut * tid) * (unsigned)p;  // a - i00 Q of the lane's first output (<= kRsArMax)
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

// The stage for a rate whose table is streamed (rs_streamed(q, t)).  taps: [t][q] floats, h / 65536, column j the phase (j P) mod Q
// (capi_create.h: make_inputs uploads it so).  Everything else as resample_fmt_kernel; the LDS holds the image and the cosine table only.
template <int FMT>
__global__ __launch_bounds__(kRsThreads) void resample_stream_kernel(const uint8_t *__restrict__ iq, size_t stride, long n_in, int p, int q,
								     int t, const float *__restrict__ taps, const uint8_t *__restrict__ tail_in,
								     uint8_t *__restrict__ tail_out, uint32_t *__restrict__ out, size_t out_stride,
								     const uint4 *__restrict__ chan, int tuned)
{
	extern __shared__ __attribute__((aligned(16))) uint32_t rss_lds[];
	typedef float f32x2 __attribute__((ext_vector_type(2)));
	const int s = blockIdx.y, tid = threadIdx.x;
	const int nthreads = (int)blockDim.x;
	__builtin_amdgcn_s_setreg(1 | (0 << 6) | (1 << 11), 2);  // fp32 rounding toward -inf (see frontend_kernel, stage 1)
	const RsTile g = rs_stage_tile<FMT>(rss_lds, iq, stride, n_in, p, q, t, tail_in, tail_out, chan, tuned);
	// ---- the lane's outputs m = m0 + o nthreads + tid: a - i00 Q = phi0 + (m - m0) P (<= kRsArMax) gives i0 - i00, and m mod Q the column
	const unsigned col0 = (unsigned)((unsigned long long)g.m0 % (unsigned)q);
	const float kMagic = 12582912.0f;  // 2^23 + 2^22
	const uint32_t *xp[kRsOut];
	const float *hp[kRsOut];
	f32x2 acc[kRsOut];
#pragma unroll
	for (int o = 0; o < kRsOut; o++) {
		const unsigned k = (unsigned)(o * nthreads + tid);  // < 1024
		xp[o] = rss_lds + g.sh + (g.phi0 + k * (unsigned)p) / (unsigned)q;
		hp[o] = taps + (col0 + k) % (unsigned)q;
		acc[o] = f32x2{ kMagic, kMagic };
	}
#pragma unroll 2
	for (int n = 0; n < t; n++) {  // (T is even)
#pragma unroll
		for (int o = 0; o < kRsOut; o++) {
			const uint32_t w = xp[o][n];
			const f32x2 d = f32x2{ (float)(int)(int16_t)(w & 0xffffu), (float)((int)w >> 16) };  // exact
			const float hs = hp[o][n * q];
			acc[o] = __builtin_elementwise_fma(d, f32x2{ hs, hs }, acc[o]);
		}
	}
	uint32_t *dst = out + (size_t)s * out_stride + g.m0 + tid;
#pragma unroll
	for (int o = 0; o < kRsOut; o++)  // the int16 store: the low half of the accumulator's mantissa
		dst[o * nthreads] = (__float_as_uint(acc[o].x) & 0xffffu) | (__float_as_uint(acc[o].y) << 16);
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

// fmt -> f(std::integral_constant<int, fmt>{}); false: no such format (U8: only where the caller has a U8 instantiation)
template <bool U8, class F>
bool fmt_dispatch(int fmt, F f)
{
	switch (fmt) {
	case kFmtU8:
		if constexpr (U8)
			f(std::integral_constant<int, kFmtU8>{});
		return U8;
	case kFmtS8:
		f(std::integral_constant<int, kFmtS8>{});
		return true;
	case kFmtS16:
		f(std::integral_constant<int, kFmtS16>{});
		return true;
	case kFmtF32:
		f(std::integral_constant<int, kFmtF32>{});
		return true;
	}
	return false;
}

// ... and of a streamed launch: the image and the cosine table.  The half tile's image is at most 20.3 KB (15359/1536).
__host__ __device__ constexpr int rs_stream_lds(int p, int q, int t, int tile) { return 8 * rs_raw_chunks(p, q, t, tile) * 4 + 2 * kTuneN; }
static_assert(rs_stream_lds(10 * kRsQDiv - 1, kRsQDiv, kRsTMax, kRsTile / 2) <= kRsLdsMax, "the half tile serves the largest rate");

// The resampling stage.  rate.taps: [q][t] floats on the device, h / 1024 (rs_streamed(q, t): the table resample_stream_kernel reads);
// n_blocks is a multiple of rs_unit(q) (the caller checked), so n_blocks * 32768 * p is one of q.  The history is the format's (above).
// tuned: a stream has an input-rate tune (6g; chan != nullptr then).  A u8 context runs resample_kernel (resample.h) while no stream is
// tuned and the table is staged, and the format kernel's U8 instantiation otherwise, which reads and writes the same raw history --
// an untuned stream's survives the change of kernels around it in both directions.  The format kernels have one geometry per rate,
// tuned or not: half the tile where the image of a whole one and the cosine table exceed the LDS limit (resample.h).  A rate whose
// table is not staged follows the same rule with its own LDS (one kernel per format, tuned or not).
hipError_t launch_resample(hipStream_t st, int fmt, const uint8_t *iq, size_t stride, int n_streams, int n_blocks, const RateTable &rate,
			   History hist, uint32_t *out, size_t out_stride, const uint4 *chan, bool tuned)
{
	const int p = rate.p, q = rate.q, t = rate.t;
	const long n_out = (long)n_blocks * (TFREC_AMD_BLOCK_BYTES / 2);  // complex samples at 1.536 MS/s
	const long n_in = n_out * p / q;
	const bool streamed = rs_streamed(q, t);
	if (fmt == kFmtU8 && !tuned && !streamed) {
		const size_t lds = (size_t)(rs_taps_dw(q, t) + 4 * rs_raw_chunks(p, q, t)) * 4;
		hipLaunchKernelGGL(resample_kernel, dim3((unsigned)(n_out / kRsTile), n_streams), dim3(kRsThreads), lds, st, iq, stride, n_in, p, q,
				   t, rate.taps, hist.in, hist.out, out, out_stride, chan);
		return hipGetLastError();
	}
	if (tuned && !chan)
		return hipErrorInvalidValue;
	const auto lds_of = [&](int tile_n) { return streamed ? rs_stream_lds(p, q, t, tile_n) : rs_tuned_lds(p, q, t, tile_n); };
	const int tile = lds_of(kRsTile) <= kRsLdsMax ? kRsTile : kRsTile / 2;
	const size_t lds = (size_t)lds_of(tile) - (tuned ? 0 : 2 * kTuneN);
	const dim3 grid((unsigned)(n_out / tile), n_streams), block(tile / kRsOut);
	const bool known = fmt_dispatch<true>(fmt, [&](auto f) {
		if (streamed)
			hipLaunchKernelGGL(resample_stream_kernel<decltype(f)::value>, grid, block, lds, st, iq, stride, n_in, p, q, t, rate.taps, hist.in,
					   hist.out, out, out_stride, chan, tuned ? 1 : 0);
		else
			hipLaunchKernelGGL(resample_fmt_kernel<decltype(f)::value>, grid, block, lds, st, iq, stride, n_in, p, q, t, rate.taps, hist.in,
					   hist.out, out, out_stride, chan, tuned ? 1 : 0);
	});
	return known ? hipGetLastError() : hipErrorInvalidValue;
}

hipError_t launch_ingest(hipStream_t st, int fmt, const uint8_t *iq, size_t stride, int n_streams, int n_blocks, uint32_t *out,
			 size_t out_stride, const uint4 *chan)
{
	const long n_chunks = (long)n_blocks * (TFREC_AMD_BLOCK_BYTES / 2) / 8;
	const dim3 grid((unsigned)((n_chunks + kIngestThreads - 1) / kIngestThreads), n_streams), block(kIngestThreads);
	const bool known = fmt_dispatch<false>(fmt, [&](auto f) {
		hipLaunchKernelGGL(ingest_kernel<decltype(f)::value>, grid, block, 0, st, iq, stride, n_chunks, out, out_stride, chan);
	});
	return known ? hipGetLastError() : hipErrorInvalidValue;
}
