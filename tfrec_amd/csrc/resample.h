// tfrec_amd/csrc/resample.h -- the resampling pre-stage, included by frontend.hip inside namespace tfrec.
//
// u8 IQ at fs_in = 1536000 P / Q  ->  1.536 MS/s int16 (I, Q), the "stage 0" buffer frontend_kernel<true, ...> reads.  The
// reference has no such stage; like the 10:1 stage it is defined here in the reference's FIR style (tfrec_amd/resample.py is
// the CPU restatement, include/tfrec_amd.h: tfrec_amd_create_rate the normative text):
//   r = P / Q input samples per output sample, gcd(P, Q) = 1, Q <= 64 or Q | 1536, 1 < r < 10;  T = 2 ceil(3 r) <= 60 taps per phase
//   output m of a submit:  a = m P,  i0 = a div Q,  phi = a mod Q        (every submit begins at phase 0 on its first sample)
//   y0[m] = int16( sum_{n<T} ( x[i0 - (T-1) + n] * h[phi][n] ) >> 16 ),  x = (u8 - 128) << 6, the T - 1 samples before a
//   submit come from the previous one's tail (silence, u8 128, after a start or restart)
// so (x * h) >> 16 = ((u8 - 128) * h) >> 10: one fp32 FMA per tap in round-toward-minus-infinity mode on the 2^23 + 2^22
// accumulator, both rails per v_pk_fma_f32 (frontend_kernel, stage 1).  h has up to 17 bits: h / 1024 is exact in fp32, the
// FMA rounds once after the exact product, and sum |h| / 8 < 32768 (a rate is refused otherwise) keeps the accumulator in
// [2^23, 2^24) and the int16 store from wrapping.
//
// One 128-thread workgroup per tile of 1024 outputs of one stream, like decim10_kernel:
//   * the tap table [Q][T] (as h / 1024, at most 15 KB) and the tile's raw bytes -- from 16 bytes at or below its first
//     sample i0(m0) - (T-1) up to its last sample i0(m0 + 1023): at most 20.6 KB -- are staged into LDS with coalesced
//     16-byte loads; the chunks in front of a submit's first sample come from the stream's history.  The LDS is sized per
//     launch from P, Q and T (dynamic shared memory: 2.9 KB at 4/3, 3.9 KB at 25/16), so that the registers and not the
//     largest rate's 36 KB set the occupancy of a common rate;
//   * the tile's first output gets i0 and phi from one 64-bit division; a lane's first output is a 32-bit division away
//     from it (the offset is below 2^24: kRsArMax), and the lane steps (i0, phi) by (P div Q, P mod Q) from there;
//   * a lane makes kRsOut = 8 consecutive outputs, tap by tap: the eight FMAs of a tap go to eight accumulators.
// `chan` (nullptr: stream s reads row s): the {.., .., input row, ..} of tfrec_amd_map_streams, as decim10_kernel<true> reads it.
// resample_kernel is the kernel of a u8 context in which no stream has an input-rate tune (6g).  While one has, the context runs
// resample_fmt_kernel<kFmtU8> (formats.h) on the same raw history instead: it rotates the tuned streams as it stages them.
// These two stage the whole table, so they serve the rates with Q T <= kRsTableMax = 3840 taps (every Q <= 64, and 2.0, 2.5, 5 or
// 10 MS/s among the Q | 1536); a rate with a larger table -- up to 92160 taps at 15359/1536 -- runs resample_stream_kernel
// (formats.h) in every format, tuned or not, on the same histories.
constexpr int kRsOut = 8;                      // outputs per lane
constexpr int kRsTile = 1024;                  // outputs per workgroup
constexpr int kRsThreads = kRsTile / kRsOut;   // 128
constexpr int kRsTail = 128;                   // raw history per stream: 64 complex samples (T - 1 <= 59 needed), 16-byte multiple
// LDS of a launch, in dwords: the table, padded to a 16-byte multiple, then the image.  A tile's last sample is at most
// floor((Q - 1 + 1023 P) / Q) samples behind its first output's i0, T - 1 lie before it, and the 16-byte alignment of the
// first chunk adds at most 14 bytes.
__host__ __device__ constexpr int rs_taps_dw(int q, int t) { return (q * t + 3) & ~3; }
__host__ __device__ constexpr int rs_raw_chunks(int p, int q, int t, int tile = kRsTile) { return (2 * ((q - 1 + (tile - 1) * p) / q + t) + 14 + 15) / 16; }
static_assert((rs_taps_dw(kRsQMax, kRsTMax) + 4 * rs_raw_chunks(10 * kRsQMax - 1, kRsQMax, kRsTMax)) * 4 <= 48 * 1024, "fits the default LDS limit");
// (a staged table is at most kRsTableMax taps whatever Q, and an image at most that of r -> 10: the two bounds above and below hold
// for the staged rates with Q | 1536 too.)  The kernels' 32-bit products: a - i00 Q of any output of a tile, and Q T.
constexpr long kRsArMax = (long)kRsQDiv - 1 + (long)(kRsTile - 1) * (10 * kRsQDiv - 1);
static_assert(kRsArMax < (1L << 24) && (long)kRsQDiv * kRsTMax < (1L << 17), "P <= 15359, Q <= 1536: the tile's offsets and the table's size stay far inside int");
// ... and of the format-aware launch (formats.h: resample_fmt_kernel, which also is the tuned kernel of a u8 context): the table, the
// int16 image (8 dwords per chunk) and the cosine table.  Where that exceeds 48 KB with a tile of 1024 outputs (the large rates)
// the launch uses 64-thread workgroups and tiles of 512: at most 44.3 KB (639/64), so no rate needs more than the default LDS limit.
constexpr int kRsLdsMax = 48 * 1024;
__host__ __device__ constexpr int rs_tuned_lds(int p, int q, int t, int tile) { return (rs_taps_dw(q, t) + 8 * rs_raw_chunks(p, q, t, tile)) * 4 + 2 * kTuneN; }
static_assert(rs_tuned_lds(10 * kRsQMax - 1, kRsQMax, kRsTMax, kRsTile / 2) <= kRsLdsMax, "the half tile serves the largest rate");

__global__ __launch_bounds__(kRsThreads) void resample_kernel(const uint8_t *__restrict__ iq, size_t stride, long n_in, int p, int q,
							      int t, const float *__restrict__ taps, const uint8_t *__restrict__ tail_in,
							      uint8_t *__restrict__ tail_out, uint32_t *__restrict__ out, size_t out_stride,
							      const uint4 *__restrict__ chan)
{
	extern __shared__ __attribute__((aligned(16))) uint32_t rs_lds[];
	float *htab = reinterpret_cast<float *>(rs_lds);
	uint32_t *raw = rs_lds + rs_taps_dw(q, t);
	typedef float f32x2 __attribute__((ext_vector_type(2)));
	const int s = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x;
	const int nthreads = kRsThreads, tile_n = kRsTile;
	__builtin_amdgcn_s_setreg(1 | (0 << 6) | (1 << 11), 2);  // fp32 rounding toward -inf (see frontend_kernel, stage 1)
	const long m0 = (long)tile * tile_n;
	const long nbytes = 2 * n_in;
	const uint8_t *src = iq + (size_t)(chan ? chan[s].z : (uint32_t)s) * stride;
	for (int i = tid; i < q * t; i += nthreads)
		htab[i] = taps[i];
	// ---- the tile's first output: a = m0 P in 64 bits
	const unsigned long long a0 = (unsigned long long)m0 * (unsigned)p;
	const long i00 = (long)(a0 / (unsigned)q);
	const unsigned phi0 = (unsigned)(a0 % (unsigned)q);
	const long lo = i00 - (t - 1);    // the first sample the tile reads (negative: history)
	const long b0 = (2 * lo) & ~15L;  // ... and the 16-byte boundary at or below it
	const long hi = i00 + (long)((phi0 + (unsigned)(tile_n - 1) * (unsigned)p) / (unsigned)q);  // its last sample: i0(m0 + 1023) < n_in
	const int nchunks = min((int)((2 * (hi + 1) - b0 + 15) >> 4), rs_raw_chunks(p, q, t, tile_n));
	for (int c = tid; c < nchunks; c += nthreads) {
		const long bo = b0 + 16L * c;  // a chunk lies wholly in the history or wholly in the submit (both are 16-byte multiples)
		uint4 v = make_uint4(0x80808080u, 0x80808080u, 0x80808080u, 0x80808080u);
		if (bo >= 0 && bo + 16 <= nbytes)
			v = *reinterpret_cast<const uint4 *>(src + bo);
		else if (bo < 0 && bo >= -kRsTail)
			v = *reinterpret_cast<const uint4 *>(tail_in + (size_t)s * kRsTail + (kRsTail + bo));
		*reinterpret_cast<uint4 *>(raw + 4 * c) = v;
	}
	// history for the next submit: the last 64 raw complex samples of this one (n_in >= 32768)
	if (tile == (int)gridDim.x - 1 && tid < kRsTail / 16)
		*reinterpret_cast<uint4 *>(tail_out + (size_t)s * kRsTail + 16 * tid) =
			*reinterpret_cast<const uint4 *>(src + nbytes - kRsTail + 16 * tid);
	__syncthreads();
	// ---- the lane's outputs m0 + 8 tid + o: sample i0 - (T-1) + n sits at byte sh + 2 (i0 - i00) + 2 n of the image
	const int sh = (int)(2 * lo - b0);
	const unsigned ar = phi0 + (unsigned)(kRsOut * tid) * (unsigned)p;  // a - i00 Q of the lane's first output, < 2^20
	unsigned di = ar / (unsigned)q, phi = ar % (unsigned)q;
	const unsigned pq = (unsigned)p / (unsigned)q, pr = (unsigned)p % (unsigned)q;
	const uint8_t *rb = reinterpret_cast<const uint8_t *>(raw);
	const float kMagic = 12582912.0f;  // 2^23 + 2^22
	const uint8_t *xp[kRsOut];
	const float *hp[kRsOut];
	f32x2 acc[kRsOut];
#pragma unroll
	for (int o = 0; o < kRsOut; o++) {
		xp[o] = rb + sh + 2 * di;
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
			const uint32_t w = *reinterpret_cast<const uint16_t *>(xp[o] + 2 * n);
			const f32x2 d = f32x2{ (float)(w & 0xffu), (float)(w >> 8) } - f32x2{ 128.0f, 128.0f };  // exact
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

static_assert((TFREC_AMD_BLOCK_BYTES / 2) % kRsTile == 0, "resample_kernel has no partial tiles");
// launch_resample (formats.h) launches it
