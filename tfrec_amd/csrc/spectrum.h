// tfrec_amd/csrc/spectrum.h -- the per-input power spectrum (tfrec_amd_enable_spectrum, include/tfrec_amd.h the normative text;
// DESIGN.md 6k): an exact integer DFT of the submit's raw input rows, per record of G frames the sum and the peak hold of every
// bin's power.  One kernel, on a low-priority stream of its own, ordered behind the producer of the input only: it reads the rows
// through the format's own loader (formats.h: fmt_load8) and depends on nothing the pipeline produces.  Included by frontend.hip
// (inside namespace tfrec) behind formats.h.  tfrec_amd/spectrum.py restates it.
//
// A submit is (frames x N windowed samples) times the fixed (N x N) twiddle matrix.  A workgroup owns one (row, record, tile of
// up to 256 bins) and walks the record's frames kSpecFrames at a time:
//   * the N-entry twiddle table W[j] = {(C, S), (-S, C)}[j * step] is staged once per workgroup (8 bytes per entry: at most 8 KB),
//     the window is read back from it: w[n] = (32767 - C[n * step]) >> 1;
//   * a batch of kSpecFrames frames is staged as xw = (x * w + 2^14) >> 15, one dword per complex sample (I low, Q high, |xw| <=
//     8192), sample-major: the kSpecFrames frames' values of one n lie side by side (32 bytes, two broadcast 16-byte LDS reads);
//   * a lane owns one bin k.  Per sample n it gathers W[(k n) mod N] once (8 bytes) and applies it to all kSpecFrames frames:
//     X_re += (xwI, xwQ) . (C, S), X_im += (xwI, xwQ) . (-S, C), one v_dot2_i32_i16 each.  A term is at most 8192 * (|C| + |S|)
//     <= 8192 * 46341 < 2^28.51 in magnitude, so FOUR terms chained through the instruction's int32 accumulator stay below
//     2^30.51; every fourth sample the int32 partials are added into int64 sums (|X| < 2^39 at N = 1024).  Integer addition is
//     associative: the grouping cannot change a bit;
//   * per frame Y = (X + 2^14) >> 15 per component (int64, arithmetic), p = Y_re^2 + Y_im^2 < 2^49; the lane keeps the record's
//     sum and maximum of p in registers and writes them once: each (row, record, bin) has one writer, no atomic.
// Frames of a batch beyond the record's end are staged as zeros: X = 0, Y = 0, p = 0 adds nothing to the sum and cannot raise the
// maximum of non-negative values.  Nothing beyond frame F - 1 of the row is read.
#pragma once

constexpr int kSpecFrames = 8;       // frames per staged batch (the register tile: 16 int32 partials + 16 int64 sums per lane)
constexpr int kSpecMaxBins = 1024;   // n_bins is one of 64, 128, 256, 512, 1024
constexpr int kSpecThreads = 256;    // lanes per workgroup at most: min(N, 256), one bin each
constexpr int kSpecGroup = 4;        // terms chained in int32: 4 * 8192 * 46341 < 2^31
static_assert(4LL * 8192 * 46341 < (1LL << 31), "four terms fit the int32 accumulator");
static_assert(kSpecFrames == 8, "a sample's frames are read as two uint4");

// sum / peak: [rows][max_records][N]; nfr: [rows][max_records].  grid = (rows analysed x n_records, N / blockDim.x), block =
// min(N, 256).  n_frames: F = floor(n_in / N) of this submit; g: frames per record; n_records = ceil(F / g).
template <int FMT>
__global__ __launch_bounds__(kSpecThreads) void spectrum_kernel(const uint8_t *__restrict__ iq, size_t stride, int n_bins, int n_frames,
								int g, int n_records, size_t max_records, unsigned long long *__restrict__ sum,
								unsigned long long *__restrict__ peak, uint32_t *__restrict__ nfr)
{
	typedef short s16x2 __attribute__((ext_vector_type(2)));
	constexpr int kBps = fmt_sample_bytes(FMT);
	extern __shared__ __attribute__((aligned(16))) uint32_t spec_lds[];
	uint2 *tw = reinterpret_cast<uint2 *>(spec_lds);        // [N] {(C, S), (-S, C)}
	uint32_t *xs = spec_lds + 2 * n_bins;                    // [N][kSpecFrames] windowed samples
	const int tid = threadIdx.x, nthreads = (int)blockDim.x;
	const int row = (int)(blockIdx.x / (unsigned)n_records), rec = (int)(blockIdx.x - (unsigned)row * (unsigned)n_records);
	const int k = (int)blockIdx.y * nthreads + tid;          // this lane's bin (< N: N is a multiple of blockDim.x)
	const int step = kTuneN / n_bins, nmask = n_bins - 1;
	const int f0 = rec * g;                                  // the record's frames [f0, f0 + nf)
	const int nf = min(g, n_frames - f0);
	const uint8_t *src = iq + (size_t)row * stride;
	for (int j = tid; j < n_bins; j += nthreads) {
		const int t = j * step;
		const int C = kTuneCos[t], S = kTuneCos[(t - kTuneN / 4) & (kTuneN - 1)];
		tw[j] = make_uint2(((uint32_t)C & 0xffffu) | ((uint32_t)S << 16), ((uint32_t)-S & 0xffffu) | ((uint32_t)C << 16));
	}
	unsigned long long acc_sum = 0, acc_peak = 0;
	const int chunks = n_bins / 8;  // chunks of 8 complex samples per frame
	for (int fb = 0; fb < nf; fb += kSpecFrames) {
		__syncthreads();  // the table is staged / the batch before this one has been consumed
		for (int c = tid; c < chunks * kSpecFrames; c += nthreads) {
			const int fr = c / chunks, n0 = (c - fr * chunks) * 8;
			uint32_t o8[8];
			if (fb + fr < nf) {
				fmt_load8<FMT>(src + ((size_t)(f0 + fb + fr) * n_bins + n0) * kBps, o8);
#pragma unroll
				for (int i = 0; i < 8; i++) {
					const int w = (32767 - (int)(int16_t)(tw[n0 + i].x & 0xffffu)) >> 1;
					const int xi = (int)(int16_t)(o8[i] & 0xffffu), xq = (int)o8[i] >> 16;
					const int wi = (xi * w + (1 << 14)) >> 15, wq = (xq * w + (1 << 14)) >> 15;
					o8[i] = ((uint32_t)wi & 0xffffu) | ((uint32_t)wq << 16);
				}
			} else {
#pragma unroll
				for (int i = 0; i < 8; i++)
					o8[i] = 0u;
			}
#pragma unroll
			for (int i = 0; i < 8; i++)
				xs[(n0 + i) * kSpecFrames + fr] = o8[i];
		}
		__syncthreads();
		long long xre[kSpecFrames], xim[kSpecFrames];
#pragma unroll
		for (int f = 0; f < kSpecFrames; f++)
			xre[f] = xim[f] = 0;
		int j = 0;  // (k n) mod N
		for (int n = 0; n < n_bins; n += kSpecGroup) {
			int pre[kSpecFrames], pim[kSpecFrames];
#pragma unroll
			for (int f = 0; f < kSpecFrames; f++)
				pre[f] = pim[f] = 0;
#pragma unroll
			for (int u = 0; u < kSpecGroup; u++) {
				const uint2 w = tw[j];
				j = (j + k) & nmask;
				const uint4 a = reinterpret_cast<const uint4 *>(xs + (n + u) * kSpecFrames)[0];
				const uint4 b = reinterpret_cast<const uint4 *>(xs + (n + u) * kSpecFrames)[1];
				const uint32_t x[kSpecFrames] = { a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w };
				const s16x2 cs = __builtin_bit_cast(s16x2, w.x), sc = __builtin_bit_cast(s16x2, w.y);
#pragma unroll
				for (int f = 0; f < kSpecFrames; f++) {
					pre[f] = __builtin_amdgcn_sdot2(__builtin_bit_cast(s16x2, x[f]), cs, pre[f], false);
					pim[f] = __builtin_amdgcn_sdot2(__builtin_bit_cast(s16x2, x[f]), sc, pim[f], false);
				}
			}
#pragma unroll
			for (int f = 0; f < kSpecFrames; f++) {
				xre[f] += pre[f];
				xim[f] += pim[f];
			}
		}
#pragma unroll
		for (int f = 0; f < kSpecFrames; f++) {
			const long long yr = (xre[f] + (1 << 14)) >> 15, yi = (xim[f] + (1 << 14)) >> 15;
			const unsigned long long p = (unsigned long long)(yr * yr) + (unsigned long long)(yi * yi);
			acc_sum += p;
			acc_peak = p > acc_peak ? p : acc_peak;
		}
	}
	const size_t o = ((size_t)row * max_records + (size_t)rec) * (size_t)n_bins + (size_t)k;
	sum[o] = acc_sum;
	peak[o] = acc_peak;
	if (blockIdx.y == 0 && tid == 0)
		nfr[(size_t)row * max_records + (size_t)rec] = (uint32_t)nf;
}

// The spectrum of rows 0 .. n_rows - 1 of a submit of n_in complex samples per row.  n_records = ceil(floor(n_in / N) / g) must
// not exceed max_records (the caller sized the buffers from max_blocks).
hipError_t launch_spectrum(hipStream_t st, int fmt, const uint8_t *iq, size_t stride, const SpectrumBufs &b)
{
	const int n_rows = b.n_rows, n_bins = b.n_bins, g = b.g;
	const size_t max_records = b.max_records;
	const long n_frames = b.n_in / n_bins;
	const long n_records = (n_frames + g - 1) / g;
	if (n_bins < 64 || n_bins > kSpecMaxBins || (n_bins & (n_bins - 1)) || g < 1 || n_rows < 1 || n_frames > 0x7fffffffL ||
	    (size_t)n_records > max_records || n_records * n_rows > 0x7fffffffL)
		return hipErrorInvalidValue;
	if (n_records == 0)
		return hipSuccess;
	const int threads = std::min(n_bins, kSpecThreads);
	const dim3 grid((unsigned)(n_records * n_rows), (unsigned)(n_bins / threads)), block((unsigned)threads);
	const size_t lds = (size_t)n_bins * (8 + 4 * kSpecFrames);  // the table and one batch: 40 KB at N = 1024
	const bool known = fmt_dispatch<true>(fmt, [&](auto f) {
		hipLaunchKernelGGL(spectrum_kernel<decltype(f)::value>, grid, block, lds, st, iq, stride, n_bins, (int)n_frames, g, (int)n_records, max_records, b.sum,
				   b.peak, b.nfr);
	});
	return known ? hipGetLastError() : hipErrorInvalidValue;
}
