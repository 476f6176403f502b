// tfrec_amd/csrc/dcblock.h -- the DC blocker (tfrec_amd_create_dc, include/tfrec_amd.h the normative text; tfrec_amd/
// dcblock.py the CPU restatement), included by frontend.hip behind formats.h inside namespace tfrec.
//
// Three kernels on the front-end stream, ahead of the pre-stage, over the rows a submit uses (n_in complex samples each, a multiple
// of 512: n_win = n_in / 512 windows):
//   * dc_sums_kernel<FMT>: a wave per window; a lane loads one chunk of 8 complex samples through the format's own loader
//     (fmt_load8), adds the two rails, the wave reduces, lane 0 writes {S_I, S_Q}.  No atomics: a window has one writer.
//   * dc_estimate_kernel: a wave per row.  The row's ring holds the sums of its last m = min(count, K) windows, window a in slot
//     a mod K (head = count mod K); with E = [those m sums || this submit's sums], the sum over the last c windows that end in the
//     submit's window i is
//         A[i] = sum(ring) + sum_{t <= i} (E[m + t] - (m + t - K >= 0 ? E[m + t - K] : 0)),
//     an int64 prefix scan in pieces of 64 with a carry; d[i] = floor((2 A + 512 c) / (1024 c)), c = min(m + i + 1, K).  The ring is
//     written only behind the scan's last read of it (one wave, program order; every value read has been consumed by then), so it
//     is updated in place, and a row the submit does not use is not touched.
//   * dc_apply_kernel<FMT>: a lane per chunk; x' = clamp(x - d, -8192, 8191) per rail, stored as int16 x' << 2 -- 4 bytes per complex
//     sample, an S16 row whose loader's >> 2 returns x' exactly: the pre-stage then runs as that of an S16 context.
constexpr int kDcWin = 512;         // L: complex samples per window
constexpr int kDcThreads = 256;     // dc_sums_kernel: four windows per workgroup; dc_apply_kernel: 256 chunks
constexpr int kDcChunks = kDcWin / 8;
static_assert(kDcChunks == 64, "a window is one wave's 64 chunks of 8 samples");

template <class T>
__device__ __forceinline__ T dc_wave_sum(T v)  // every lane gets the total
{
#pragma unroll
	for (int m = 32; m >= 1; m >>= 1)
		v += __shfl_xor(v, m, 64);
	return v;
}

template <int FMT>
__global__ __launch_bounds__(kDcThreads) void dc_sums_kernel(const uint8_t *__restrict__ iq, size_t stride, int n_win, int2 *__restrict__ sums,
							     int win_stride)
{
	const int row = blockIdx.y, lane = threadIdx.x & 63;
	const int w = (int)blockIdx.x * (kDcThreads / 64) + ((int)threadIdx.x >> 6);
	if (w >= n_win)  // (uniform for the wave)
		return;
	uint32_t o8[8];
	fmt_load8<FMT>(iq + (size_t)row * stride + ((size_t)w * kDcWin + 8 * (size_t)lane) * fmt_sample_bytes(FMT), o8);
	int si = 0, sq = 0;
#pragma unroll
	for (int i = 0; i < 8; i++) {
		si += (int)(int16_t)(o8[i] & 0xffffu);
		sq += (int)o8[i] >> 16;
	}
	si = dc_wave_sum(si);
	sq = dc_wave_sum(sq);
	if (lane == 0)
		sums[(size_t)row * win_stride + w] = make_int2(si, sq);
}

// floor((2 a + 512 c) / (1024 c)), c > 0
__device__ __forceinline__ int dc_round_mean(long long a, int c)
{
	const long long num = 2 * a + (long long)kDcWin * c, den = 2LL * kDcWin * c;
	long long q = num / den;
	if (num % den < 0)
		q--;  // (floor, not C's truncation)
	return (int)q;
}

// state[row] = { m, head }; ring[row][k]; d[row][win_stride] as {d_I, d_Q} int16 pairs
__global__ __launch_bounds__(64) void dc_estimate_kernel(const int2 *__restrict__ sums, int n_win, int win_stride, int k, int2 *ring,
							 int2 *__restrict__ state, uint32_t *__restrict__ d)
{
	const int row = blockIdx.x, lane = threadIdx.x;
	const int2 st = state[row];
	const int m = st.x, head = st.y;
	const int2 *s = sums + (size_t)row * win_stride;
	int2 *r = ring + (size_t)row * k;
	long long ai = 0, aq = 0;
	for (int j = lane; j < m; j += 64) {  // the valid slots are the first m: all of them once count >= K, slots 0 .. count - 1 before
		const int2 v = r[j];
		ai += v.x;
		aq += v.y;
	}
	ai = dc_wave_sum(ai);
	aq = dc_wave_sum(aq);
	for (int i0 = 0; i0 < n_win; i0 += 64) {
		const int i = i0 + lane;
		long long di = 0, dq = 0;
		if (i < n_win) {
			const int2 v = s[i];
			di = v.x;
			dq = v.y;
			if (m + i - k >= 0) {  // the window that leaves the average: of this submit, or window count + i - K in slot (head + i) mod K
				const int2 o = i - k >= 0 ? s[i - k] : r[(head + i) % k];
				di -= o.x;
				dq -= o.y;
			}
		}
#pragma unroll
		for (int sh = 1; sh < 64; sh <<= 1) {  // inclusive scan
			const long long ui = __shfl_up(di, sh, 64), uq = __shfl_up(dq, sh, 64);
			if (lane >= sh) {
				di += ui;
				dq += uq;
			}
		}
		if (i < n_win) {
			const int c = min(m + i + 1, k);
			const int vi = dc_round_mean(ai + di, c), vq = dc_round_mean(aq + dq, c);
			d[(size_t)row * win_stride + i] = ((uint32_t)vi & 0xffffu) | ((uint32_t)vq << 16);
		}
		ai += __shfl(di, 63, 64);
		aq += __shfl(dq, 63, 64);
	}
	// the ring behind the submit: its last min(n_win, K) sums, window count + i in slot (head + i) mod K
	for (int i = max(0, n_win - k) + lane; i < n_win; i += 64)
		r[(head + i) % k] = s[i];
	if (lane == 0)
		state[row] = make_int2(min(m + n_win, k), (head + n_win % k) % k);
}

template <int FMT>
__global__ __launch_bounds__(kDcThreads) void dc_apply_kernel(const uint8_t *__restrict__ iq, size_t stride, long n_chunks,
							      const uint32_t *__restrict__ d, int win_stride, uint8_t *__restrict__ out,
							      size_t out_stride)
{
	const int row = blockIdx.y;
	const long c = (long)blockIdx.x * kDcThreads + threadIdx.x;
	if (c >= n_chunks)
		return;
	uint32_t o8[8];
	fmt_load8<FMT>(iq + (size_t)row * stride + (size_t)c * (8 * fmt_sample_bytes(FMT)), o8);
	const uint32_t dw = d[(size_t)row * win_stride + (c / kDcChunks)];
	const int di = (int)(int16_t)(dw & 0xffffu), dq = (int)dw >> 16;
#pragma unroll
	for (int i = 0; i < 8; i++) {
		const int xi = min(max((int)(int16_t)(o8[i] & 0xffffu) - di, -8192), 8191);
		const int xq = min(max(((int)o8[i] >> 16) - dq, -8192), 8191);
		o8[i] = ((uint32_t)(xi * 4) & 0xffffu) | ((uint32_t)(xq * 4) << 16);
	}
	uint4 *dst = reinterpret_cast<uint4 *>(out + (size_t)row * out_stride + (size_t)c * 32);
	dst[0] = make_uint4(o8[0], o8[1], o8[2], o8[3]);
	dst[1] = make_uint4(o8[4], o8[5], o8[6], o8[7]);
}

// The three kernels over rows 0 .. n_rows - 1 of a submit of n_in samples per row (a multiple of 512).  sums, ring and state are the
// context's (the front-end stream orders one submit's use of them behind the last one's); d and out are the set's.
hipError_t launch_dc(hipStream_t st, int fmt, const uint8_t *iq, size_t stride, int n_rows, long n_in, int k, int2 *sums, int win_stride,
		     int2 *ring, int2 *state, uint32_t *d, uint8_t *out, size_t out_stride)
{
	if (n_in <= 0 || n_in % kDcWin != 0 || n_in / kDcWin > win_stride || n_rows < 1 || k < 1)
		return hipErrorInvalidValue;
	const int n_win = (int)(n_in / kDcWin);
	const long n_chunks = n_in / 8;
	const dim3 gs((unsigned)((n_win + kDcThreads / 64 - 1) / (kDcThreads / 64)), n_rows);
	const dim3 ga((unsigned)((n_chunks + kDcThreads - 1) / kDcThreads), n_rows);
	bool known = fmt_dispatch<true>(fmt, [&](auto f) {
		hipLaunchKernelGGL(dc_sums_kernel<decltype(f)::value>, gs, dim3(kDcThreads), 0, st, iq, stride, n_win, sums, win_stride);
	});
	if (!known)
		return hipErrorInvalidValue;
	hipError_t e = hipGetLastError();
	if (e != hipSuccess)
		return e;
	hipLaunchKernelGGL(dc_estimate_kernel, dim3(n_rows), dim3(64), 0, st, sums, n_win, win_stride, k, ring, state, d);
	e = hipGetLastError();
	if (e != hipSuccess)
		return e;
	fmt_dispatch<true>(fmt, [&](auto f) {
		hipLaunchKernelGGL(dc_apply_kernel<decltype(f)::value>, ga, dim3(kDcThreads), 0, st, iq, stride, n_chunks, d, win_stride, out,
				   out_stride);
	});
	return hipGetLastError();
}
