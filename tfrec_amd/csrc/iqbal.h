// tfrec_amd/csrc/iqbal.h -- the IQ balancer (tfrec_amd_create_iq, include/tfrec_amd.h the normative text; tfrec_amd/
// iqbal.py the CPU restatement), included by frontend.hip behind dcblock.h inside namespace tfrec.
//
// Three kernels on the front-end stream in the place of the DC blocker's three, over the rows a submit uses (n_in complex samples
// each, a multiple of 512: n_win = n_in / 512 windows).  They do the blocker's work too -- a context has the one set or the other:
//   * iq_sums_kernel<FMT>: a wave per window; a lane loads one chunk of 8 complex samples (fmt_load8) and adds x_I, x_Q, x_I^2, x_Q^2
//     and x_I x_Q (a lane's 8 squares fit int32, a wave's total does not: the three moments are reduced as int64); lane 0 writes
//     the five sums.  No atomics: a window has one writer.
//   * iq_estimate_kernel: a wave per row, two scans.  The first is dc_estimate_kernel's, statement for statement, on S_I and S_Q:
//     d[i] (dc_k == 0, a context without the blocker: d = 0 and no DC state is touched); the lane that has d[i] forms
//         A = M_II - 2 d_I S_I + 512 d_I^2,  B likewise,  C = M_IQ - d_I S_Q - d_Q S_I + 512 d_I d_Q
//     and stores the triple.  The second scan runs over the triples and the balancer's own ring of K triples by the same rule: with
//     E = [the ring's m triples || this submit's], SA[i] = sum(ring) + sum_{t <= i} (E[m + t] - (m + t - K >= 0 ? E[m + t - K] : 0)),
//     int64, in pieces of 64 with a carry; then (t, g) per window (iq_tg).  Each ring is written only behind its scan's last read
//     of it.  The triples are written and read back by the same wave: a barrier of the (one-wave) workgroup lies between.
//   * iq_apply_kernel<FMT>: a lane per chunk; x' = clamp(x - d), Q'' = clamp(((Q' 2^14 - t I' + 2^13) >> 14) g + 2^13 >> 14), stored
//     as int16 x'' << 2 into the set's corrected rows: the pre-stage then runs as that of an S16 context, as behind the DC blocker.
struct IqSums {  // a window's five raw sums (32 bytes)
	int si, sq;
	long long mii, mqq, miq;
};
struct IqMoments {  // a window's A, B, C
	long long a, b, c;
};
static_assert(sizeof(IqSums) == 32 && sizeof(IqMoments) == 24, "capi_ctx.h sizes the context's buffers by these (kIqSumsBytes, kIqMomentsBytes)");

template <int FMT>
__global__ __launch_bounds__(kDcThreads) void iq_sums_kernel(const uint8_t *__restrict__ iq, size_t stride, int n_win, IqSums *__restrict__ sums,
							     int win_stride)
{
	const int row = blockIdx.y, lane = threadIdx.x & 63;
	const int w = (int)blockIdx.x * (kDcThreads / 64) + ((int)threadIdx.x >> 6);
	if (w >= n_win)  // (uniform for the wave)
		return;
	uint32_t o8[8];
	fmt_load8<FMT>(iq + (size_t)row * stride + ((size_t)w * kDcWin + 8 * (size_t)lane) * fmt_sample_bytes(FMT), o8);
	int si = 0, sq = 0, ii = 0, qq = 0, iq2 = 0;
#pragma unroll
	for (int i = 0; i < 8; i++) {  // |x| <= 8192: a product is <= 2^26, eight of them <= 2^29
		const int xi = (int)(int16_t)(o8[i] & 0xffffu), xq = (int)o8[i] >> 16;
		si += xi;
		sq += xq;
		ii += xi * xi;
		qq += xq * xq;
		iq2 += xi * xq;
	}
	si = dc_wave_sum(si);
	sq = dc_wave_sum(sq);
	const long long mii = dc_wave_sum((long long)ii), mqq = dc_wave_sum((long long)qq), miq = dc_wave_sum((long long)iq2);
	if (lane == 0) {
		IqSums s;
		s.si = si;
		s.sq = sq;
		s.mii = mii;
		s.mqq = mqq;
		s.miq = miq;
		sums[(size_t)row * win_stride + w] = s;
	}
}

// floor(num / den), den > 0
__device__ __forceinline__ long long iq_floor_div(long long num, long long den)
{
	long long q = num / den;
	if (num % den < 0)
		q--;
	return q;
}

// floor(sqrt(d)), 0 <= d < 2^62: the double's square root is within a few units of it (d itself is rounded to 53 bits first), the
// two loops make it exact; (r + 1)^2 <= (2^31 + 2)^2 fits
__device__ __forceinline__ long long iq_isqrt(long long d)
{
	long long r = (long long)sqrt((double)d);
	while (r * r > d)
		r--;
	while ((r + 1) * (r + 1) <= d)
		r++;
	return r;
}

// (t, g) of a window's sums SA, SB, SC as {t, g} int16 pairs; the identity where a guard trips
__device__ __forceinline__ uint32_t iq_tg(long long sa, long long sb, long long sc)
{
	const uint32_t ident = 16384u << 16;
	const long long top = max(sa, sb);
	const int s = max(0, (top > 0 ? 64 - __clzll(top) : 0) - 31);
	const long long a = sa >> s, b = sb >> s, c = sc >> s;  // (an arithmetic shift: floor)
	const long long dd = a * b - c * c;
	if (a == 0 || dd <= 0)
		return ident;
	const long long r = iq_isqrt(dd);
	const long long t = iq_floor_div(c * 32768 + a, 2 * a), g = iq_floor_div(a * 32768 + r, 2 * r);
	if (t > 4096 || t < -4096 || g < 12288 || g > 20480)
		return ident;
	return ((uint32_t)(int)t & 0xffffu) | ((uint32_t)(int)g << 16);
}

// sums[row][win_stride]; the DC blocker's ring[row][dc_k], state[row] = { m, head } and d[row][win_stride] (dc_k == 0: none of
// them is read or written); the balancer's mom[row][win_stride], iq_ring[row][k], iq_state[row] = { m, head }, tg[row][win_stride]
__global__ __launch_bounds__(64) void iq_estimate_kernel(const IqSums *__restrict__ sums, int n_win, int win_stride, int dc_k, int2 *dc_ring,
							 int2 *dc_state, uint32_t *d, IqMoments *mom, int k, IqMoments *iq_ring, int2 *iq_state,
							 uint32_t *__restrict__ tg)
{
	const int row = blockIdx.x, lane = threadIdx.x;
	const IqSums *s = sums + (size_t)row * win_stride;
	IqMoments *mo = mom + (size_t)row * win_stride;
	// ---- the DC scan (dc_estimate_kernel's), and the triples
	{
		int m = 0, head = 0;
		int2 *r = nullptr;
		long long ai = 0, aq = 0;
		if (dc_k) {
			const int2 st = dc_state[row];
			m = st.x;
			head = st.y;
			r = dc_ring + (size_t)row * dc_k;
			for (int j = lane; j < m; j += 64) {
				const int2 v = r[j];
				ai += v.x;
				aq += v.y;
			}
			ai = dc_wave_sum(ai);
			aq = dc_wave_sum(aq);
		}
		for (int i0 = 0; i0 < n_win; i0 += 64) {
			const int i = i0 + lane;
			IqSums w = {};
			if (i < n_win)
				w = s[i];
			int vi = 0, vq = 0;
			if (dc_k) {
				long long di = 0, dq = 0;
				if (i < n_win) {
					di = w.si;
					dq = w.sq;
					if (m + i - dc_k >= 0) {  // the window that leaves the average: of this submit, or of the ring
						int2 o;
						if (i - dc_k >= 0)
							o = make_int2(s[i - dc_k].si, s[i - dc_k].sq);
						else
							o = r[(head + i) % dc_k];
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
					const int c = min(m + i + 1, dc_k);
					vi = dc_round_mean(ai + di, c);
					vq = dc_round_mean(aq + dq, c);
					d[(size_t)row * win_stride + i] = ((uint32_t)vi & 0xffffu) | ((uint32_t)vq << 16);
				}
				ai += __shfl(di, 63, 64);
				aq += __shfl(dq, 63, 64);
			}
			if (i < n_win) {
				IqMoments v;
				v.a = w.mii - 2LL * vi * w.si + (long long)kDcWin * vi * vi;
				v.b = w.mqq - 2LL * vq * w.sq + (long long)kDcWin * vq * vq;
				v.c = w.miq - (long long)vi * w.sq - (long long)vq * w.si + (long long)kDcWin * vi * vq;
				mo[i] = v;
			}
		}
		if (dc_k) {  // the ring behind the submit: its last min(n_win, K) sums
			for (int i = max(0, n_win - dc_k) + lane; i < n_win; i += 64)
				r[(head + i) % dc_k] = make_int2(s[i].si, s[i].sq);
			if (lane == 0)
				dc_state[row] = make_int2(min(m + n_win, dc_k), (head + n_win % dc_k) % dc_k);
		}
	}
	__syncthreads();  // the triples: written above by one lane, read below by others of the same wave
	// ---- the balancer's scan
	const int2 st = iq_state[row];
	const int m = st.x, head = st.y;
	IqMoments *r = iq_ring + (size_t)row * k;
	long long sa = 0, sb = 0, sc = 0;
	for (int j = lane; j < m; j += 64) {
		const IqMoments v = r[j];
		sa += v.a;
		sb += v.b;
		sc += v.c;
	}
	sa = dc_wave_sum(sa);
	sb = dc_wave_sum(sb);
	sc = dc_wave_sum(sc);
	for (int i0 = 0; i0 < n_win; i0 += 64) {
		const int i = i0 + lane;
		long long da = 0, db = 0, dc = 0;
		if (i < n_win) {
			const IqMoments v = mo[i];
			da = v.a;
			db = v.b;
			dc = v.c;
			if (m + i - k >= 0) {
				const IqMoments o = i - k >= 0 ? mo[i - k] : r[(head + i) % k];
				da -= o.a;
				db -= o.b;
				dc -= o.c;
			}
		}
#pragma unroll
		for (int sh = 1; sh < 64; sh <<= 1) {
			const long long ua = __shfl_up(da, sh, 64), ub = __shfl_up(db, sh, 64), uc = __shfl_up(dc, sh, 64);
			if (lane >= sh) {
				da += ua;
				db += ub;
				dc += uc;
			}
		}
		if (i < n_win)
			tg[(size_t)row * win_stride + i] = iq_tg(sa + da, sb + db, sc + dc);
		sa += __shfl(da, 63, 64);
		sb += __shfl(db, 63, 64);
		sc += __shfl(dc, 63, 64);
	}
	for (int i = max(0, n_win - k) + lane; i < n_win; i += 64)
		r[(head + i) % k] = mo[i];
	if (lane == 0)
		iq_state[row] = make_int2(min(m + n_win, k), (head + n_win % k) % k);
}

// d == nullptr: a context without the DC blocker
template <int FMT>
__global__ __launch_bounds__(kDcThreads) void iq_apply_kernel(const uint8_t *__restrict__ iq, size_t stride, long n_chunks,
							      const uint32_t *__restrict__ d, const uint32_t *__restrict__ tg, int win_stride,
							      uint8_t *__restrict__ out, size_t out_stride)
{
	const int row = blockIdx.y;
	const long c = (long)blockIdx.x * kDcThreads + threadIdx.x;
	if (c >= n_chunks)
		return;
	uint32_t o8[8];
	fmt_load8<FMT>(iq + (size_t)row * stride + (size_t)c * (8 * fmt_sample_bytes(FMT)), o8);
	const size_t w = (size_t)row * win_stride + (c / kDcChunks);
	const uint32_t dw = d ? d[w] : 0u, tw = tg[w];
	const int di = (int)(int16_t)(dw & 0xffffu), dq = (int)dw >> 16;
	const int t = (int)(int16_t)(tw & 0xffffu), g = (int)tw >> 16;
#pragma unroll
	for (int i = 0; i < 8; i++) {
		const int xi = min(max((int)(int16_t)(o8[i] & 0xffffu) - di, -8192), 8191);
		const int xq = min(max(((int)o8[i] >> 16) - dq, -8192), 8191);
		const int v = (xq * 16384 - t * xi + 8192) >> 14;  // |t xi| <= 2^25, |v| <= 10241
		const int yq = min(max((v * g + 8192) >> 14, -8192), 8191);  // |v g| < 2^28
		o8[i] = ((uint32_t)(xi * 4) & 0xffffu) | ((uint32_t)(yq * 4) << 16);
	}
	uint4 *dst = reinterpret_cast<uint4 *>(out + (size_t)row * out_stride + (size_t)c * 32);
	dst[0] = make_uint4(o8[0], o8[1], o8[2], o8[3]);
	dst[1] = make_uint4(o8[4], o8[5], o8[6], o8[7]);
}

// The three kernels over rows 0 .. n_rows - 1 of a submit of n_in samples per row (a multiple of 512).  sums, mom, the rings and
// the states are the context's (the front-end stream orders one submit's use of them behind the last one's); d, tg and out are the
// set's.  dc_k == 0: no DC blocker (dc_ring, dc_state and d are not used).
hipError_t launch_iq(hipStream_t st, int fmt, const uint8_t *iq, size_t stride, int n_rows, long n_in, void *sums, int win_stride, int dc_k,
		     int2 *dc_ring, int2 *dc_state, uint32_t *d, void *mom, int k, void *iq_ring, int2 *iq_state, uint32_t *tg, uint8_t *out,
		     size_t out_stride)
{
	if (n_in <= 0 || n_in % kDcWin != 0 || n_in / kDcWin > win_stride || n_rows < 1 || k < 1 || dc_k < 0)
		return hipErrorInvalidValue;
	const int n_win = (int)(n_in / kDcWin);
	const long n_chunks = n_in / 8;
	const dim3 gs((unsigned)((n_win + kDcThreads / 64 - 1) / (kDcThreads / 64)), n_rows);
	const dim3 ga((unsigned)((n_chunks + kDcThreads - 1) / kDcThreads), n_rows);
	IqSums *s5 = static_cast<IqSums *>(sums);
	bool known = fmt_dispatch<true>(fmt, [&](auto f) {
		hipLaunchKernelGGL(iq_sums_kernel<decltype(f)::value>, gs, dim3(kDcThreads), 0, st, iq, stride, n_win, s5, win_stride);
	});
	if (!known)
		return hipErrorInvalidValue;
	hipError_t e = hipGetLastError();
	if (e != hipSuccess)
		return e;
	hipLaunchKernelGGL(iq_estimate_kernel, dim3(n_rows), dim3(64), 0, st, s5, n_win, win_stride, dc_k, dc_ring, dc_state, d,
			   static_cast<IqMoments *>(mom), k, static_cast<IqMoments *>(iq_ring), iq_state, tg);
	e = hipGetLastError();
	if (e != hipSuccess)
		return e;
	const uint32_t *dd = dc_k ? d : nullptr;
	fmt_dispatch<true>(fmt, [&](auto f) {
		hipLaunchKernelGGL(iq_apply_kernel<decltype(f)::value>, ga, dim3(kDcThreads), 0, st, iq, stride, n_chunks, dd, tg, win_stride, out,
				   out_stride);
	});
	return hipGetLastError();
}
