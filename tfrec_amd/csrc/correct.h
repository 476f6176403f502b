// tfrec_amd/csrc/correct.h -- the input correction: the DC blocker (tfrec_amd_create_dc, DESIGN.md 6m, tfrec_amd/dcblock.py the CPU
// restatement) and the IQ balancer (tfrec_amd_create_iq, DESIGN.md 6o, tfrec_amd/iqbal.py) as one stage; include/tfrec_amd.h is the
// normative text of both.  Included by frontend.hip behind formats.h inside namespace tfrec.
//
// Three kernels on the front-end stream, ahead of the pre-stage, over the rows a submit uses (n_in complex samples each, a multiple
// of 512: n_win = n_in / 512 windows), each a template over what the context has (DC: the blocker, IQ: the balancer; one at least):
//   * correct_sums_kernel<FMT, MOM>: a wave per window; a lane loads one chunk of 8 complex samples through the format's own loader
//     (fmt_load8), adds the two rails and -- MOM, the balancer -- x_I^2, x_Q^2 and x_I x_Q (a lane's 8 squares fit int32, a wave's
//     total does not: the three moments are reduced as int64); the wave reduces, lane 0 writes {S_I, S_Q} or the five sums.  No
//     atomics: a window has one writer.
//   * correct_estimate_kernel<DC, IQ>: a wave per row, one window_scan per estimator.  An estimator's ring holds the values of the
//     row's last m = min(count, K) windows, window a in slot a mod K (head = count mod K); with E = [those m values || this
//     submit's], the sum over the last c windows that end in the submit's window i is
//         A[i] = sum(ring) + sum_{t <= i} (E[m + t] - (m + t - K >= 0 ? E[m + t - K] : 0)),
//     an int64 prefix scan in pieces of 64 with a carry.  The blocker's values are the sums {S_I, S_Q}:
//     d[i] = floor((2 A + 512 c) / (1024 c)), c = min(m + i + 1, K) (no blocker: d = 0 and no DC state is touched).  The lane that
//     has d[i] forms
//         A = M_II - 2 d_I S_I + 512 d_I^2,  B likewise,  C = M_IQ - d_I S_Q - d_Q S_I + 512 d_I d_Q
//     and stores the triple; the balancer's values are those triples, its sums give (t, g) per window (iq_tg).  The triples are
//     written and read back by the same wave: a barrier of the (one-wave) workgroup lies between.
//   * correct_apply_kernel<FMT, DC, IQ>: a lane per chunk; x' = clamp(x - d, -8192, 8191) per rail, then -- IQ --
//     Q'' = clamp(((Q' 2^14 - t I' + 2^13) >> 14) g + 2^13 >> 14); stored as int16 x'' << 2 -- 4 bytes per complex sample, an S16 row
//     whose loader's >> 2 returns x'' exactly: the pre-stage then runs as that of an S16 context.
constexpr int kDcWin = 512;         // L: complex samples per window
constexpr int kDcThreads = 256;     // correct_sums_kernel: four windows per workgroup; correct_apply_kernel: 256 chunks
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

template <int FMT, bool MOM>
__global__ __launch_bounds__(kDcThreads) void correct_sums_kernel(const uint8_t *__restrict__ iq, size_t stride, int n_win,
								  std::conditional_t<MOM, IqSums, int2> *__restrict__ sums, int win_stride)
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
		if constexpr (MOM) {
			ii += xi * xi;
			qq += xq * xq;
			iq2 += xi * xq;
		}
	}
	si = dc_wave_sum(si);
	sq = dc_wave_sum(sq);
	if constexpr (MOM) {
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
	} else {
		if (lane == 0)
			sums[(size_t)row * win_stride + w] = make_int2(si, sq);
	}
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

// a ring element as its int64 components
__device__ __forceinline__ void win_vec(const int2 &e, long long (&v)[2])
{
	v[0] = e.x;
	v[1] = e.y;
}
__device__ __forceinline__ void win_vec(const IqMoments &e, long long (&v)[3])
{
	v[0] = e.a;
	v[1] = e.b;
	v[2] = e.c;
}

// The moving-window scan of one estimator over one row, by one wave: r is the row's ring of k elements of N components, state its
// {m, head}, win(i) the value of the submit's window i as a ring element.  The lane that owns window i gets emit(i, c, A): A the sum
// over the last c = min(m + i + 1, k) windows that end in i.  Then the submit's last min(n_win, k) values go into the ring, window
// count + i into slot (head + i) mod k, and the state follows.  The ring is written only behind the scan's last read of it (one
// wave, program order; every value read has been consumed by then), so it is updated in place.
template <int N, class T, class Win, class Emit>
__device__ __forceinline__ void window_scan(int n_win, int k, T *r, int2 *state, int lane, Win win, Emit emit)
{
	const int2 st = *state;
	const int m = st.x, head = st.y;
	long long a[N] = {};
	for (int j = lane; j < m; j += 64) {  // the valid slots are the first m: all of them once count >= K, slots 0 .. count - 1 before
		long long v[N];
		win_vec(r[j], v);
#pragma unroll
		for (int c = 0; c < N; c++)
			a[c] += v[c];
	}
#pragma unroll
	for (int c = 0; c < N; c++)
		a[c] = dc_wave_sum(a[c]);
	for (int i0 = 0; i0 < n_win; i0 += 64) {
		const int i = i0 + lane;
		long long d[N] = {};
		if (i < n_win) {
			win_vec(win(i), d);
			if (m + i - k >= 0) {  // the window that leaves the average: of this submit, or window count + i - K in slot (head + i) mod K
				long long o[N];
				win_vec(i - k >= 0 ? win(i - k) : r[(head + i) % k], o);
#pragma unroll
				for (int c = 0; c < N; c++)
					d[c] -= o[c];
			}
		}
#pragma unroll
		for (int sh = 1; sh < 64; sh <<= 1) {  // inclusive scan
			long long u[N];
#pragma unroll
			for (int c = 0; c < N; c++)
				u[c] = __shfl_up(d[c], sh, 64);
#pragma unroll
			for (int c = 0; c < N; c++)
				if (lane >= sh)
					d[c] += u[c];
		}
		if (i < n_win) {
			long long t[N];
#pragma unroll
			for (int c = 0; c < N; c++)
				t[c] = a[c] + d[c];
			emit(i, min(m + i + 1, k), t);
		}
#pragma unroll
		for (int c = 0; c < N; c++)
			a[c] += __shfl(d[c], 63, 64);
	}
	for (int i = max(0, n_win - k) + lane; i < n_win; i += 64)
		r[(head + i) % k] = win(i);
	if (lane == 0)
		*state = make_int2(min(m + n_win, k), (head + n_win % k) % k);
}

// sums[row][win_stride] ({S_I, S_Q}, or -- IQ -- the five sums); the blocker's ring[row][dc_k], state[row] = { m, head } and
// d[row][win_stride] as {d_I, d_Q} int16 pairs (not DC: none of them is read or written); the balancer's mom[row][win_stride],
// iq_ring[row][k], iq_state[row] and tg[row][win_stride] (not IQ: likewise).  A row the submit does not use is not touched.
template <bool DC, bool IQ>
__global__ __launch_bounds__(64) void correct_estimate_kernel(const std::conditional_t<IQ, IqSums, int2> *__restrict__ sums, int n_win,
							      int win_stride, int dc_k, int2 *dc_ring, int2 *__restrict__ dc_state,
							      uint32_t *__restrict__ d, IqMoments *mom, int k, IqMoments *iq_ring, int2 *iq_state,
							      uint32_t *__restrict__ tg)
{
	static_assert(DC || IQ, "a context without either stage launches none of the three kernels");
	const int row = blockIdx.x, lane = threadIdx.x;
	const auto *s = sums + (size_t)row * win_stride;
	// the blocker's estimate of window i from the sum A over its c windows: stored, and returned as {d_I, d_Q}
	[[maybe_unused]] auto put_d = [&](int i, int c, const long long(&a)[2]) {
		const int vi = dc_round_mean(a[0], c), vq = dc_round_mean(a[1], c);
		d[(size_t)row * win_stride + i] = ((uint32_t)vi & 0xffffu) | ((uint32_t)vq << 16);
		return make_int2(vi, vq);
	};
	[[maybe_unused]] int2 *dc_r = dc_ring + (size_t)row * dc_k;
	if constexpr (!IQ) {
		window_scan<2>(n_win, dc_k, dc_r, dc_state + row, lane, [&](int i) -> const int2 & { return s[i]; }, put_d);
	} else {
		IqMoments *mo = mom + (size_t)row * win_stride;
		auto triple = [&](int i, int2 v) {  // window i's A, B, C about the estimate v
			const IqSums w = s[i];
			IqMoments t;
			t.a = w.mii - 2LL * v.x * w.si + (long long)kDcWin * v.x * v.x;
			t.b = w.mqq - 2LL * v.y * w.sq + (long long)kDcWin * v.y * v.y;
			t.c = w.miq - (long long)v.x * w.sq - (long long)v.y * w.si + (long long)kDcWin * v.x * v.y;
			mo[i] = t;
		};
		if constexpr (DC) {
			window_scan<2>(
				n_win, dc_k, dc_r, dc_state + row, lane, [&](int i) { return make_int2(s[i].si, s[i].sq); },
				[&](int i, int c, const long long(&a)[2]) { triple(i, put_d(i, c, a)); });
		} else {
			for (int i = lane; i < n_win; i += 64)
				triple(i, make_int2(0, 0));
		}
		__syncthreads();  // the triples: written above by one lane, read below by others of the same wave
		window_scan<3>(
			n_win, k, iq_ring + (size_t)row * k, iq_state + row, lane, [&](int i) -> const IqMoments & { return mo[i]; },
			[&](int i, int, const long long(&a)[3]) { tg[(size_t)row * win_stride + i] = iq_tg(a[0], a[1], a[2]); });
	}
}

template <int FMT, bool DC, bool IQ>
__global__ __launch_bounds__(kDcThreads) void correct_apply_kernel(const uint8_t *__restrict__ iq, size_t stride, long n_chunks,
								   const uint32_t *__restrict__ d, int win_stride, uint8_t *__restrict__ out,
								   size_t out_stride, const uint32_t *__restrict__ tg)
{
	static_assert(DC || IQ, "a context without either stage launches none of the three kernels");
	const int row = blockIdx.y;
	const long c = (long)blockIdx.x * kDcThreads + threadIdx.x;
	if (c >= n_chunks)
		return;
	uint32_t o8[8];
	fmt_load8<FMT>(iq + (size_t)row * stride + (size_t)c * (8 * fmt_sample_bytes(FMT)), o8);
	const size_t w = (size_t)row * win_stride + (c / kDcChunks);
	uint32_t dw = 0u, tw = 0u;
	if constexpr (DC)
		dw = d[w];
	if constexpr (IQ)
		tw = tg[w];
	const int di = (int)(int16_t)(dw & 0xffffu), dq = (int)dw >> 16;
	[[maybe_unused]] const int t = (int)(int16_t)(tw & 0xffffu), g = (int)tw >> 16;
#pragma unroll
	for (int i = 0; i < 8; i++) {
		const int xi = min(max((int)(int16_t)(o8[i] & 0xffffu) - di, -8192), 8191);
		int xq = min(max(((int)o8[i] >> 16) - dq, -8192), 8191);
		if constexpr (IQ) {
			const int v = (xq * 16384 - t * xi + 8192) >> 14;  // |t xi| <= 2^25, |v| <= 10241
			xq = min(max((v * g + 8192) >> 14, -8192), 8191);  // |v g| < 2^28
		}
		o8[i] = ((uint32_t)(xi * 4) & 0xffffu) | ((uint32_t)(xq * 4) << 16);
	}
	uint4 *dst = reinterpret_cast<uint4 *>(out + (size_t)row * out_stride + (size_t)c * 32);
	dst[0] = make_uint4(o8[0], o8[1], o8[2], o8[3]);
	dst[1] = make_uint4(o8[4], o8[5], o8[6], o8[7]);
}

// The three kernels over rows 0 .. n_rows - 1 of a submit of n_in samples per row (a multiple of 512).  b (tfrec_dev.h): the
// context's sums, moments, rings and states (the front-end stream orders one submit's use of them behind the last one's) and the
// set's d, tg and out.
hipError_t launch_correct(hipStream_t st, int fmt, const uint8_t *iq, size_t stride, int n_rows, long n_in, const CorrectBufs &b)
{
	if (n_in <= 0 || n_in % kDcWin != 0 || n_in / kDcWin > b.win_stride || n_rows < 1 || b.dc_k < 0 || b.iq_k < 0 || (!b.dc_k && !b.iq_k))
		return hipErrorInvalidValue;
	const int n_win = (int)(n_in / kDcWin);
	const long n_chunks = n_in / 8;
	const dim3 gs((unsigned)((n_win + kDcThreads / 64 - 1) / (kDcThreads / 64)), n_rows);
	const dim3 ga((unsigned)((n_chunks + kDcThreads - 1) / kDcThreads), n_rows);
	// f(DC, IQ) with what the context has as constants
	auto stages = [&](auto f) {
		if (!b.iq_k)
			f(std::true_type{}, std::false_type{});
		else if (b.dc_k)
			f(std::true_type{}, std::true_type{});
		else
			f(std::false_type{}, std::true_type{});
	};
	bool known = fmt_dispatch<true>(fmt, [&](auto f) {
		if (b.iq_k)
			hipLaunchKernelGGL((correct_sums_kernel<decltype(f)::value, true>), gs, dim3(kDcThreads), 0, st, iq, stride, n_win, b.iq_sums,
					   b.win_stride);
		else
			hipLaunchKernelGGL((correct_sums_kernel<decltype(f)::value, false>), gs, dim3(kDcThreads), 0, st, iq, stride, n_win, b.dc_sums,
					   b.win_stride);
	});
	if (!known)
		return hipErrorInvalidValue;
	hipError_t e = hipGetLastError();
	if (e != hipSuccess)
		return e;
	stages([&](auto dc, auto iq_) {
		const auto *sums = [&] {
			if constexpr (decltype(iq_)::value)
				return b.iq_sums;
			else
				return b.dc_sums;
		}();
		hipLaunchKernelGGL((correct_estimate_kernel<decltype(dc)::value, decltype(iq_)::value>), dim3(n_rows), dim3(64), 0, st, sums, n_win,
				   b.win_stride, b.dc_k, b.dc_ring, b.dc_state, b.d, b.mom, b.iq_k, b.iq_ring, b.iq_state, b.tg);
	});
	e = hipGetLastError();
	if (e != hipSuccess)
		return e;
	fmt_dispatch<true>(fmt, [&](auto f) {
		stages([&](auto dc, auto iq_) {
			hipLaunchKernelGGL((correct_apply_kernel<decltype(f)::value, decltype(dc)::value, decltype(iq_)::value>), ga, dim3(kDcThreads), 0,
					   st, iq, stride, n_chunks, b.d, b.win_stride, b.out, b.out_stride, b.tg);
		});
	});
	return hipGetLastError();
}
