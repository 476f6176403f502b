// tfrec_amd/csrc/demod.h -- the burst demodulator (tfrec_amd_enable_burst_demod, include/tfrec_amd.h: tfrec_amd_demod): per
// run of the recorder's table one int16 soft decision per symbol -- the burst correlator's soft sample summed over each symbol, or
// the difference of a Manchester bit's two chips -- at a symbol timing measured on the chain's first piece.  capture.h's
// run_records_init_kernel, corr.h's corr_soft_kernel on this stage's own soft bytes and centre (the soft sample IS the correlator's:
// the same kernel, not a copy of it), demod_list_kernel, demod_timing_kernel, demod_symbol_kernel and demod_carry_kernel, on the
// recorder's low-priority lane behind the burst correlator's.  They read the recorder's table and working set, the decimated samples
// and prevdec, and the 384 soft bytes, A and p* they carried themselves.  Exact integers only.  Included by frontend.hip (inside
// namespace tfrec) behind corr.h.  tfrec_amd/demod.py restates the result.
//
// A symbol sum is a boxcar: the difference of two entries of the soft bytes' prefix sum.  Both heavy kernels stage soft bytes in
// LDS, turn them into an int32 prefix sum in place (a serial sum per lane over its own stretch, a wave scan of the lanes' sums, the
// waves' offsets through LDS) and read every decision as two or three entries of it.  The matrix instructions have no place here: a
// product would spend 384 multiply-adds on what two loads and a subtraction give.
#pragma once

static_assert(sizeof(tfrec_amd_demod) == 72 && offsetof(tfrec_amd_demod, phase) == 24 && offsetof(tfrec_amd_demod, n_symbols) == 36 &&
		      offsetof(tfrec_amd_demod, e_best) == 40 && offsetof(tfrec_amd_demod, first_symbol) == 56 && offsetof(tfrec_amd_demod, pool_offset) == 64,
	      "the init kernel copies a table entry's first 24 bytes and its pool_offset");
// run_records_init_kernel's rule -- the entry's first 24 bytes, its pool_offset in the last 8, zeros between (timing NONE)
template <>
__device__ inline uint32_t run_record_word<tfrec_amd_demod>(const uint32_t *src, int w)
{
	return w < 6 ? src[w] : w >= 16 ? src[w - 10] : 0u;
}

constexpr int kDemodThreads = 256;
constexpr int kDemodGrid = 2048;    // demod_timing_kernel's and demod_symbol_kernel's workgroups at the most: each walks its list in strides
constexpr int kDemodTile = 4096;    // samples per tile of demod_symbol_kernel
constexpr int kDemodSpan = 384;     // a decision's samples at the most, ceil(384000 / 1000): what a tile stages ahead of itself, and the carried bytes
constexpr int kDemodHead = 8192;    // the timing's decisions end within g(Nt) <= 8192 samples behind the phase
constexpr int kDemodTimed = 64;     // Nt at the most
constexpr int kDemodMinTimed = 8;   // fewer decisions than this: no timing
// a lane's stretch of the prefix sum is an odd number of dwords, so the 64 lanes of a wave walk 64 different banks
constexpr int kDemodTimingChunk = ((kDemodHead + kDemodSpan + 1 + kDemodThreads - 1) / kDemodThreads) | 1;  // 35
constexpr int kDemodSymbolChunk = ((kDemodTile + kDemodSpan + 1 + kDemodThreads - 1) / kDemodThreads) | 1;  // 19
static_assert(kDemodTimingChunk * kDemodThreads >= kDemodHead + kDemodSpan + 1 && kDemodSymbolChunk * kDemodThreads >= kDemodTile + kDemodSpan + 1,
	      "every entry of the prefix sums has a lane");

// the settings as the kernels take them: R, the code, Pn and Nt
struct DemodShape {
	int rate, man, pn, nt;
};

__device__ inline unsigned long long demod_grid(unsigned long long j, int rate) { return 384000ull * j / (unsigned)rate; }  // g(j)
// b(2 j + 1) of the Manchester chips: where bit j's second chip begins
__device__ inline unsigned long long demod_mid(unsigned long long j, int rate) { return 384000ull * (2ull * j + 1ull) / (2u * (unsigned)rate); }
// the decisions that end ahead of chain sample x under the phase p: the m >= 1 with p + g(m) <= x
__device__ inline unsigned long long demod_ended(unsigned long long x, uint32_t p, int rate)
{
	return x < p ? 0ull : ((x - p + 1ull) * (unsigned)rate - 1ull) / 384000ull;
}

// l[0 .. n) -> its inclusive prefix sum, in place; lane t owns the entries [t chunk, (t + 1) chunk).  Called by all 256 lanes with the
// entries in place behind a barrier; leaves the sums in place behind one.  |sum| <= 64 * 8576 < 2^20.
__device__ inline void demod_prefix(int *l, int n, int chunk, int t, int *l_wave)
{
	const int lane = t & 63, w = t >> 6;
	const int a = t * chunk < n ? t * chunk : n, e = a + chunk < n ? a + chunk : n;
	int sum = 0;
	for (int i = a; i < e; i++)
		sum += l[i];
	int x = sum;
#pragma unroll
	for (int d = 1; d < 64; d <<= 1) {
		const int o = __shfl_up(x, d);
		if (lane >= d)
			x += o;
	}
	if (lane == 63)
		l_wave[w] = x;
	__syncthreads();
	int at = x - sum;
	for (int v = 0; v < w; v++)
		at += l_wave[v];
	for (int i = a; i < e; i++) {
		at += l[i];
		l[i] = at;
	}
	__syncthreads();
}

// The tiles and the timed runs of a stream's runs that have a record and fit the pool (both monotone in table order: a prefix of the
// stream's runs) -> { tiles, runs without CONTINUES }
__device__ inline uint2 demod_stream_counts(const CaptureStage *__restrict__ srow, int nr, unsigned long long e0, unsigned long long pool0,
					    uint32_t max_runs, unsigned long long max_samples)
{
	uint2 c = make_uint2(0u, 0u);
	for (int k = 0; k < nr && e0 + (unsigned)k < max_runs; k++) {
		const int n = srow[k].end - srow[k].start;
		if (pool0 + srow[k].rank + (unsigned)n > max_samples)
			break;
		c.x += (uint32_t)(n + kDemodTile - 1) / kDemodTile;
		c.y += (srow[k].flags & TFREC_AMD_RUN_CONTINUES) ? 0u : 1u;
	}
	return c;
}

// The two work lists, of every run that has a record and fits the pool, in the order of the table: { table entry, run-relative first
// sample } of every tile of 4096 samples, partial ones included, and the table entry of every run that needs a timing, one without
// CONTINUES; n_work = their two lengths.  corr_list_kernel's shape: a wave per 64 streams, a stream per lane; where its parts of the
// lists begin the wave finds by counting the streams ahead of its own once more.  Shuffles only.  A stream's runs hold at most
// 2 n_blocks whole tiles and one partial tile each: neither `cap` is reached.
__global__ __launch_bounds__(64) void demod_list_kernel(const CaptureStage *__restrict__ stage, int stage_cap, const uint2 *__restrict__ cnt,
							const uint4 *__restrict__ base, int n_streams, uint32_t max_runs,
							unsigned long long max_samples, uint2 *__restrict__ work, uint32_t cap,
							uint32_t *__restrict__ timed, uint32_t timed_cap, uint32_t *__restrict__ n_work)
{
	const int lane = threadIdx.x, s_first = blockIdx.x * 64;
	uint32_t before = 0, tbefore = 0;  // the tiles and the timed runs of the streams ahead of this wave's
	for (int s = lane; s < s_first; s += 64) {
		const uint4 bs = base[s];
		const uint2 c = demod_stream_counts(stage + (size_t)s * stage_cap, (int)cnt[s].x, bs.x, (unsigned long long)bs.z | ((unsigned long long)bs.w << 32),
						    max_runs, max_samples);
		before += c.x;
		tbefore += c.y;
	}
	before = (uint32_t)burst_wave_sum((long long)before);
	tbefore = (uint32_t)burst_wave_sum((long long)tbefore);
	const int s = s_first + lane;
	const bool live = s < n_streams;
	const CaptureStage *srow = stage + (size_t)(live ? s : 0) * stage_cap;
	const int nr = live ? (int)cnt[s].x : 0;
	const uint4 bs = live ? base[s] : make_uint4(0, 0, 0, 0);
	const unsigned long long e0 = bs.x, pool0 = (unsigned long long)bs.z | ((unsigned long long)bs.w << 32);
	const uint2 c = demod_stream_counts(srow, nr, e0, pool0, max_runs, max_samples);
	uint32_t at = before + (uint32_t)cap_prefix_excl((int)c.x, lane), tat = tbefore + (uint32_t)cap_prefix_excl((int)c.y, lane);
	if (blockIdx.x == gridDim.x - 1 && lane == 63) {
		n_work[0] = at + c.x < cap ? at + c.x : cap;
		n_work[1] = tat + c.y < timed_cap ? tat + c.y : timed_cap;
	}
	for (int k = 0; k < nr && e0 + (unsigned)k < max_runs; k++) {
		const int n = srow[k].end - srow[k].start;
		if (pool0 + srow[k].rank + (unsigned)n > max_samples)
			break;
		if (!(srow[k].flags & TFREC_AMD_RUN_CONTINUES)) {
			if (tat < timed_cap)
				timed[tat] = (uint32_t)(e0 + (unsigned)k);
			tat++;
		}
		for (int n0 = 0; n0 < n; n0 += kDemodTile, at++)
			if (at < cap)
				work[at] = make_uint2((uint32_t)(e0 + (unsigned)k), (uint32_t)n0);
	}
}

// The timing of the listed runs, the chains' first pieces; a workgroup takes the runs blockIdx.x, blockIdx.x + gridDim.x, ... of the list.
//   1. Ns = min(Nt, the m >= 1 with Pn - 1 + g(m) <= n).  Below 8: phase 0, FLAGGED, and the next run.
//   2. The run's first m = min(n, 8192 + 384) soft bytes into LDS as dwords, entry 0 a zero ahead of them, and their prefix sum in
//      place: entry i is the sum of u[0 .. i).  g(j), j <= Ns, and the Manchester chips' middles beside them, a decision per lane.
//   3. A phase per lane and step, p < Pn <= 384: its Ns decisions as differences of entries p + g(j) -- the largest index, Pn - 1 +
//      g(Ns), is at most n and at most 383 + 8192 --, E[p] = the sum of their magnitudes, at most 64 * 64 * 384 < 2^21.
//   4. (E << 32 | ~p) under a maximum -- the first p of the largest E -- and the sum of E, over the wave by shuffles and over the
//      waves in LDS; lane 0 writes the record.  The carried p* is demod_carry_kernel's to write: a stream's run that CONTINUES is read
//      by demod_symbol_kernel, behind this kernel, with the p* the submit before left.
// Every loop and barrier is uniform over the workgroup.
__global__ __launch_bounds__(kDemodThreads) void demod_timing_kernel(const tfrec_amd_run *__restrict__ runs, const uint32_t *__restrict__ timed,
								      const uint32_t *__restrict__ n_work, const int8_t *__restrict__ soft,
								      const DemodShape sh, tfrec_amd_demod *__restrict__ out)
{
	__shared__ int l_sum[kDemodTimingChunk * kDemodThreads];
	__shared__ int l_grid[kDemodTimed + 1], l_mid[kDemodTimed];
	__shared__ int l_wave[4];
	__shared__ unsigned long long l_key[4], l_tot[4];
	const int t = threadIdx.x, lane = t & 63, w = t >> 6;
	const uint32_t nt = n_work[1];
	for (uint32_t item = blockIdx.x; item < nt; item += gridDim.x) {
		const uint32_t e = timed[item];
		const tfrec_amd_run r = runs[e];
		const int n = (int)r.n_samples;
		const unsigned long long fit = n >= sh.pn - 1 ? demod_ended((unsigned long long)(n - (sh.pn - 1)), 0u, sh.rate) : 0ull;
		const int ns = fit < (unsigned)sh.nt ? (int)fit : sh.nt;
		if (ns < kDemodMinTimed) {
			if (t == 0) {
				out[e].timing = TFREC_AMD_DEMOD_FLAGGED;
				out[e].n_timed = (uint32_t)ns;
			}
			continue;
		}
		const int m = n < kDemodHead + kDemodSpan ? n : kDemodHead + kDemodSpan;
		for (int i = t; i <= m; i += kDemodThreads)
			l_sum[i] = i ? (int)soft[r.pool_offset + (unsigned)(i - 1)] : 0;  // (pool_offset + n <= max_samples: the list holds no other run)
		if (t <= ns)
			l_grid[t] = (int)demod_grid((unsigned)t, sh.rate);
		if (t < ns)
			l_mid[t] = (int)demod_mid((unsigned)t, sh.rate);
		__syncthreads();
		demod_prefix(l_sum, m + 1, kDemodTimingChunk, t, l_wave);
		unsigned long long key = 0ull, tot = 0ull;
		for (int p = t; p < sh.pn; p += kDemodThreads) {
			const int *at = l_sum + p;
			uint32_t energy = 0u;
			int lo = at[0];
			for (int j = 0; j < ns; j++) {
				const int hi = at[l_grid[j + 1]];  // (p + g(j + 1) <= Pn - 1 + g(Ns) <= m)
				const int d = sh.man ? 2 * at[l_mid[j]] - lo - hi : hi - lo;
				energy += (uint32_t)(d < 0 ? -d : d);
				lo = hi;
			}
			const unsigned long long k = ((unsigned long long)energy << 32) | (uint32_t)~p;
			key = k > key ? k : key;
			tot += energy;
		}
#pragma unroll
		for (int d = 1; d < 64; d <<= 1) {
			const unsigned long long o = __shfl_xor(key, d);
			key = o > key ? o : key;
			tot += __shfl_xor(tot, d);
		}
		if (lane == 0) {
			l_key[w] = key;
			l_tot[w] = tot;
		}
		__syncthreads();
		if (t == 0) {
#pragma unroll
			for (int v = 1; v < 4; v++) {
				key = l_key[v] > key ? l_key[v] : key;
				tot += l_tot[v];
			}
			tfrec_amd_demod *o = out + e;
			o->phase = ~(uint32_t)key;  // (every phase has a key: Pn >= 4)
			o->timing = TFREC_AMD_DEMOD_MEASURED;
			o->n_timed = (uint32_t)ns;
			o->e_best = key >> 32;
			o->e_sum = tot;
		}
		__syncthreads();  // (the next run's writes to LDS lie behind this run's last reads)
	}
}

// A tile of the work list: the decisions whose LAST sample is one of the samples n0 .. n0 + 4095 of a run.  With A the chain's samples
// ahead of the piece and p its phase -- the record's, where demod_timing_kernel wrote it; the stream's carried ones where the run
// CONTINUES -- those are the chain indices demod_ended(A + n0) .. demod_ended(A + ne) - 1, ne the tile's end inside the piece.
//   1. The soft bytes of the run-relative samples n0 - 384 .. ne - 1 into LDS as dwords behind a zero: out of the pool; out of the
//      stream's carried bytes where the index is negative and the run CONTINUES (crow[384 + x] is the chain's sample x of the piece);
//      else 0, ahead of the chain, where no decision reaches.  Their prefix sum in place: entry i is the sum of the i samples from n0 - 384.
//   2. A decision per lane and step: it ends in the tile and spans at most 384 samples, so both ends lie in the entries 1 .. 384 + ne -
//      n0.  It is stored at pool_offset + its chain index less the piece's first: no order of tiles matters.
//   3. The entries of the run's part of the decision pool that hold no decision (n_symbols <= i < n) are zeroed by the tile of sample i.
//   4. The tile's count goes to n_symbols with one atomic; the tile of n0 = 0 writes first_symbol and, where the run CONTINUES, the
//      inherited phase.
__device__ inline void demod_tile(const tfrec_amd_run *__restrict__ runs, const uint2 we, const int8_t *__restrict__ soft,
				  const int8_t *__restrict__ carry, const unsigned long long *__restrict__ ahead, const uint32_t *__restrict__ cphase,
				  const DemodShape &sh, tfrec_amd_demod *__restrict__ out, int16_t *__restrict__ dec, int t, int *l_sum, int *l_wave)
{
	const tfrec_amd_run r = runs[we.x];
	const int n = (int)r.n_samples, n0 = (int)we.y;
	const int ne = n0 + kDemodTile < n ? n0 + kDemodTile : n;
	const bool cont = (r.flags & TFREC_AMD_RUN_CONTINUES) != 0;
	const unsigned long long A = cont ? ahead[r.stream] : 0ull;
	const uint32_t p = cont ? cphase[r.stream] : out[we.x].phase;
	const int8_t *crow = carry + (size_t)r.stream * kDemodSpan;
	const int m = kDemodSpan + ne - n0;  // staged samples
	for (int i = t; i <= m; i += kDemodThreads) {
		const int x = n0 - kDemodSpan + i - 1;
		int v = 0;
		if (i) {
			if (x >= 0)
				v = soft[r.pool_offset + (unsigned)x];  // (x < ne <= n)
			else if (cont)
				v = crow[kDemodSpan + x];  // (0 <= . < 384)
		}
		l_sum[i] = v;
	}
	__syncthreads();
	demod_prefix(l_sum, m + 1, kDemodSymbolChunk, t, l_wave);
	const unsigned long long j0 = demod_ended(A, p, sh.rate), jn = demod_ended(A + (unsigned)n, p, sh.rate);
	const unsigned long long ja = demod_ended(A + (unsigned)n0, p, sh.rate), jb = demod_ended(A + (unsigned)ne, p, sh.rate);
	const long long origin = (long long)A + n0 - kDemodSpan - (long long)p;  // entry i is the prefix at chain sample origin + p + i
	for (unsigned long long j = ja + (unsigned)t; j < jb; j += kDemodThreads) {
		const int lo = (int)((long long)demod_grid(j, sh.rate) - origin), hi = (int)((long long)demod_grid(j + 1, sh.rate) - origin);  // 1 <= lo < hi <= m
		int d = l_sum[hi] - l_sum[lo];
		if (sh.man)
			d = 2 * l_sum[(int)((long long)demod_mid(j, sh.rate) - origin)] - l_sum[lo] - l_sum[hi];
		dec[r.pool_offset + (j - j0)] = (int16_t)d;  // (j - j0 < jn - j0 <= n)
	}
	const unsigned long long ns = jn - j0;
	for (int i = n0 + t; i < ne; i += kDemodThreads)
		if ((unsigned)i >= ns)
			dec[r.pool_offset + (unsigned)i] = 0;
	if (t == 0) {
		tfrec_amd_demod *o = out + we.x;
		if (jb > ja)
			atomicAdd(&o->n_symbols, (uint32_t)(jb - ja));
		if (n0 == 0) {
			o->first_symbol = j0;
			if (cont) {
				o->phase = p;
				o->timing = TFREC_AMD_DEMOD_INHERITED;
			}
		}
	}
	__syncthreads();  // (the next tile's writes to LDS lie behind this tile's last reads)
}

__global__ __launch_bounds__(kDemodThreads) void demod_symbol_kernel(const tfrec_amd_run *__restrict__ runs, const uint2 *__restrict__ work,
								      const uint32_t *__restrict__ n_work, const int8_t *__restrict__ soft,
								      const int8_t *__restrict__ carry, const unsigned long long *__restrict__ ahead,
								      const uint32_t *__restrict__ cphase, const DemodShape sh,
								      tfrec_amd_demod *__restrict__ out, int16_t *__restrict__ dec)
{
	__shared__ int l_sum[kDemodSymbolChunk * kDemodThreads];
	__shared__ int l_wave[4];
	const uint32_t nw = n_work[0];
	for (uint32_t tile = blockIdx.x; tile < nw; tile += gridDim.x)
		demod_tile(runs, work[tile], soft, carry, ahead, cphase, sh, out, dec, threadIdx.x, l_sum, l_wave);
}

// What the next submit needs of this one, behind demod_symbol_kernel on the same stream -- so the kernel that reads the carried
// state has ended before it is written, and the next submit's reads come behind these writes (the burst track's race argument,
// DESIGN.md 6t).  One workgroup per stream, 384 lanes.  If the stream's last run reaches the submit's last sample, has a record and
// fits the pool: lane i writes the chain's soft sample 384 - i ahead of the next piece out of the run's own, 0 ahead of the run -- a
// run shorter than 384 samples began inside the submit, so it does not CONTINUE and nothing older belongs to its chain; one that
// CONTINUES is at least a block long --, A grows by n (from 0 unless the run CONTINUES) and p* is the record's.  Otherwise A = 0 and p*
// = 0: the piece that CONTINUES an unread run is read as a chain of its own at phase 0.
__global__ __launch_bounds__(kDemodSpan) void demod_carry_kernel(int n_blocks, const CaptureStage *__restrict__ stage, int stage_cap,
								  const uint2 *__restrict__ cnt, const uint4 *__restrict__ base, uint32_t max_runs,
								  unsigned long long max_samples, const int8_t *__restrict__ soft,
								  const tfrec_amd_demod *__restrict__ out, int8_t *__restrict__ carry,
								  unsigned long long *__restrict__ ahead, uint32_t *__restrict__ cphase)
{
	const int s = blockIdx.x, i = threadIdx.x;
	const int nr = (int)cnt[s].x;
	const int M = n_blocks * kBlockDec;
	const uint4 bs = base[s];
	const unsigned long long e0 = bs.x;
	const unsigned long long pool0 = (unsigned long long)bs.z | ((unsigned long long)bs.w << 32);
	unsigned long long a = 0ull;
	uint32_t p = 0u;
	if (nr) {
		const CaptureStage r = stage[(size_t)s * stage_cap + (nr - 1)];
		const unsigned long long dst0 = pool0 + r.rank;
		const int n = r.end - r.start;
		if (r.end == M && e0 + (unsigned)(nr - 1) < max_runs && dst0 + (unsigned)n <= max_samples) {
			const int x = n - kDemodSpan + i;  // the run-relative sample of byte i
			carry[(size_t)s * kDemodSpan + i] = x >= 0 ? soft[dst0 + (unsigned)x] : (int8_t)0;
			a = ((r.flags & TFREC_AMD_RUN_CONTINUES) ? ahead[s] : 0ull) + (unsigned)n;
			p = out[e0 + (unsigned)(nr - 1)].phase;
		}
	}
	if (i == 0) {
		ahead[s] = a;
		cphase[s] = p;
	}
}

hipError_t launch_burst_demod(hipStream_t st, const FrontOut &o, const CaptureBufs &b, const DemodBufs &k)
{
	// a stream's runs hold at most 2 n_blocks whole tiles and a partial one each (capture.h: a run but the first and the last is at least 356 samples long)
	const uint32_t runs_cap = (uint32_t)o.n_streams * (uint32_t)(o.n_blocks * kBlockDec / 356 + 3);  // (<= the buffers': the context's largest submit)
	const uint32_t cap = (uint32_t)o.n_streams * 2u * (uint32_t)o.n_blocks + runs_cap;
	const DemodShape sh = { k.rate, k.man, k.pn, k.nt };
	launch_run_records_init(st, b, k.recs, nullptr);
	hipLaunchKernelGGL(corr_soft_kernel, dim3(o.n_blocks, o.n_streams), dim3(kCorrThreads), 0, st, o.dec, o.dec_stride, o.prevdec, b.stage,
			   b.stage_cap, b.cnt, b.base, b.max_runs, b.max_samples, k.centre_bin, k.soft);
	hipLaunchKernelGGL(demod_list_kernel, dim3((o.n_streams + 63) / 64), dim3(64), 0, st, b.stage, b.stage_cap, b.cnt, b.base, o.n_streams,
			   b.max_runs, b.max_samples, k.work, cap, k.timed, runs_cap, k.n_work);
	hipLaunchKernelGGL(demod_timing_kernel, dim3(runs_cap < (uint32_t)kDemodGrid ? runs_cap : (uint32_t)kDemodGrid), dim3(kDemodThreads), 0, st,
			   b.runs, k.timed, k.n_work, k.soft, sh, k.recs);
	hipLaunchKernelGGL(demod_symbol_kernel, dim3(cap < (uint32_t)kDemodGrid ? cap : (uint32_t)kDemodGrid), dim3(kDemodThreads), 0, st, b.runs,
			   k.work, k.n_work, k.soft, k.carry, k.ahead, k.cphase, sh, k.recs, k.dec);
	hipLaunchKernelGGL(demod_carry_kernel, dim3(o.n_streams), dim3(kDemodSpan), 0, st, o.n_blocks, b.stage, b.stage_cap, b.cnt, b.base,
			   b.max_runs, b.max_samples, k.soft, k.recs, k.carry, k.ahead, k.cphase);
	return hipGetLastError();
}
