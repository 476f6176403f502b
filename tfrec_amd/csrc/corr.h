// tfrec_amd/csrc/corr.h -- the burst correlator (tfrec_amd_enable_burst_corr, include/tfrec_amd.h: tfrec_amd_corr): per run
// of the recorder's table and per sync template (a word at a rate, up to 16) the largest and the smallest score of a soft matched
// filter over the burst's per-sample direction, where each ends, the defined positions and the sum of |score|.  capture.h's
// run_records_init_kernel, corr_soft_kernel, corr_list_kernel, corr_product_kernel and corr_carry_kernel, on the recorder's
// low-priority lane behind the burst band's.  They read the recorder's table and working set, the decimated samples and prevdec, and
// the 2047 soft bytes and H they carried themselves.  Exact integers only: n_pos and sum_abs are sums, the extremes one 64-bit maximum
// and one 64-bit minimum each, so neither the order of the atomics nor the grouping of the matrix instruction's sums can matter.
// Included by frontend.hip (inside namespace tfrec) behind band.h.  tfrec_amd/corr.py restates the result.
//
// The correlation of a tile of 256 positions with the bank is ONE int8 product, positions as rows:
//   Y[256 x 16] = A[256 x Kp] B[Kp x 16],   A[r][j] = w[r + j], w[i] = u[n0 - Kp + 1 + i] (a Hankel matrix),   B[j][t] = Tp_t[j],
// Tp_t the template right-aligned in Kp taps, on __builtin_amdgcn_mfma_i32_16x16x64_i8.  -64 <= u <= 63 and T = +-1: no planes, and
// every int32 accumulator stays at or below 64 * 2048 = 2^17.
#pragma once

static_assert(sizeof(tfrec_amd_corr_score) == 32 && offsetof(tfrec_amd_corr_score, trough) == 8 && offsetof(tfrec_amd_corr_score, n_pos) == 16 &&
		      offsetof(tfrec_amd_corr_score, sum_abs) == 24 && sizeof(tfrec_amd_corr) == 536 && offsetof(tfrec_amd_corr, t) == 24,
	      "the init kernel copies a table entry's first 24 bytes; corr_product_kernel keeps one 64-bit key in a score's first and one in its second 8 bytes");
// run_records_init_kernel's rule -- the entry's first 24 bytes; per template the maximum's start, 0, in its first 8 bytes, the
// minimum's start, all ones, in its second 8, and zeros (corr_carry_kernel turns the keys into peak, peak_at, trough, trough_at)
template <>
__device__ inline uint32_t run_record_word<tfrec_amd_corr>(const uint32_t *src, int w)
{
	return w < 6 ? src[w] : (((w - 6) & 7) == 2 || ((w - 6) & 7) == 3) ? 0xffffffffu : 0u;
}

constexpr int kCorrThreads = 256;   // corr_soft_kernel: a workgroup per (stream, block); corr_product_kernel: four waves per tile
constexpr int kCorrGrid = 4096;     // corr_product_kernel's workgroups at the most: 16 a compute unit, each walks the list in strides
constexpr int kCorrTile = 256;      // positions per tile: 16 row tiles of the instruction
constexpr int kCorrHist = 2047;     // the soft bytes ahead of a piece that a score may need: the largest K_t - 1
constexpr int kCorrCarry = 2048;    // bytes per stream: byte j is u[j - 2047] of the piece that continues the chain
constexpr int kCorrBase = kCorrTile + kCorrMaxTaps + 32;  // the tile's window w, with the 16 bytes the shifted copies read past it
constexpr int kCorrCopy = kCorrTile + kCorrMaxTaps + 16;  // a copy's stride, 2320 = 9 * 256 + 16 bytes: copy m begins 16 m bytes into
							   // the 256 bytes that the 64 banks hold: 16 consecutive lanes read sixteen different bank quads (corr_tile, step 2)
static_assert(kCorrMaxTaps == 2048 && kCorrHist == kCorrMaxTaps - 1 && kCorrCopy % 256 == 16 && kCorrCopy % 16 == 0 && kCorrBase % 4 == 0,
	      "the copies' bank spread and alignment");
static_assert(kCorrBase + 16 * kCorrCopy + 4 * 16 * 32 <= 64 * 1024, "corr_product_kernel's LDS is static");

typedef int corr_v4i __attribute__((ext_vector_type(4)));

// the settings as the kernels take them: every template's taps, the bank's depth and size, and the centre's bin
struct CorrShape {
	int kt[16];
	int n_templates, kp, c;
};

// Block blockIdx.x of stream blockIdx.y, with track_kernel's geometry and capture_run_range's lookup: for every run of the stream
// that meets the block, has a record and fits the pool, the soft byte of every sample of the run's part of the block, a sample
// per lane and step, written where the sample's pair lies in the pool.  The product is the burst meter's: the pair before it
// inside the row, or prevdec at the submit's first sample; none at a run's first sample unless the run CONTINUES.
__global__ __launch_bounds__(kCorrThreads) void corr_soft_kernel(const uint32_t *__restrict__ dec, size_t dec_stride,
								  const uint32_t *__restrict__ prevdec, const CaptureStage *__restrict__ stage,
								  int stage_cap, const uint2 *__restrict__ cnt, const uint4 *__restrict__ base,
								  uint32_t max_runs, unsigned long long max_samples, int c,
								  int8_t *__restrict__ soft)
{
	const int b = blockIdx.x, s = blockIdx.y, t = threadIdx.x;
	const int nr = (int)cnt[s].x;  // (<= stage_cap)
	if (nr == 0)
		return;
	const CaptureStage *srow = stage + (size_t)s * stage_cap;
	const uint4 bs = base[s];
	const unsigned long long e0 = bs.x;
	const unsigned long long pool0 = (unsigned long long)bs.z | ((unsigned long long)bs.w << 32);
	const int b0 = b * kBlockDec, b1 = b0 + kBlockDec;
	int lo, hi;
	capture_run_range(srow, nr, b0, b1, t, kCorrThreads, lo, hi);
	const uint32_t *row = dec + (size_t)s * dec_stride;
	for (int k = lo; k < hi; k++) {
		if (e0 + (unsigned)k >= max_runs)
			break;  // (and every later run of the stream: no record)
		const CaptureStage r = srow[k];
		const unsigned long long dst0 = pool0 + r.rank;  // the run's first byte
		if (dst0 + (unsigned)(r.end - r.start) > max_samples)
			break;  // (and every later run of the stream)
		const bool cont = (r.flags & TFREC_AMD_RUN_CONTINUES) != 0;
		const int a = r.start > b0 ? r.start : b0, e = r.end < b1 ? r.end : b1;  // b0 <= a < e <= b1 <= M
		for (int n = a + t; n < e; n += kCorrThreads) {
			int u = 0;
			if (n > r.start || cont) {
				const uint32_t w = row[n], wp = n > 0 ? row[n - 1] : prevdec[s];
				const int I = (int16_t)(w & 0xffffu), Q = (int16_t)(w >> 16);
				const int Ip = (int16_t)(wp & 0xffffu), Qp = (int16_t)(wp >> 16);
				const long long dot = (long long)I * Ip + (long long)Q * Qp, crs = (long long)Q * Ip - (long long)I * Qp;
				if (dot | crs) {
					const int j = burst_bin(dot, crs);
					u = (j < 32 ? j : j - 64) - c;  // (-32 - 32 .. 31 + 32)
				}
			}
			soft[dst0 + (unsigned)(n - r.start)] = (int8_t)u;  // (below dst0 + n_samples <= max_samples)
		}
	}
}

// The tiles of a stream's runs that have a record and fit the pool (both monotone in table order: a prefix of the stream's runs)
__device__ inline uint32_t corr_stream_tiles(const CaptureStage *__restrict__ srow, int nr, unsigned long long e0, unsigned long long pool0,
					     uint32_t max_runs, unsigned long long max_samples)
{
	uint32_t c = 0;
	for (int k = 0; k < nr && e0 + (unsigned)k < max_runs; k++) {
		const int n = srow[k].end - srow[k].start;
		if (pool0 + srow[k].rank + (unsigned)n > max_samples)
			break;
		c += (uint32_t)(n + kCorrTile - 1) / kCorrTile;
	}
	return c;
}

// The work list: { table entry, run-relative first position } of every tile of 256 positions, partial ones included, of every run
// that has a record and fits the pool, by stream, run and tile -- the order of the table --, and its length.  band_list_kernel's
// shape: a wave per 64 streams, a stream per lane; where its part of the list begins the wave finds by counting the streams ahead
// of its own once more, a strided share per lane.  Shuffles only; no LDS, no atomic.  A stream's runs hold at most 32 n_blocks
// whole tiles and one partial tile each: `cap`, n_streams (32 n_blocks + the recorder's bound on a stream's runs), is never reached.
__global__ __launch_bounds__(64) void corr_list_kernel(const CaptureStage *__restrict__ stage, int stage_cap, const uint2 *__restrict__ cnt,
						       const uint4 *__restrict__ base, int n_streams, uint32_t max_runs,
						       unsigned long long max_samples, uint2 *__restrict__ work, uint32_t cap,
						       uint32_t *__restrict__ n_work)
{
	const int lane = threadIdx.x, s_first = blockIdx.x * 64;
	uint32_t before = 0;  // the tiles of the streams ahead of this wave's
	for (int s = lane; s < s_first; s += 64) {
		const uint4 bs = base[s];
		before += corr_stream_tiles(stage + (size_t)s * stage_cap, (int)cnt[s].x, bs.x, (unsigned long long)bs.z | ((unsigned long long)bs.w << 32),
					    max_runs, max_samples);
	}
	before = (uint32_t)burst_wave_sum((long long)before);
	const int s = s_first + lane;
	const bool live = s < n_streams;
	const CaptureStage *srow = stage + (size_t)(live ? s : 0) * stage_cap;
	const int nr = live ? (int)cnt[s].x : 0;
	const uint4 bs = live ? base[s] : make_uint4(0, 0, 0, 0);
	const unsigned long long e0 = bs.x, pool0 = (unsigned long long)bs.z | ((unsigned long long)bs.w << 32);
	const uint32_t c = corr_stream_tiles(srow, nr, e0, pool0, max_runs, max_samples);
	uint32_t at = before + (uint32_t)cap_prefix_excl((int)c, lane);
	if (blockIdx.x == gridDim.x - 1 && lane == 63)
		*n_work = at + c < cap ? at + c : cap;
	for (int k = 0; k < nr && e0 + (unsigned)k < max_runs; k++) {
		const int n = srow[k].end - srow[k].start;
		if (pool0 + srow[k].rank + (unsigned)n > max_samples)
			break;
		for (int n0 = 0; n0 < n; n0 += kCorrTile, at++)
			if (at < cap)
				work[at] = make_uint2((uint32_t)(e0 + (unsigned)k), (uint32_t)n0);
	}
}

// A tile of the work list: the positions n0 .. n0 + 255 of one run against the whole bank.  corr_product_kernel's workgroups take
// the tiles blockIdx.x, blockIdx.x + gridDim.x, ...: the grid is at most kCorrGrid workgroups, not one per possible tile.
//   1. The tile's window w[i] = u[n0 - Kp + 1 + i], 0 <= i < 256 + Kp + 16, into LDS, a byte per lane and step: out of the soft
//      pool where the index lies in the piece, out of the stream's carried bytes where it is negative and within the H of a run that
//      CONTINUES, else 0 (ahead of the chain; behind the piece, whose rows are masked).
//   2. Sixteen byte-shifted copies, copy_m[i] = w[i + m], a dword per lane and step out of two dwords of w: row 16 q + m of the
//      product reads the taps 64 c + 16 g .. + 15 of chunk c as the 16 ALIGNED bytes copy_m[16 q + 64 c + 16 g ..].  A copy's
//      stride is 2320 bytes, so the sixteen lanes of equal g, whose reads lie a stride apart, read sixteen different 16-byte
//      quads of the 256 bytes the banks hold -- on the assumption, not measured, that a wave's 64 16-byte reads are served in
//      groups of 16 consecutive lanes (lanes (m, g) and (m + 1, g - 1) do share a quad).
//   3. The Hankel structure: the operand of (row tile q, chunk c) is that of (q + 4, c - 1).  Wave w owns the row tiles w, w + 4, w +
//      8, w + 12 and keeps a ring of four operands, A(d) = the 16 bytes at 16 w + 64 d + 16 g of copy lane & 15: one LDS read a
//      chunk, A(c + 3), feeds four instructions; the chunk's 16 bytes of the bank per lane come from global memory, once for the four.
//      No chunk is zero for every template (the longest one's taps begin fewer than 64 taps into the bank): the loop starts at 0.
//   4. Register i of accumulator j of lane l is template l & 15 at position n0 + 16 (w + 4 j) + 4 (l >> 4) + i.  Positions behind
//      the piece, undefined ones (k + H < K_t - 1) and templates at or above n_templates are masked.  (Y, first k) folds into one
//      64-bit key per extreme -- (Y + 2^31) << 32 | ~k under a maximum, (Y + 2^31) << 32 | k under a minimum: the tie goes to the
//      first k --, reduced over the four lanes of a template with shuffles and over the waves in LDS; one round of atomics per
//      (run, template, tile): the two keys, sum_abs and n_pos, where anything is defined.
// Every loop and barrier is uniform over the workgroup.  No floating point.
__device__ inline void corr_tile(const tfrec_amd_run *__restrict__ runs, const uint2 we, const int8_t *__restrict__ soft,
				 const int8_t *__restrict__ carry, const uint32_t *__restrict__ hist, const int8_t *__restrict__ bank,
				 const CorrShape &sh, tfrec_amd_corr *__restrict__ out, int t, int lane, int w, int8_t *l_base, int8_t *l_copy,
				 unsigned long long (*l_max)[16], unsigned long long (*l_min)[16], unsigned long long (*l_abs)[16],
				 uint32_t (*l_pos)[16])
{
	const tfrec_amd_run r = runs[we.x];
	const int n = (int)r.n_samples, n0 = (int)we.y, kp = sh.kp;
	const bool cont = (r.flags & TFREC_AMD_RUN_CONTINUES) != 0;
	const int H = cont ? (int)hist[r.stream] : 0;  // (<= 2047)
	const int8_t *crow = carry + (size_t)r.stream * kCorrCarry;
	for (int i = t; i < kCorrTile + kp + 16; i += kCorrThreads) {
		const int x = n0 - kp + 1 + i;
		int8_t v = 0;
		if (x >= 0) {
			if (x < n)
				v = soft[r.pool_offset + (unsigned)x];  // (pool_offset + n <= max_samples: the list holds no other run)
		} else if (x >= -H) {
			v = crow[kCorrHist + x];  // (0 <= 2047 - H <= . <= 2046)
		}
		l_base[i] = v;
	}
	__syncthreads();
	const int nd = (kCorrTile + kp) / 4;  // dwords per copy
	const uint32_t *bw = reinterpret_cast<const uint32_t *>(l_base);
#pragma unroll 4
	for (int m = 0; m < 16; m++) {
		uint32_t *cw = reinterpret_cast<uint32_t *>(l_copy + m * kCorrCopy);
		const int dw = m >> 2, bits = 8 * (m & 3);
		for (int j = t; j < nd; j += kCorrThreads) {
			const uint32_t lo = bw[j + dw], hi = bw[j + dw + 1];  // (j + dw + 1 <= nd + 3: within the 16 bytes past the window)
			cw[j] = bits ? (lo >> bits) | (hi << (32 - bits)) : lo;
		}
	}
	__syncthreads();
	const int8_t *cp = l_copy + (lane & 15) * kCorrCopy + 16 * w + 16 * (lane >> 4);
	const corr_v4i *gb = reinterpret_cast<const corr_v4i *>(bank) + lane;
	corr_v4i acc[4];
#pragma unroll
	for (int j = 0; j < 4; j++)
		acc[j] = corr_v4i{ 0, 0, 0, 0 };
	corr_v4i a0 = *reinterpret_cast<const corr_v4i *>(cp), a1 = *reinterpret_cast<const corr_v4i *>(cp + 64),
		 a2 = *reinterpret_cast<const corr_v4i *>(cp + 128);
	const int nch = kp / 64;
	for (int c = 0; c < nch; c++) {
		const corr_v4i a3 = *reinterpret_cast<const corr_v4i *>(cp + 64 * (c + 3));  // (ends at or below 16 w + 48 + 64 (nch + 2) + 16 <= 256 + Kp)
		const corr_v4i bq = gb[c * 64];
		acc[0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a0, bq, acc[0], 0, 0, 0);
		acc[1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a1, bq, acc[1], 0, 0, 0);
		acc[2] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a2, bq, acc[2], 0, 0, 0);
		acc[3] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a3, bq, acc[3], 0, 0, 0);
		a0 = a1;
		a1 = a2;
		a2 = a3;
	}
	// the instruction's result: register i of lane l is row 4 (l >> 4) + i, column l & 15 of the 16 x 16 tile
	const int tt = lane & 15;
	const int kt = sh.kt[tt];
	const int k_first = tt < sh.n_templates ? kt - 1 - H : 0x7fffffff;  // the first defined position
	unsigned long long kmax = 0ull, kmin = ~0ull, sabs = 0ull;
	uint32_t npos = 0;
#pragma unroll
	for (int j = 0; j < 4; j++)
#pragma unroll
		for (int i = 0; i < 4; i++) {
			const int k = n0 + 16 * (w + 4 * j) + 4 * (lane >> 4) + i;
			if (k < n && k >= k_first) {
				const int y = acc[j][i];
				const unsigned long long yb = (unsigned long long)((uint32_t)y + 0x80000000u) << 32;  // (unsigned: the sum wraps)
				const unsigned long long hi = yb | (uint32_t)~k, lo = yb | (uint32_t)k;
				kmax = hi > kmax ? hi : kmax;
				kmin = lo < kmin ? lo : kmin;
				sabs += (unsigned long long)(y < 0 ? -y : y);
				npos++;
			}
		}
#pragma unroll
	for (int d = 16; d <= 32; d <<= 1) {
		const unsigned long long om = __shfl_xor(kmax, d), on = __shfl_xor(kmin, d);
		kmax = om > kmax ? om : kmax;
		kmin = on < kmin ? on : kmin;
		sabs += __shfl_xor(sabs, d);
		npos += __shfl_xor(npos, d);
	}
	if (lane < 16) {
		l_max[w][lane] = kmax;
		l_min[w][lane] = kmin;
		l_abs[w][lane] = sabs;
		l_pos[w][lane] = npos;
	}
	__syncthreads();
	if (t < 16) {
#pragma unroll
		for (int v = 1; v < 4; v++) {
			kmax = l_max[v][t] > kmax ? l_max[v][t] : kmax;
			kmin = l_min[v][t] < kmin ? l_min[v][t] : kmin;
			sabs += l_abs[v][t];
			npos += l_pos[v][t];
		}
		if (npos) {
			tfrec_amd_corr_score *o = &out[we.x].t[t];
			atomicMax(reinterpret_cast<unsigned long long *>(&o->peak), kmax);
			atomicMin(reinterpret_cast<unsigned long long *>(&o->trough), kmin);
			atomicAdd(reinterpret_cast<unsigned long long *>(&o->sum_abs), sabs);
			atomicAdd(&o->n_pos, npos);
		}
	}
}

__global__ __launch_bounds__(kCorrThreads) void corr_product_kernel(const tfrec_amd_run *__restrict__ runs, const uint2 *__restrict__ work,
								     const uint32_t *__restrict__ n_work, const int8_t *__restrict__ soft,
								     const int8_t *__restrict__ carry, const uint32_t *__restrict__ hist,
								     const int8_t *__restrict__ bank, const CorrShape sh,
								     tfrec_amd_corr *__restrict__ out)
{
	const uint32_t nw = *n_work;
	const int t = threadIdx.x, lane = t & 63, w = t >> 6;
	__shared__ __attribute__((aligned(16))) int8_t l_base[kCorrBase];
	__shared__ __attribute__((aligned(16))) int8_t l_copy[16 * kCorrCopy];
	__shared__ unsigned long long l_max[4][16], l_min[4][16], l_abs[4][16];
	__shared__ uint32_t l_pos[4][16];
	// a tile's first write to a part of LDS lies two barriers behind the tile before's last read of it
	for (uint32_t tile = blockIdx.x; tile < nw; tile += gridDim.x)
		corr_tile(runs, work[tile], soft, carry, hist, bank, sh, out, t, lane, w, l_base, l_copy, l_max, l_min, l_abs, l_pos);
}

// What the next submit needs of this one, and the records' keys, behind corr_product_kernel on the same stream -- so the kernel
// that reads carry and hist has ended before they are written, and the next submit's reads come behind these writes (the burst
// track's race argument).  One workgroup per stream.  If the stream's last run reaches the submit's last sample, has
// a record and fits the pool, lane i builds the bytes 8 i .. 8 i + 7 of the chain's last 2047 soft bytes out of the run's, 0 ahead of it
// -- a run shorter than 2047 samples began inside the submit, so it does not CONTINUE and no older byte belongs to its chain; one that
// CONTINUES began at the submit's first sample and is at least a block long --, and H = min(2047, H' + n), H' = 0 unless it CONTINUES.  Otherwise H = 0 and the bytes stay.  Every score of the stream's records gets peak and trough = its key's
// high word less 2^31, peak_at = the complement of the maximum's low word and trough_at = the minimum's low word (0 where n_pos is 0).
__global__ __launch_bounds__(kCorrThreads) void corr_carry_kernel(int n_blocks, const CaptureStage *__restrict__ stage, int stage_cap,
								   const uint2 *__restrict__ cnt, const uint4 *__restrict__ base, uint32_t max_runs,
								   unsigned long long max_samples, const int8_t *__restrict__ soft,
								   int8_t *__restrict__ carry, uint32_t *__restrict__ hist, tfrec_amd_corr *__restrict__ out)
{
	const int s = blockIdx.x, i = threadIdx.x;
	const int nr = (int)cnt[s].x;
	const int M = n_blocks * kBlockDec;
	const uint4 bs = base[s];
	const unsigned long long e0 = bs.x;
	const unsigned long long pool0 = (unsigned long long)bs.z | ((unsigned long long)bs.w << 32);
	int8_t *crow = carry + (size_t)s * kCorrCarry;
	int8_t v[8] = {};
	uint32_t h = 0u;
	bool open = false;
	if (nr) {
		const CaptureStage r = stage[(size_t)s * stage_cap + (nr - 1)];
		const unsigned long long dst0 = pool0 + r.rank;
		const int n = r.end - r.start;
		if (r.end == M && e0 + (unsigned)(nr - 1) < max_runs && dst0 + (unsigned)n <= max_samples) {
			const bool cont = (r.flags & TFREC_AMD_RUN_CONTINUES) != 0;
			const int H = cont ? (int)hist[s] : 0;
			const long long total = (long long)H + n;
			h = (uint32_t)(total < kCorrHist ? total : kCorrHist);
#pragma unroll
			for (int p = 0; p < 8; p++) {
				const int j = 8 * i + p;           // (byte 2047 is never read)
				const int x = n - kCorrHist + j;   // the chain's byte at run-relative x
				if (j < kCorrHist)
					v[p] = x >= 0 ? soft[dst0 + (unsigned)x] : (int8_t)0;
			}
			open = true;
		}
	}
	for (int q = i; q < 16 * nr; q += kCorrThreads) {
		const unsigned long long e = e0 + (unsigned)(q >> 4);
		if (e >= max_runs)
			break;
		uint32_t *f = reinterpret_cast<uint32_t *>(&out[e].t[q & 15]);
		const uint32_t mx_lo = f[0], mx_hi = f[1], mn_lo = f[2], mn_hi = f[3];
		const bool any = f[4] != 0;
		f[0] = mx_hi - 0x80000000u;
		f[1] = any ? ~mx_lo : 0u;
		f[2] = mn_hi - 0x80000000u;
		f[3] = any ? mn_lo : 0u;
	}
	__syncthreads();
	if (open)
#pragma unroll
		for (int p = 0; p < 8; p++)
			crow[8 * i + p] = v[p];
	if (i == 0)
		hist[s] = h;
}

hipError_t launch_burst_corr(hipStream_t st, const FrontOut &o, const CaptureBufs &b, const CorrBufs &k)
{
	// a stream's runs hold at most 32 n_blocks whole tiles and a partial one each (capture.h: a run but the first and the last is at least 356 samples long)
	const uint32_t cap = (uint32_t)o.n_streams * (32u * (uint32_t)o.n_blocks + (uint32_t)(o.n_blocks * kBlockDec / 356 + 3));  // (<= the buffer's: the context's largest submit)
	CorrShape sh;
	for (int t = 0; t < 16; t++)
		sh.kt[t] = k.taps[t];
	sh.n_templates = k.n_templates;
	sh.kp = k.kp;
	sh.c = k.centre_bin;
	launch_run_records_init(st, b, k.recs, nullptr);
	hipLaunchKernelGGL(corr_soft_kernel, dim3(o.n_blocks, o.n_streams), dim3(kCorrThreads), 0, st, o.dec, o.dec_stride, o.prevdec, b.stage,
			   b.stage_cap, b.cnt, b.base, b.max_runs, b.max_samples, sh.c, k.soft);
	hipLaunchKernelGGL(corr_list_kernel, dim3((o.n_streams + 63) / 64), dim3(64), 0, st, b.stage, b.stage_cap, b.cnt, b.base, o.n_streams,
			   b.max_runs, b.max_samples, k.work, cap, k.n_work);
	hipLaunchKernelGGL(corr_product_kernel, dim3(cap < (uint32_t)kCorrGrid ? cap : (uint32_t)kCorrGrid), dim3(kCorrThreads), 0, st, b.runs, k.work, k.n_work, k.soft, k.carry, k.hist, k.bank, sh,
			   k.recs);
	hipLaunchKernelGGL(corr_carry_kernel, dim3(o.n_streams), dim3(kCorrThreads), 0, st, o.n_blocks, b.stage, b.stage_cap, b.cnt, b.base,
			   b.max_runs, b.max_samples, k.soft, k.carry, k.hist, k.recs);
	return hipGetLastError();
}
