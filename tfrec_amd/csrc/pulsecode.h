// tfrec_amd/csrc/pulsecode.h -- the pulse slicer (tfrec_amd_enable_burst_symbols, include/tfrec_amd.h: "Pulse slicer"):
// an optional stage of the burst track for pulse-width and pulse-gap keyed bursts.  Per run of the recorder's table a stream of
// SYMBOLS -- short, long or break, one per deciding edge (a fall in WIDTH mode, a rise in GAP mode) by the length of the stretch of
// equal track bits ahead of the edge -- as two dense bitmaps (value, break mark) from the run's pool_offset on, and a 48-byte record.
// Behind the track's kernels on the recorder's low-priority lane: the records' init kernel, pulse_zero_kernel, pulse_kernel (edges,
// stretches and classes -> three per-sample bitmaps in the track's packing), pulse_pack_kernel (compaction) and the line code's carry
// kernel on the stage's own 64 words and H.  They read the recorder's table and working set and the track's bitmap of the same set --
// complete: the track's kernels have ended.  Integers only: every bit is joined by OR on zeroed words and every count is a sum, so
// the order of the atomics cannot matter.  The geometry, the run lookup and the LDS fill (code_chain_word) are the line code's.
// Included by frontend.hip (inside namespace tfrec) behind linecode.h.  tfrec_amd/pulsecode.py restates the result.
#pragma once

static_assert(sizeof(tfrec_amd_burst_symbols) == 48 && offsetof(tfrec_amd_burst_symbols, bit_offset) == 24 &&
		      offsetof(tfrec_amd_burst_symbols, n_symbols) == 32 && offsetof(tfrec_amd_burst_symbols, reserved) == 44,
	      "the init kernel copies a table entry's 32 bytes");
// run_records_init_kernel's rule: the entry's 32 bytes (its first 24 and its pool_offset), then the three counts and the reserved 0
template <>
__device__ inline uint32_t run_record_word<tfrec_amd_burst_symbols>(const uint32_t *src, int w)
{
	return w < 8 ? src[w] : 0u;
}

constexpr int kPulseCap = 2047;      // a stretch is counted this far: above every hi
constexpr int kPulseFlagWords = kSyncLds / 64;  // the 320 words ahead of and in the block, a flag each
static_assert(kPulseCap == kSyncHist && kSyncCarryWords == 64 && kSyncThreads == 256, "a lane's walk back spans one 64-bit flag window");

// The words of the set's five bitmaps that the submit's pairs use, zeroed: what the stage's ORs start from (a grid-stride loop)
__global__ __launch_bounds__(256) void pulse_zero_kernel(const CaptureHeader *__restrict__ hdr, unsigned long long max_samples, size_t nw,
							  uint32_t *__restrict__ maps)
{
	const unsigned long long pairs = hdr->n_pairs < max_samples ? hdr->n_pairs : max_samples;
	const size_t bw = (size_t)((pairs + 31) >> 5);  // (<= nw)
	for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < bw * kPulseMaps; i += (size_t)gridDim.x * 256)
		maps[(i / bw) * nw + i % bw] = 0u;
}

// 32 bits of a bitmap from bit D on, D > -32: the bits ahead of bit 0 read 0
__device__ inline uint32_t pulse_fetch(const uint32_t *__restrict__ w, size_t nw, long long D)
{
	return D >= 0 ? sync_fetch(w, nw, (unsigned long long)D) : sync_fetch(w, nw, 0ull) << (int)-D;
}

// bit j of v (a lane's samples) to bit D + j of a zeroed bitmap, D > -32 and every set bit at or behind bit 0: linecode_kernel's step 3
__device__ inline void pulse_or(uint32_t *__restrict__ words, long long D, uint32_t v)
{
	if (!v)
		return;
	const long long wi = D >> 5;
	const int sh = (int)(D & 31);
	const uint32_t vl = v << sh, vh = sh ? v >> (32 - sh) : 0u;
	if (vl)  // (D < 0: every set bit lies in vh)
		atomicOr(words + wi, vl);
	if (vh)
		atomicOr(words + wi + 1, vh);
}

// Block blockIdx.x of stream blockIdx.y, with linecode_kernel's geometry, run lookup and LDS fill: for every run of the stream that
// meets the block and fits the pool, the symbols' per-sample form of the run's part of the block.
//   1. LDS word i holds the chain's track bits at the submit-relative samples b0 - 2048 + 32 i .. + 31 (321 words; the bits ahead of
//      the H available ones are 0).  v is the value of the stretch a deciding edge ends: 1 in WIDTH mode, 0 in GAP mode, uniform.
//   2. Flags: bit i of l_flag says that LDS word i is all v.  Every wave ballots its lanes' own words (words 64 + t), wave 0 the 64
//      history words too: five 64-bit masks per run.
//   3. Lane t owns the samples [b0 + 32 t, + 32): word 64 + t.  Its deciding edges are one mask: the word compared with itself
//      shifted by one over the bit ahead of it (word 63 + t's top bit).  Two deciding edges have a bit that is not v between them,
//      so only the FIRST edge's stretch can leave the word.  Where it does, the lane walks back once: the 64 flags of the words
//      ahead of it are one unaligned 64-bit window of l_flag, the count of its leading ones is the number of whole words of v, and
//      one LDS read of the word behind them and a count of leading bits end the stretch; 64 whole words are 2048 > 2047 bits.
//   4. The loop over the word's at most 16 edges runs in registers: the stretch inside the word is a count of leading zeros of
//      (word ^ v) below the edge.  l is cut to k + H -- the zeros ahead of a chain are no gap -- and to 2047, then classed.
//   5. The event, value and mark words go to the per-sample bitmaps at the run's pool_offset as linecode_kernel's word does; the
//      glitches are reduced over each wave, then in LDS; one atomic per (run, block).
// The run loop is uniform over the workgroup.
__global__ __launch_bounds__(kSyncThreads) void pulse_kernel(const CaptureStage *__restrict__ stage, int stage_cap, const uint2 *__restrict__ cnt,
							      const uint4 *__restrict__ base, uint32_t max_runs, unsigned long long max_samples,
							      const uint32_t *__restrict__ track, const uint32_t *__restrict__ carry,
							      const uint32_t *__restrict__ hist, int gap, int lo_w, int mid_w, int hi_w, int short_one,
							      tfrec_amd_burst_symbols *__restrict__ out, uint32_t *__restrict__ ev_map,
							      uint32_t *__restrict__ val_map, uint32_t *__restrict__ mark_map)
{
	const int b = blockIdx.x, s = blockIdx.y, t = threadIdx.x;
	const int nr = (int)cnt[s].x;  // (<= stage_cap)
	if (nr == 0)
		return;
	const CaptureStage *srow = stage + (size_t)s * stage_cap;
	const uint4 bs = base[s];
	const uint32_t e0 = bs.x;  // the stream's first table entry
	const unsigned long long pool0 = (unsigned long long)bs.z | ((unsigned long long)bs.w << 32);
	__shared__ uint32_t l_gl;
	__shared__ unsigned long long l_flag[kPulseFlagWords];
	__shared__ uint32_t l_t[kSyncLds];
	if (t == 0)
		l_gl = 0;
	const int b0 = b * kBlockDec, b1 = b0 + kBlockDec;
	int lo, hi;
	capture_run_range(srow, nr, b0, b1, t, kSyncThreads, lo, hi);
	if (lo >= hi)
		return;
	const size_t nw = (size_t)((max_samples + 31) >> 5);
	const int H0 = (int)hist[s];  // (<= 2047)
	const uint32_t *crow = carry + (size_t)s * kSyncCarryWords;
	const int n0 = b0 + 32 * t;  // the lane's first sample
	const uint32_t vm = gap ? 0u : ~0u;  // a word of v
	for (int k = lo; k < hi; k++) {
		if ((unsigned long long)e0 + (unsigned)k >= max_runs)
			break;  // (and every later run of the stream: no record)
		const CaptureStage r = srow[k];
		const unsigned long long dst0 = pool0 + r.rank;  // the run's first bit
		const int n = r.end - r.start;  // (1 .. M)
		if (dst0 + (unsigned)n > max_samples)
			continue;  // (uniform) the track has no bits of it
		const bool cont = r.flags & TFREC_AMD_RUN_CONTINUES;
		const int H = cont ? H0 : 0;
		const int a = r.start > b0 ? r.start : b0, e = r.end < b1 ? r.end : b1;  // b0 <= a < e <= b1 <= M
		for (int i = t; i < kSyncLds; i += kSyncThreads) {
			const int m0 = b0 - kSyncCarryBits + 32 * i;  // the word's first sample
			l_t[i] = (m0 + 32 > a - kSyncHist && m0 < e) ? code_chain_word(m0 - r.start, H, cont, crow, track, nw, dst0, n) : 0u;
		}
		__syncthreads();
		const uint32_t w = l_t[kSyncCarryWords + t];
		const unsigned long long own = __ballot(w == vm);
		if ((t & 63) == 0)
			l_flag[1 + (t >> 6)] = own;
		if (t < 64) {
			const unsigned long long old = __ballot(l_t[t] == vm);
			if (t == 0)
				l_flag[0] = old;
		}
		__syncthreads();
		const int j0 = a > n0 ? a - n0 : 0, j1 = e - n0 < 32 ? e - n0 : 32;  // the lane's samples of the run: [n0 + j0, n0 + j1)
		uint32_t ev = 0, val = 0, mk = 0;
		int gl = 0;
		if (j0 < j1) {
			const uint32_t ahead = (w << 1) | (l_t[kSyncCarryWords + t - 1] >> 31);  // t[k - 1] where w holds t[k]
			const uint32_t d = w ^ vm;  // 1 where the track is not v
			const uint32_t edges = d & ~(ahead ^ vm) & (j1 - j0 == 32 ? ~0u : ((1u << (j1 - j0)) - 1u) << j0);
			int back = 0;  // the bits of v ahead of the word, where the first edge's stretch reaches them
			if (edges && !(d & ((1u << (__ffs((int)edges) - 1)) - 1u))) {
				const int q = t >> 6, sh = t & 63;  // the flags of the words t .. t + 63: the top one is the word ahead
				const unsigned long long win = sh ? (l_flag[q] >> sh) | (l_flag[q + 1] << (64 - sh)) : l_flag[q];
				const int c = ~win ? __clzll((long long)~win) : 64;
				back = 32 * kSyncCarryWords;
				if (c < 64)
					back = 32 * c + __clz((int)(l_t[kSyncCarryWords + t - 1 - c] ^ vm));  // (not all v: the count is below 32)
			}
			const int k0 = n0 - r.start + H;  // k + H of the lane's bit 0
			for (uint32_t rest = edges; rest; rest &= rest - 1u) {
				const int j = __ffs((int)rest) - 1;
				const uint32_t m = d & ((1u << j) - 1u);
				int l = m ? j - 32 + __clz((int)m) : j + back;
				const int lim = k0 + j;  // (>= 0)
				l = l < lim ? l : lim;
				l = l < kPulseCap ? l : kPulseCap;
				const bool brk = (gap && l == lim && lim < kPulseCap) || l > hi_w;
				if (!brk && l < lo_w) {
					gl++;
					continue;
				}
				ev |= 1u << j;
				if (brk)
					mk |= 1u << j;
				else if ((l < mid_w) == (short_one != 0))
					val |= 1u << j;
			}
			const long long D = (long long)dst0 + (n0 - r.start);  // bit j of ev is bit D + j of the bitmaps (D > -32; D + j0 >= 0)
			pulse_or(ev_map, D, ev);
			pulse_or(val_map, D, val);
			pulse_or(mark_map, D, mk);
		}
#pragma unroll
		for (int dd = 32; dd >= 1; dd >>= 1)
			gl += __shfl_xor(gl, dd);
		if ((t & 63) == 0 && gl)
			atomicAdd(&l_gl, (uint32_t)gl);
		__syncthreads();
		if (t == 0) {
			if (l_gl)
				atomicAdd(&out[e0 + (unsigned)k].n_glitches, l_gl);
			l_gl = 0;
		}
		__syncthreads();
	}
}

// The compaction, behind pulse_kernel on the same stream, in its geometry: for every run of the stream that meets the block, has a
// record and fits the pool, the symbols of the run's part of the block to their dense places.
//   1. The symbol index of an event is the number of events of the same run ahead of it: the population count of the event bitmap
//      over the run's bits ahead of the block, [pool_offset, pool_offset + b0 - start) -- at most 12288 words, read 256 lanes wide,
//      the two end words masked --, plus an exclusive scan of the lanes' own counts: wave shuffles and one LDS round.
//   2. A lane fetches its 32 samples' event, value and mark bits (unaligned: two words and a shift each), compresses the values and
//      marks at the event bits into at most 16 dense bits and ORs them into `bits` and `marks` at pool_offset + index: at most
//      (n + 1) / 2 symbols a run, so the run's own region.
//   3. n_symbols and n_breaks: one round of atomics per (run, block).
__global__ __launch_bounds__(kSyncThreads) void pulse_pack_kernel(const CaptureStage *__restrict__ stage, int stage_cap, const uint2 *__restrict__ cnt,
								   const uint4 *__restrict__ base, uint32_t max_runs, unsigned long long max_samples,
								   const uint32_t *__restrict__ ev_map, const uint32_t *__restrict__ val_map,
								   const uint32_t *__restrict__ mark_map, tfrec_amd_burst_symbols *__restrict__ out,
								   uint32_t *__restrict__ bits, uint32_t *__restrict__ marks)
{
	const int b = blockIdx.x, s = blockIdx.y, t = threadIdx.x;
	const int nr = (int)cnt[s].x;  // (<= stage_cap)
	if (nr == 0)
		return;
	const CaptureStage *srow = stage + (size_t)s * stage_cap;
	const uint4 bs = base[s];
	const uint32_t e0 = bs.x;
	const unsigned long long pool0 = (unsigned long long)bs.z | ((unsigned long long)bs.w << 32);
	__shared__ uint32_t l_ahead, l_brk;
	__shared__ uint32_t l_wave[kSyncThreads / 64];
	if (t == 0)
		l_ahead = l_brk = 0;
	const int b0 = b * kBlockDec, b1 = b0 + kBlockDec;
	int lo, hi;
	capture_run_range(srow, nr, b0, b1, t, kSyncThreads, lo, hi);
	if (lo >= hi)
		return;
	const size_t nw = (size_t)((max_samples + 31) >> 5);
	const int n0 = b0 + 32 * t;
	for (int k = lo; k < hi; k++) {
		if ((unsigned long long)e0 + (unsigned)k >= max_runs)
			break;
		const CaptureStage r = srow[k];
		const unsigned long long dst0 = pool0 + r.rank;
		const int n = r.end - r.start;
		if (dst0 + (unsigned)n > max_samples)
			continue;  // (uniform)
		const int a = r.start > b0 ? r.start : b0, e = r.end < b1 ? r.end : b1;
		int ahead = 0;
		if (r.start < b0) {  // the run's events ahead of the block: bits [dst0, p1) of the event bitmap (p1 <= dst0 + n <= max_samples)
			const unsigned long long p1 = dst0 + (unsigned)(b0 - r.start);
			const size_t w0 = (size_t)(dst0 >> 5), w1 = (size_t)((p1 - 1) >> 5);
			for (size_t wi = w0 + (unsigned)t; wi <= w1; wi += kSyncThreads) {
				uint32_t m = ~0u;
				if (wi == w0)
					m &= ~0u << (dst0 & 31);
				if (wi == w1 && (p1 & 31))
					m &= (1u << (p1 & 31)) - 1u;
				ahead += __popc(ev_map[wi] & m);
			}
		}
		const int j0 = a > n0 ? a - n0 : 0, j1 = e - n0 < 32 ? e - n0 : 32;
		const long long D = (long long)dst0 + (n0 - r.start);  // the lane's bit j is bit D + j of the per-sample bitmaps
		uint32_t ev = 0, val = 0, mk = 0;
		if (j0 < j1) {
			const uint32_t mask = j1 - j0 == 32 ? ~0u : ((1u << (j1 - j0)) - 1u) << j0;  // (the bits outside it are other runs')
			ev = pulse_fetch(ev_map, nw, D) & mask;
			if (ev) {
				val = pulse_fetch(val_map, nw, D);
				mk = pulse_fetch(mark_map, nw, D) & ev;
			}
		}
		const int c = __popc(ev);
		const int ex = cap_prefix_excl(c, t & 63);  // the events of the wave's lanes ahead of this one
		int brk = __popc(mk);
#pragma unroll
		for (int dd = 32; dd >= 1; dd >>= 1) {
			ahead += __shfl_xor(ahead, dd);
			brk += __shfl_xor(brk, dd);
		}
		if ((t & 63) == 63)
			l_wave[t >> 6] = (uint32_t)(ex + c);
		if ((t & 63) == 0) {
			if (ahead)
				atomicAdd(&l_ahead, (uint32_t)ahead);
			if (brk)
				atomicAdd(&l_brk, (uint32_t)brk);
		}
		__syncthreads();
		uint32_t idx = l_ahead + (uint32_t)ex, total = 0;
#pragma unroll
		for (int q = 0; q < kSyncThreads / 64; q++) {
			idx += q < (t >> 6) ? l_wave[q] : 0u;
			total += l_wave[q];
		}
		if (ev) {
			uint32_t dv = 0, dm = 0;
			int i = 0;
			for (uint32_t rest = ev; rest; rest &= rest - 1u, i++) {
				const int j = __ffs((int)rest) - 1;
				dv |= ((val >> j) & 1u) << i;
				dm |= ((mk >> j) & 1u) << i;
			}
			const long long P = (long long)(dst0 + idx);  // (idx + c <= (n + 1) / 2: inside the run's bits)
			pulse_or(bits, P, dv);
			pulse_or(marks, P, dm);
		}
		__syncthreads();
		if (t == 0) {
			tfrec_amd_burst_symbols *o = out + (e0 + (unsigned)k);
			if (total)
				atomicAdd(&o->n_symbols, total);
			if (l_brk)
				atomicAdd(&o->n_breaks, l_brk);
			l_ahead = l_brk = 0;
		}
		__syncthreads();
	}
}

// The carry is the line code's kernel on the stage's own words and H: the chain's last 2048 TRACK bits and H = min(2047, H' + n)
// behind an OPEN run that has a record and fits the pool, H = 0 otherwise.
hipError_t launch_burst_symbols(hipStream_t st, const FrontOut &o, const CaptureBufs &b, const PulseBufs &k)
{
	launch_run_records_init(st, b, k.recs, (uint32_t *)nullptr);
	const size_t nw = (size_t)((b.max_samples + 31) >> 5);
	uint32_t *ev = k.maps + 2 * nw, *val = k.maps + 3 * nw, *mark = k.maps + 4 * nw;
	const unsigned blocks = (unsigned)std::max<size_t>(1, std::min<size_t>(1024, (nw * kPulseMaps + 255) / 256));
	hipLaunchKernelGGL(pulse_zero_kernel, dim3(blocks), dim3(256), 0, st, b.hdr, b.max_samples, nw, k.maps);
	hipLaunchKernelGGL(pulse_kernel, dim3(o.n_blocks, o.n_streams), dim3(kSyncThreads), 0, st, b.stage, b.stage_cap, b.cnt, b.base, b.max_runs,
			   b.max_samples, k.track, k.carry, k.hist, k.mode == TFREC_AMD_PULSE_GAP, k.lo, k.mid, k.hi,
			   (int)(k.flags & TFREC_AMD_PULSE_SHORT_ONE), k.recs, ev, val, mark);
	hipLaunchKernelGGL(pulse_pack_kernel, dim3(o.n_blocks, o.n_streams), dim3(kSyncThreads), 0, st, b.stage, b.stage_cap, b.cnt, b.base, b.max_runs,
			   b.max_samples, ev, val, mark, k.recs, k.maps, k.maps + nw);
	hipLaunchKernelGGL(linecode_carry_kernel, dim3(o.n_streams), dim3(kSyncCarryWords), 0, st, o.n_blocks, b.stage, b.stage_cap, b.cnt, b.base,
			   b.max_runs, b.max_samples, k.track, k.carry, k.hist);
	return hipGetLastError();
}
