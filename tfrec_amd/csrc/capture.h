// tfrec_amd/csrc/capture.h -- the squelched recorder (tfrec_amd_enable_capture, include/tfrec_amd.h: tfrec_amd_run):
// the decimated IQ of every triggered sample, packed run by run, with a table that says where each run lay.  Three kernels behind
// the front end, on a low-priority stream of their own; they read the decimated samples and the FINAL trigger mask, like the level
// meter, and nothing a demodulator owns.  Also what the burst stages behind it (burst.h .. sync.h) share: the run lookup
// (capture_run_range), the records' init kernel (run_records_init_kernel) and burst_wave_sum.  Included by frontend.hip (inside
// namespace tfrec); CaptureState and CaptureStage are declared in tfrec_dev.h.  tfrec_amd/capture.py restates the result.
//
// A sample is captured while it lies within wmax samples after a trigger, the trigger's own sample included (level_trig_kernel's
// `triggered`).  wmax >= 356 > 64, so within one 64-sample mask word the captured samples are [0, carried) -- what an earlier
// trigger still covers -- and [first, 64), first being the word's own first trigger: a word holds at most one run end (at
// `carried`, when carried < first) and at most one run start (at `first`), the end ahead of the start.  Runs and ends alternate
// along the stream, so the k-th end belongs to the k-th start, and both indices are prefix counts: no atomics, and the order of
// the table is the order of the samples.
#pragma once

static_assert(sizeof(CaptureState) == 16 && sizeof(CaptureStage) == 20 && sizeof(tfrec_amd_run) == 32, "capture records");

constexpr int kCapMaskWords = kBlockDec / 64;  // 128 mask words per block
constexpr int kCapThreads = 256;               // capture_copy_kernel: a workgroup per (stream, block)
constexpr int kCapTile = 4 * kCapThreads;      // samples per step of its copy: one 16-byte load per lane
static_assert(kBlockDec % kCapTile == 0, "capture_copy_kernel's tiling");

__device__ inline int cap_prefix_excl(int v, int lane)  // exclusive prefix sum over the wave's lanes
{
	int x = v;
#pragma unroll
	for (int d = 1; d < 64; d <<= 1) {
		const int o = __shfl_up(x, d);
		if (lane >= d)
			x += o;
	}
	return x - v;
}

__device__ inline long long burst_wave_sum(long long v)  // the sum over the wave's lanes, in every lane
{
#pragma unroll
	for (int d = 32; d >= 1; d >>= 1)
		v += __shfl_xor(v, d);
	return v;
}

// The run lookup of a (stream, block) workgroup, for capture_copy_kernel and every burst stage's kernel behind it.  The stream's nr
// staged runs (srow) are sorted, so those that meet the block's samples [b0, b1) are the index range [lo, hi): lo = runs that end at
// or before the block's first sample, hi = runs that start before its end -- two counts (integer sums: their order does not
// matter), a strided share per lane, joined by two LDS atomics.  Called by all `threads` lanes of the workgroup; two barriers;
// leaves lo and hi in every lane.  What else a kernel zeroes in LDS ahead of the call is in place behind the first barrier.
__device__ inline void capture_run_range(const CaptureStage *__restrict__ srow, int nr, int b0, int b1, int lane, int threads, int &lo, int &hi)
{
	__shared__ int l_lo, l_hi;
	if (lane == 0)
		l_lo = l_hi = 0;
	__syncthreads();
	lo = hi = 0;
	for (int k = lane; k < nr; k += threads) {
		lo += srow[k].end <= b0;
		hi += srow[k].start < b1;
	}
	if (lo)
		atomicAdd(&l_lo, lo);
	if (hi)
		atomicAdd(&l_hi, hi);
	__syncthreads();
	lo = l_lo;
	hi = l_hi;
}

// The records of a burst stage, one per table entry of the submit below max_runs: word w of a record is run_record_word<Rec>(src,
// w), src being the dwords of the entry capture_copy_kernel wrote -- each stage states its rule next to its record's
// static_assert.  With a bitmap (words != null) the zeroed words of the submit's pairs too, as far as the pool holds them.  A
// dword per lane.
template <class Rec>
__device__ inline uint32_t run_record_word(const uint32_t *src, int w);
template <class Rec>
__global__ __launch_bounds__(256) void run_records_init_kernel(const tfrec_amd_run *__restrict__ runs, const CaptureHeader *__restrict__ hdr,
								uint32_t max_runs, unsigned long long max_samples, Rec *__restrict__ out,
								uint32_t *__restrict__ words)
{
	constexpr int kWords = (int)(sizeof(Rec) / 4);
	const unsigned long long total = hdr->n_runs;
	const size_t rw = (size_t)(total < max_runs ? (uint32_t)total : max_runs) * kWords;
	size_t bw = 0;
	if (words) {
		const unsigned long long pairs = hdr->n_pairs < max_samples ? hdr->n_pairs : max_samples;
		bw = (size_t)((pairs + 31) >> 5);
	}
	for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < rw + bw; i += (size_t)gridDim.x * 256) {
		if (i >= rw) {
			words[i - rw] = 0u;
			continue;
		}
		const size_t e = i / kWords;
		const int w = (int)(i - e * kWords);
		reinterpret_cast<uint32_t *>(out + e)[w] = run_record_word<Rec>(reinterpret_cast<const uint32_t *>(runs + e), w);
	}
}

// The init kernel's launch: as many workgroups as the records and the bitmap (max_samples bits, with words) have dwords, 1024 at the most
template <class Rec>
void launch_run_records_init(hipStream_t st, const CaptureBufs &b, Rec *out, uint32_t *words)
{
	const size_t dwords = (size_t)b.max_runs * (sizeof(Rec) / 4) + (words ? (size_t)((b.max_samples + 31) >> 5) : 0);
	const unsigned blocks = (unsigned)std::max<size_t>(1, std::min<size_t>(1024, (dwords + 255) / 256));
	hipLaunchKernelGGL(run_records_init_kernel<Rec>, dim3(blocks), dim3(256), 0, st, b.runs, b.hdr, b.max_runs, b.max_samples, out, words);
}

// The runs of stream blockIdx.x in this submit -> stage[s * stage_cap + k] (submit-relative start and exclusive end, the
// threshold in force at the start, the flags the start decides, and the rank of the run's first pair among the stream's
// captured pairs) and cnt[s] = { runs, pairs }.  One wave per stream, a mask word per lane, 64 words (half a block) per step, as
// level_trig_kernel: the last trigger before a word is an inclusive maximum scan over the lanes, carried from step to step,
// block to block and submit to submit (CaptureState); the threshold's recurrence (fm_demod.cpp:58-73) is recomputed from the
// captured count of each block, wave-uniform.  Reads and writes no FskState and no LevelState.
__global__ __launch_bounds__(64) void capture_scan_kernel(const unsigned long long *__restrict__ mask, size_t mask_stride, int n_blocks,
							  CaptureState *__restrict__ cst, const StreamCfg *__restrict__ scfg,
							  CaptureStage *__restrict__ stage, int stage_cap, uint2 *__restrict__ cnt)
{
	const int s = blockIdx.x, lane = threadIdx.x;
	const int wmax = scfg[s].wmax;
	const bool autoth = scfg[s].autoth != 0;
	const unsigned long long *mrow = mask + (size_t)s * mask_stride;
	const unsigned long long below = lane ? ~0ull >> (64 - lane) : 0ull;  // the lanes before this one
	CaptureStage *srow = stage + (size_t)s * stage_cap;
	CaptureState st = cst[s];
	int last_trig = st.last_trig;
	int n_start = 0, n_end = 0, pairs = 0;
	bool open = false;  // the sample before the next word is captured
	for (int b = 0; b < n_blocks; b++) {
		int triggered = 0;
		st.runs++;
#pragma unroll
		for (int h = 0; h < kCapMaskWords / 64; h++) {
			const int w = b * kCapMaskWords + h * 64 + lane;
			const unsigned long long m = mrow[w];
			const int g0 = w << 6;
			// the last trigger at or before this word's end, then before its start
			int lt = m ? g0 + 63 - __builtin_clzll(m) : -(1 << 29);
#pragma unroll
			for (int d = 1; d < 64; d <<= 1) {
				const int o = __shfl_up(lt, d);
				if (lane >= d && o > lt)
					lt = o;
			}
			int before = __shfl_up(lt, 1);
			if (lane == 0 || before < last_trig)
				before = last_trig;
			const int first = m ? __builtin_ctzll(m) : 64;
			const int raw = before + wmax - g0;  // samples from g0 on that the earlier trigger covers, were there no new one
			const int carried = raw < 0 ? 0 : (raw > first ? first : raw);
			const int captured = carried + (64 - first);
			// The sample before the word is captured iff raw >= 0.  A run that the submit before left open goes on at the
			// submit's first sample: that sample is captured (covered, or a trigger itself) and so was the one before it
			const bool cont = w == 0 && (raw > 0 || (raw == 0 && first == 0));
			const bool has_end = raw >= 0 && raw < first && !(w == 0 && raw == 0);  // (raw == 0: it ended with the word before)
			const bool has_start = first < 64 && raw < first;
			const int rank = pairs + cap_prefix_excl(captured, lane);  // captured pairs of the stream before this word
			const unsigned long long eb = __ballot(has_end), sb = __ballot(has_start);
			if (cont) {  // (lane 0 of the first step: n_start == 0)
				srow[0].start = 0;
				srow[0].thresh = st.thresh;
				srow[0].flags = TFREC_AMD_RUN_CONTINUES;
				srow[0].rank = 0;
			}
			const int c0 = __shfl((int)cont, 0);
			if (has_end) {
				const int k = n_end + __popcll(eb & below);
				if (k < stage_cap)
					srow[k].end = g0 + raw;
			}
			if (has_start) {
				const int k = n_start + c0 + __popcll(sb & below);
				if (k < stage_cap) {
					srow[k].start = g0 + first;
					srow[k].thresh = st.thresh;
					srow[k].flags = 0;
					srow[k].rank = (uint32_t)(rank + carried);
				}
			}
			n_start += c0 + __popcll(sb);
			n_end += __popcll(eb);
			const int tot = __shfl(rank + captured, 63);
			triggered += tot - pairs;
			pairs = tot;
			open = __shfl((int)(first < 64 || carried == 64), 63) != 0;
			const int end = __shfl(lt, 63);
			last_trig = end > last_trig ? end : last_trig;
		}
		st.triggered_avg = (31 * st.triggered_avg + triggered) / 32;
		if (autoth && (st.runs & 3) == 0) {
			if (st.triggered_avg >= kIndexSpan / 32)
				st.thresh += 2;
			else if (st.triggered_avg <= kIndexSpan / 64 && st.thresh > 50)
				st.thresh -= 2;
		}
	}
	if (lane == 0) {
		const int M = n_blocks * kBlockDec;
		if (open && n_start >= 1 && n_start - 1 < stage_cap)  // the run that reaches the submit's last sample (n_end == n_start - 1)
			srow[n_start - 1].end = M;
		cnt[s] = make_uint2((uint32_t)(n_start < stage_cap ? n_start : stage_cap), (uint32_t)pairs);
		st.last_trig = last_trig - M < -(1 << 28) ? -(1 << 28) : last_trig - M;
		cst[s] = st;
	}
}

// Every stream's place in the table and in the pool: the exclusive prefix sums over the streams of cnt[].x (runs) and cnt[].y
// (pairs) -> base[s] = { first table entry, 0, first pair (low, high word) }, and the true totals -> hdr.  One wave, 64 streams
// per step.
__global__ __launch_bounds__(64) void capture_offsets_kernel(const uint2 *__restrict__ cnt, int n_streams, uint4 *__restrict__ base,
							     CaptureHeader *__restrict__ hdr)
{
	const int lane = threadIdx.x;
	unsigned long long runs = 0, pairs = 0;  // of the streams before this step
	for (int s0 = 0; s0 < n_streams; s0 += 64) {
		const int s = s0 + lane;
		const uint2 c = s < n_streams ? cnt[s] : make_uint2(0u, 0u);
		unsigned long long r = c.x, p = c.y;
#pragma unroll
		for (int d = 1; d < 64; d <<= 1) {
			const unsigned long long ro = __shfl_up(r, d), po = __shfl_up(p, d);
			if (lane >= d) {
				r += ro;
				p += po;
			}
		}
		if (s < n_streams) {
			const unsigned long long rb = runs + r - c.x, pb = pairs + p - c.y;
			base[s] = make_uint4((uint32_t)rb, 0u, (uint32_t)pb, (uint32_t)(pb >> 32));
		}
		runs += __shfl(r, 63);
		pairs += __shfl(p, 63);
	}
	if (lane == 0) {
		hdr->n_runs = runs;
		hdr->n_pairs = pairs;
	}
}

// Block blockIdx.x of stream blockIdx.y: the pairs of the stream's runs that lie in the block -> the pool, and (blockIdx.x == 0) the
// stream's entries of the run table.  Capacity: a table entry is written only below max_runs, a run's pairs only when the whole
// run ends at or below max_samples; both conditions are monotone in table order, so what is written is a prefix (the host
// cuts it to whole runs that satisfy both).
// The runs that meet the block are the index range [lo, hi) of the stream's staged runs (capture_run_range).  Each such run's
// part of the block is copied in steps of kCapTile source samples: one aligned 16-byte load per lane into LDS, then four
// rounds in which consecutive lanes store consecutive pairs -- a wave writes 256 contiguous bytes of the pool, wherever the run
// begins in it.  The loops are uniform over the workgroup.
__global__ __launch_bounds__(kCapThreads) void capture_copy_kernel(const uint32_t *__restrict__ dec, size_t dec_stride, int n_blocks,
								   long long sample_base, const CaptureStage *__restrict__ stage,
								   int stage_cap, const uint2 *__restrict__ cnt, const uint4 *__restrict__ base,
								   tfrec_amd_run *__restrict__ runs, uint32_t max_runs,
								   uint32_t *__restrict__ pool, unsigned long long max_samples)
{
	const int b = blockIdx.x, s = blockIdx.y, t = threadIdx.x;
	const int nr = (int)cnt[s].x;  // (<= stage_cap)
	if (nr == 0)
		return;
	const CaptureStage *srow = stage + (size_t)s * stage_cap;
	const uint4 bs = base[s];
	const unsigned long long pool0 = (unsigned long long)bs.z | ((unsigned long long)bs.w << 32);
	const int M = n_blocks * kBlockDec;
	if (b == 0)
		for (int k = t; k < nr; k += kCapThreads) {
			const unsigned long long e = (unsigned long long)bs.x + (unsigned)k;
			if (e >= max_runs)
				break;
			const CaptureStage r = srow[k];
			tfrec_amd_run o;
			o.stream = (uint32_t)s;
			o.flags = r.flags | (r.end == M ? TFREC_AMD_RUN_OPEN : 0u);
			o.start_sample = sample_base + r.start;
			o.n_samples = (uint32_t)(r.end - r.start);
			o.thresh = r.thresh;
			o.pool_offset = pool0 + r.rank;
			runs[e] = o;
		}
	__shared__ uint4 l_tile[kCapThreads];
	const int b0 = b * kBlockDec, b1 = b0 + kBlockDec;
	int lo, hi;
	capture_run_range(srow, nr, b0, b1, t, kCapThreads, lo, hi);
	const uint32_t *row = dec + (size_t)s * dec_stride;
	const uint32_t *tile = reinterpret_cast<const uint32_t *>(l_tile);
	for (int k = lo; k < hi; k++) {
		const CaptureStage r = srow[k];
		const unsigned long long dst0 = pool0 + r.rank;  // the run's first pair in the pool
		if (dst0 + (unsigned)(r.end - r.start) > max_samples)
			break;  // (and every later run of the stream)
		const int a = r.start > b0 ? r.start : b0, e = r.end < b1 ? r.end : b1;  // b0 <= a < e <= b1 <= M
		for (int n0 = a & ~3; n0 < e; n0 += kCapTile) {
			const int n = n0 + 4 * t;  // (a multiple of 4 below M: the 16 bytes lie inside the stream's row)
			if (n < e)
				l_tile[t] = *reinterpret_cast<const uint4 *>(row + n);
			__syncthreads();
#pragma unroll
			for (int j = 0; j < 4; j++) {
				const int i = j * kCapThreads + t, p = n0 + i;
				if (p >= a && p < e)
					pool[dst0 + (unsigned)(p - r.start)] = tile[i];
			}
			__syncthreads();
		}
	}
}

hipError_t launch_capture(hipStream_t st, const FrontOut &o, long long sample_base, const CaptureBufs &b, const StreamCfg *scfg)
{
	hipLaunchKernelGGL(capture_scan_kernel, dim3(o.n_streams), dim3(64), 0, st, o.mask, o.mask_stride, o.n_blocks, b.state, scfg, b.stage,
			   b.stage_cap, b.cnt);
	hipLaunchKernelGGL(capture_offsets_kernel, dim3(1), dim3(64), 0, st, b.cnt, o.n_streams, b.base, b.hdr);
	hipLaunchKernelGGL(capture_copy_kernel, dim3(o.n_blocks, o.n_streams), dim3(kCapThreads), 0, st, o.dec, o.dec_stride, o.n_blocks,
			   sample_base, b.stage, b.stage_cap, b.cnt, b.base, b.runs, b.max_runs, b.pool, b.max_samples);
	return hipGetLastError();
}
