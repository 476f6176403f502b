// tfrec_amd/csrc/levels.h -- the level meter (TFREC_AMD_F_LEVELS, include/tfrec_amd.h: tfrec_amd_level): per stream
// and block of 8192 decimated samples the power the receiver saw and fsk_demod::process's trigger bookkeeping
// (fm_demod.cpp:45-73).  Two kernels behind the front end, on a low-priority stream of their own; they read the decimated samples
// and the FINAL trigger mask and write one 32-byte record per (stream, block).  Included by frontend.hip (inside namespace tfrec);
// LevelState, what level_trig_kernel carries from submit to submit, is declared in tfrec_dev.h beside FskState.
// tfrec_amd/levels.py restates both.
#pragma once

static_assert(sizeof(LevelState) == 16 && sizeof(tfrec_amd_level) == 32, "level meter records");

constexpr int kLevelThreads = 256;                // level_sum_kernel: a workgroup per (stream, block)
constexpr int kLevelMaskWords = kBlockDec / 64;   // 128 mask words per block
static_assert(kBlockDec % (4 * kLevelThreads) == 0 && kLevelMaskWords <= kLevelThreads, "level_sum_kernel's tiling");

// energy, pwr_sum, pwr_max and n_over of block blockIdx.x of stream blockIdx.y.  The block's 32 KB of samples are read once with
// 16-byte loads (4 samples per lane and step, 8 steps), the 128 mask words by the first two waves; a lane's partial sums stay
// in registers (I*I + Q*Q <= 2^31 per sample: 64 bits; pwr <= 2^16, 32 samples per lane: 32 bits), then wave shuffles and one
// pass through LDS.  Everything is an exact integer, so the order of the sums does not matter.
__global__ __launch_bounds__(kLevelThreads) void level_sum_kernel(const uint32_t *__restrict__ dec, size_t dec_stride,
								  const unsigned long long *__restrict__ mask, size_t mask_stride,
								  int n_blocks, tfrec_amd_level *__restrict__ out)
{
	const int b = blockIdx.x, s = blockIdx.y, t = threadIdx.x;
	const uint4 *src = reinterpret_cast<const uint4 *>(dec + (size_t)s * dec_stride + (size_t)b * kBlockDec);
	unsigned long long energy = 0;
	uint32_t psum = 0;
	int pmax = 0;
	uint4 v[kBlockDec / (4 * kLevelThreads)];
#pragma unroll
	for (int k = 0; k < kBlockDec / (4 * kLevelThreads); k++)
		v[k] = src[k * kLevelThreads + t];
	int over = t < kLevelMaskWords ? __popcll(mask[(size_t)s * mask_stride + (size_t)b * kLevelMaskWords + t]) : 0;
#pragma unroll
	for (int k = 0; k < kBlockDec / (4 * kLevelThreads); k++) {
		const uint32_t w[4] = { v[k].x, v[k].y, v[k].z, v[k].w };
#pragma unroll
		for (int j = 0; j < 4; j++) {
			const int I = (int)(int16_t)(w[j] & 0xffff), Q = (int)w[j] >> 16;
			energy += (uint32_t)(I * I) + (uint32_t)(Q * Q);  // (2^30 each at most: the sum fits 32 bits)
			const int pwr = abs(I) + abs(Q);
			psum += (uint32_t)pwr;
			pmax = pwr > pmax ? pwr : pmax;
		}
	}
#pragma unroll
	for (int d = 32; d > 0; d >>= 1) {
		energy += __shfl_xor(energy, d);
		psum += __shfl_xor(psum, d);
		over += __shfl_xor(over, d);
		const int o = __shfl_xor(pmax, d);
		pmax = o > pmax ? o : pmax;
	}
	__shared__ unsigned long long l_energy[kLevelThreads / 64];
	__shared__ uint32_t l_psum[kLevelThreads / 64];
	__shared__ int l_pmax[kLevelThreads / 64], l_over[kLevelThreads / 64];
	if ((t & 63) == 0) {
		l_energy[t >> 6] = energy;
		l_psum[t >> 6] = psum;
		l_pmax[t >> 6] = pmax;
		l_over[t >> 6] = over;
	}
	__syncthreads();
	if (t == 0) {
#pragma unroll
		for (int k = 1; k < kLevelThreads / 64; k++) {
			energy += l_energy[k];
			psum += l_psum[k];
			over += l_over[k];
			pmax = l_pmax[k] > pmax ? l_pmax[k] : pmax;
		}
		tfrec_amd_level *r = out + (size_t)s * n_blocks + b;
		r->energy = energy;
		r->pwr_sum = psum;
		r->pwr_max = pmax;
		r->n_over = over;
	}
}

// triggered, thresh and triggered_avg of every block of stream blockIdx.x: fsk_demod::process's bookkeeping (fm_demod.cpp:36-73)
// recomputed from the final mask alone.  One wave per stream, a mask word per lane, 64 words (half a block) per step.  A sample
// counts as triggered while some registered demodulator's timeout counter runs, that is within wmax samples after a trigger
// (windows.h: threshold_kernel; wmax >= 355 > 64, so everything behind a word's first trigger is inside).  What a word needs of
// its predecessors is the last trigger before it: an inclusive maximum scan over the lanes, carried from step to step, block to
// block and submit to submit.  The recurrence of the threshold is wave-uniform.  Reads and writes no FskState.
// scfg: every stream's settings as this submit runs with them (the context's d_scfg, kept by stream_reset_kernel) -- the stream's
// own longest window, and whether its threshold moves.
__global__ __launch_bounds__(64) void level_trig_kernel(const unsigned long long *__restrict__ mask, size_t mask_stride, int n_blocks,
							LevelState *__restrict__ lev, const StreamCfg *__restrict__ scfg,
							tfrec_amd_level *__restrict__ out)
{
	const int s = blockIdx.x, lane = threadIdx.x;
	const int wmax = scfg[s].wmax;
	const bool autoth = scfg[s].autoth != 0;
	const unsigned long long *mrow = mask + (size_t)s * mask_stride;
	LevelState st = lev[s];
	int last_trig = st.last_trig;
	for (int b = 0; b < n_blocks; b++) {
		int triggered = 0;
		st.runs++;
#pragma unroll
		for (int h = 0; h < kLevelMaskWords / 64; h++) {
			const int w = b * kLevelMaskWords + h * 64 + lane;
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
			int carried = before + wmax - g0;  // samples from g0 on still covered by the earlier trigger
			carried = carried < 0 ? 0 : (carried > first ? first : carried);
			triggered += carried + (64 - first);
			const int end = __shfl(lt, 63);
			last_trig = end > last_trig ? end : last_trig;
		}
#pragma unroll
		for (int d = 32; d > 0; d >>= 1)
			triggered += __shfl_xor(triggered, d);
		const int used = st.thresh;
		st.triggered_avg = (31 * st.triggered_avg + triggered) / 32;
		if (autoth && (st.runs & 3) == 0) {
			if (st.triggered_avg >= kIndexSpan / 32)
				st.thresh += 2;
			else if (st.triggered_avg <= kIndexSpan / 64 && st.thresh > 50)
				st.thresh -= 2;
		}
		if (lane == 0) {
			tfrec_amd_level *r = out + (size_t)s * n_blocks + b;
			r->triggered = triggered;
			r->thresh = used;
			r->triggered_avg = st.triggered_avg;
		}
	}
	if (lane == 0) {
		const int M = n_blocks * kBlockDec;
		st.last_trig = last_trig - M < -(1 << 28) ? -(1 << 28) : last_trig - M;
		lev[s] = st;
	}
}

hipError_t launch_levels(hipStream_t st, const FrontOut &o, LevelState *lev, const StreamCfg *scfg, tfrec_amd_level *out)
{
	hipLaunchKernelGGL(level_sum_kernel, dim3(o.n_blocks, o.n_streams), dim3(kLevelThreads), 0, st, o.dec, o.dec_stride, o.mask, o.mask_stride,
			   o.n_blocks, out);
	hipLaunchKernelGGL(level_trig_kernel, dim3(o.n_streams), dim3(64), 0, st, o.mask, o.mask_stride, o.n_blocks, lev, scfg, out);
	return hipGetLastError();
}
