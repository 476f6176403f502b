// tfrec_amd/csrc/occupancy.h -- the occupancy detector (tfrec_amd_enable_occupancy, include/tfrec_amd.h the normative text; DESIGN.md
// 6l): per record of the spectrum (spectrum.h) a noise floor -- the lower median of the bins' mean powers -- and a bitmap of the bins
// whose peak hold stands `ratio` times above it and within 1 / `rel` of the record's strongest.  Exact integers only.  One kernel, on
// the spectrum's stream directly behind spectrum_kernel: it reads the records where they lie in device memory.  Included by
// frontend.hip (inside namespace tfrec) behind spectrum.h.  tfrec_amd/occupancy.py restates it.
//
// A workgroup owns one (row, record) and has one lane per bin: N = 64 is one wave, N = 1024 sixteen -- all N bins in one workgroup,
// although spectrum_kernel tiles them by 256, because the median is one of all of them.
//   * m = sum / n_frames (one 64-bit division per lane), and the key (m << 10) | k goes to LDS (8 bytes per bin: at most 8 KB).  m <
//     2^49 and k < 2^10, so the key fits 59 bits; the bin index in its low bits makes the N keys distinct, so that their order is
//     total and the rank below is a permutation.  Ties cannot matter: the median is the value m of the key, whichever bin held it.
//   * the selection is a RANK COUNT: every lane counts the keys smaller than its own, reading all N of them from LDS, and the one
//     lane whose count is N / 2 - 1 holds the lower median.  Every lane of a wave reads the same address (a broadcast: no bank
//     conflict, 16 bytes = two keys per ds_read_b128), so a key costs a 64-bit compare and an add: N^2 <= 2^20 compares per record.
//     The alternatives need a workgroup barrier per step and data-dependent control: a bitonic sort of 1024 keys has 55 passes with
//     a barrier each, a ballot radix select 49 rounds (one per bit of m) with two -- at sixteen waves that is no fewer cycles than
//     the count, which has two barriers, no branch that depends on the data and nothing to get wrong.
//   * the record's largest peak: a butterfly over the wave's lanes, then one LDS slot per wave that every lane reads back.
//   * hit = peak > max(floor, 1) * ratio && peak * rel >= top (both products < 2^61); __ballot forms the wave's 64 bits = two bitmap
//     words, written by its lane 0, and its popcount goes through LDS to the one lane that writes the record's struct.
// One writer per output word; no atomic.
#pragma once

constexpr int kOccMaxBins = kSpecMaxBins;  // lanes per workgroup at most: one per bin
constexpr int kOccKeyShift = 10;           // the bin index below m in a key
static_assert((1 << kOccKeyShift) >= kOccMaxBins, "the bin index fits below m in the key");
static_assert(sizeof(tfrec_amd_occupancy) == 16, "occupancy record");

// sum / peak: [rows][max_records][N], nfr: [rows][max_records] as spectrum_kernel wrote them; recs: [rows][max_records], bits:
// [rows][max_records][N / 32].  grid = rows analysed x n_records, block = N.
__global__ __launch_bounds__(kOccMaxBins) void occupancy_kernel(const unsigned long long *__restrict__ sum, const unsigned long long *__restrict__ peak,
								const uint32_t *__restrict__ nfr, int n_bins, int n_records, size_t max_records,
								unsigned long long ratio, unsigned long long rel, tfrec_amd_occupancy *__restrict__ recs,
								uint32_t *__restrict__ bits)
{
	__shared__ __attribute__((aligned(16))) unsigned long long key[kOccMaxBins];
	__shared__ unsigned long long wave_top[kOccMaxBins / 64];
	__shared__ uint32_t wave_hits[kOccMaxBins / 64];
	__shared__ unsigned long long floor_s;
	const int k = (int)threadIdx.x, lane = k & 63, wave = k >> 6, n_waves = n_bins >> 6;
	const int row = (int)(blockIdx.x / (unsigned)n_records), rec = (int)(blockIdx.x - (unsigned)row * (unsigned)n_records);
	const size_t r = (size_t)row * max_records + (size_t)rec;
	const uint32_t nf = nfr[r];
	const unsigned long long m = sum[r * (size_t)n_bins + (size_t)k] / (unsigned long long)max(nf, 1u);  // (a record holds a frame at least)
	const unsigned long long p = peak[r * (size_t)n_bins + (size_t)k];
	const unsigned long long mine = (m << kOccKeyShift) | (unsigned long long)k;
	key[k] = mine;
	unsigned long long top = p;
#pragma unroll
	for (int d = 32; d >= 1; d >>= 1) {
		const unsigned long long o = __shfl_xor(top, d, 64);
		top = o > top ? o : top;
	}
	if (lane == 0)
		wave_top[wave] = top;
	__syncthreads();
	int below = 0;
	const ulonglong2 *key2 = reinterpret_cast<const ulonglong2 *>(key);
#pragma unroll 8
	for (int j = 0; j < n_bins / 2; j++) {
		const ulonglong2 a = key2[j];
		below += (a.x < mine) + (a.y < mine);
	}
	if (below == n_bins / 2 - 1)  // exactly one lane: the keys are distinct
		floor_s = m;
	for (int w = 0; w < n_waves; w++) {
		const unsigned long long o = wave_top[w];
		top = o > top ? o : top;
	}
	__syncthreads();
	const unsigned long long floor = floor_s;
	const bool hit = p > (floor > 1 ? floor : 1) * ratio && p * rel >= top;
	const unsigned long long b = __ballot(hit);
	if (lane == 0) {
		uint32_t *w = bits + r * (size_t)(n_bins / 32) + (size_t)wave * 2;
		w[0] = (uint32_t)b;
		w[1] = (uint32_t)(b >> 32);
		wave_hits[wave] = (uint32_t)__popcll(b);
	}
	__syncthreads();
	if (k == 0) {
		uint32_t n_hit = 0;
		for (int w = 0; w < n_waves; w++)
			n_hit += wave_hits[w];
		tfrec_amd_occupancy o;
		o.floor = floor;
		o.n_hit = n_hit;
		o.n_frames = nf;
		recs[r] = o;
	}
}

// The detector on the records launch_spectrum has just queued on `st` (the same SpectrumBufs).
hipError_t launch_occupancy(hipStream_t st, const SpectrumBufs &b, uint32_t ratio, uint32_t rel, tfrec_amd_occupancy *recs, uint32_t *bits)
{
	const int n_rows = b.n_rows, n_bins = b.n_bins, g = b.g;
	const size_t max_records = b.max_records;
	const long n_frames = b.n_in / n_bins;
	const long n_records = (n_frames + g - 1) / g;
	if (n_bins < 64 || n_bins > kOccMaxBins || (n_bins & (n_bins - 1)) || g < 1 || n_rows < 1 || (size_t)n_records > max_records ||
	    n_records * n_rows > 0x7fffffffL || ratio < 2 || ratio > 4096 || rel < 1 || rel > 4096)
		return hipErrorInvalidValue;
	if (n_records == 0)
		return hipSuccess;
	hipLaunchKernelGGL(occupancy_kernel, dim3((unsigned)(n_records * n_rows)), dim3((unsigned)n_bins), 0, st, b.sum, b.peak, b.nfr, n_bins,
			   (int)n_records, max_records, (unsigned long long)ratio, (unsigned long long)rel, recs, bits);
	return hipGetLastError();
}
