// tfrec_amd/csrc/state.h -- tfrec_amd_save_streams / tfrec_amd_load_streams: the kernel that gathers a stream's carried state into
// a blob, or scatters a blob over it.  Included by capi.hip; the launcher is declared in launch.h.
#pragma once

namespace tfrec {

// One entry of the inventory: per stream s the `bytes` bytes at base + s * stride, kept at `off` inside the stream's blob
struct StateSeg {
	uint8_t *base;
	unsigned long long stride;
	uint32_t bytes, off;
};
constexpr int kStateSegs = 32;
// The whole inventory of one context (capi_state.h builds it from the records launch_resets reads), passed by value as kernel
// argument.  blob_bytes: a stream's blob, header included (a multiple of 16, as every off is).
struct StateTable {
	StateSeg seg[kStateSegs];
	int32_t n_seg, n_streams;
	uint32_t blob_bytes;
};

template <bool LOAD, class T>
__device__ inline void state_copy(uint8_t *dev, uint8_t *blob, uint32_t bytes, int ln)
{
	T *d = reinterpret_cast<T *>(dev), *b = reinterpret_cast<T *>(blob);
	const uint32_t n = bytes / (uint32_t)sizeof(T);
	for (uint32_t i = (uint32_t)ln; i < n; i += 64) {
		if constexpr (LOAD)
			d[i] = b[i];
		else
			b[i] = d[i];
	}
}

// A workgroup per listed stream (list[0 .. n_list): distinct, < n_streams), like stream_reset_kernel: LOAD false copies every
// segment of stream list[g] into blob g of the staging buffer, LOAD true copies it back.  16 bytes per lane where the stream's
// address and the size allow, dwords or bytes otherwise (the blob side is 16-byte aligned by construction).  Nothing else runs
// on the context while it does: the caller has waited for every stream.
template <bool LOAD>
__global__ __launch_bounds__(64) void stream_state_kernel(StateTable T, const int32_t *__restrict__ list, int n_list, uint8_t *stage)
{
	if ((int)blockIdx.x >= n_list)
		return;
	const int s = list[blockIdx.x];
	if (s < 0 || s >= T.n_streams)
		return;
	const int ln = threadIdx.x;
	uint8_t *blob = stage + (size_t)blockIdx.x * T.blob_bytes;
	for (int k = 0; k < T.n_seg && k < kStateSegs; k++) {
		const StateSeg g = T.seg[k];
		uint8_t *dev = g.base + (size_t)s * g.stride;
		const unsigned al = (unsigned)(uintptr_t)dev | g.bytes;
		if ((al & 15u) == 0)
			state_copy<LOAD, uint4>(dev, blob + g.off, g.bytes, ln);
		else if ((al & 3u) == 0)
			state_copy<LOAD, uint32_t>(dev, blob + g.off, g.bytes, ln);
		else
			state_copy<LOAD, uint8_t>(dev, blob + g.off, g.bytes, ln);
	}
}

hipError_t launch_stream_state(hipStream_t st, bool load, const StateTable &T, const int32_t *list, int n_list, uint8_t *stage)
{
	if (n_list < 1 || T.n_seg < 0 || T.n_seg > kStateSegs || T.blob_bytes % 16 != 0)
		return hipErrorInvalidValue;
	if (load)
		hipLaunchKernelGGL(stream_state_kernel<true>, dim3(n_list), dim3(64), 0, st, T, list, n_list, stage);
	else
		hipLaunchKernelGGL(stream_state_kernel<false>, dim3(n_list), dim3(64), 0, st, T, list, n_list, stage);
	return hipGetLastError();
}

}  // namespace tfrec
