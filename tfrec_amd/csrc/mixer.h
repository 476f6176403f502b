// tfrec_amd/csrc/mixer.h -- the phase mixer of the input pre-stages (DESIGN.md 6d's rotation at the input rate: 6e, 6g, 6h), included
// by frontend.hip inside namespace tfrec behind kTuneCos.  decim10_kernel<true> and resample_fmt_kernel stage their tile through it.
// (frontend_kernel's tuned_x keeps its own form -- a packed (C, S) table and the 15 / 17 shift pair -- where the benchmark times it.)
//
// A sample travels as one dword, I in the low int16 half and Q in the high one, either as x (-8192 <= x <= 8191) or as 4 x: the
// 8-bit formats' b << 8, which one v_perm_b32 makes of the bytes and which the rotation's shift by 17 instead of 15 takes back.

// kTuneCos -> 4096 int16 in LDS (8 KB; S[k] is C[k - 1024]); the caller's barrier comes behind it
__device__ __forceinline__ void mixer_stage_table(int16_t *ctab, int tid, int nthreads)
{
	for (int i = tid; i < kTuneN / 2; i += nthreads)
		reinterpret_cast<uint32_t *>(ctab)[i] = (uint32_t)(uint16_t)kTuneCos[2 * i] | ((uint32_t)(uint16_t)kTuneCos[2 * i + 1] << 16);
}

// sample `half` (0, 1) of a dword of two's-complement bytes I0 Q0 I1 Q1 -> (b << 8) per half: the bytes into the high bytes
__device__ __forceinline__ uint32_t mixer_b8(uint32_t w, int half)
{
	return __builtin_amdgcn_perm(0u, w, half ? 0x030c020cu : 0x010c000cu);
}

// 4 x -> x, and back: an arithmetic >> 2 per half ((b << 8) >> 2 = b << 6; an s16 >> 2), and << 2
__device__ __forceinline__ uint32_t mixer_x(uint32_t x4)
{
	return ((uint32_t)((int)(int16_t)(x4 & 0xffffu) >> 2) & 0xffffu) | ((uint32_t)((int)x4 >> 18) << 16);
}
__device__ __forceinline__ uint32_t mixer_x4(uint32_t x) { return (x << 2) & 0xfffcfffcu; }

// (4 I, 4 Q) at phase p (2^-32 turns) -> (I', Q'): k = p >> 20, I' = (4 I C[k] + 4 Q S[k] + 2^16) >> 17 and
// Q' = (4 Q C[k] - 4 I S[k] + 2^16) >> 17 as two v_dot2_i32_i16.  |4 x| <= 32768 and |C| + |S| < 2^15.6 keep the dot product in
// int32, and |I'|, |Q'| <= 11585: nothing saturates.
__device__ __forceinline__ uint32_t mixer_rotate(const int16_t *ctab, uint32_t x4, uint32_t p)
{
	typedef short s16x2 __attribute__((ext_vector_type(2)));
	const uint32_t k = p >> (32 - TFREC_TUNE_BITS);
	const int C = ctab[k], S = ctab[(k - kTuneN / 4) & (kTuneN - 1)];
	const uint32_t cs = ((uint32_t)C & 0xffffu) | ((uint32_t)S << 16);   // (C, S)
	const uint32_t sc = ((uint32_t)-S & 0xffffu) | ((uint32_t)C << 16);  // (-S, C)
	const int vi = __builtin_amdgcn_sdot2(__builtin_bit_cast(s16x2, x4), __builtin_bit_cast(s16x2, cs), 1 << 16, false) >> 17;
	const int vq = __builtin_amdgcn_sdot2(__builtin_bit_cast(s16x2, x4), __builtin_bit_cast(s16x2, sc), 1 << 16, false) >> 17;
	return ((uint32_t)vi & 0xffffu) | ((uint32_t)vq << 16);
}
