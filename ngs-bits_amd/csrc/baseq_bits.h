// The pure pieces of baseq_tile_kernel (scan.hip): qualities to "below min_baseq" bits, and a word of those bits cut to a range of read positions. Plain integer
// code without a load or a lane, so that tests/emul/baseq_bits_emul.cpp can hold it against the obvious loops on the CPU, exhaustively. thr is
// 0x01010101 * (min_baseq & 127); the byte trick holds for min_baseq 1 .. 127 (a larger threshold goes byte by byte in the kernel).
#pragma once
#include <cstdint>

namespace ngsqc {

// the four qualities of a dword -> four flags (bit k: byte k is below the threshold)
__device__ __forceinline__ uint32_t bq_below4(uint32_t w, uint32_t thr)
{
	// bit 7 of a byte of y = (x | 0x80) - min_baseq is set iff the byte's low seven bits reach the threshold, bit 7 of x iff the byte is 128 or more
	// (0xff: no quality): clear in both = below. The four flags (bits 7, 15, 23, 31) move to bits 21..24 of the product: no two terms meet in a bit
	const uint32_t lt = (~(((w | 0x80808080u) - thr) | w) & 0x80808080u) >> 7;
	return ((lt * 0x00204081u) >> 21) & 15u;
}

// the 64 flags of 64 qualities, of which the first `left` are kept (left >= 1; 64 and more: all). The sixteen bq_below4 steps that fill mm stay a loop of the kernel:
// as a function of this file they left the kernel with other register counts (72 VGPRs / 81 SGPRs against 73 / 84) - the move was to be a move and nothing else
__device__ __forceinline__ unsigned long long bq_keep_first(unsigned long long mm, uint32_t left)
{
	return left >= 64u ? mm : mm & ((1ull << left) - 1ull);
}

// word cw of the flags (read positions 64 cw .. 64 cw + 63) cut to the read positions [a_lo, b_hi); the caller has a_lo < 64 cw + 64 and 64 cw < b_hi
__device__ __forceinline__ unsigned long long bq_clip_word(unsigned long long m, uint32_t a_lo, uint32_t b_hi, uint32_t cw)
{
	if (a_lo > 64u * cw) m &= ~0ull << (a_lo - 64u * cw);
	if (b_hi < 64u * cw + 64u) m &= (1ull << (b_hi - 64u * cw)) - 1ull;
	return m;
}

} // namespace ngsqc
