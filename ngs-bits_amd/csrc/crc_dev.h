// CRC-32 (gzip) on the device, shared by the member check of K1 (crc.hip) and the BGZF writer (deflate.hip): the polynomial, the layout of the constant
// tables crc.hip builds and uploads once per device, and the GF(2) multiplication that combines the states of independent pieces of a message.
#pragma once
#include "common.h"

namespace ngsqc {

constexpr uint32_t CRC_POLY = 0xEDB88320u;   // reflected CRC-32 (gzip)
constexpr int CRC_ROUND = 4096, CRC_PIECE = 64;
constexpr int TAB_SLICE = 0, TAB_GAP = 1024, TAB_LANE = 2048, TAB_INIT = 2048 + 64, TAB_GAP2 = TAB_INIT + 65537, TAB_GAP4 = TAB_GAP2 + 1024, TAB_ADV = TAB_GAP4 + 1024, TAB_TOTAL = TAB_ADV + 1024;
// TAB_SLICE + 256 k + x: the state of byte x followed by k zero bytes (k = 0: the byte table of a bytewise CRC); TAB_INIT + m: x^(8 m) * 0xFFFFFFFF (the initial
// value's share of a message of m bytes); TAB_GAP / TAB_GAP2 / TAB_GAP4: a state advanced over the zero bytes between a chain's pieces in rounds of 4 / 8 / 16 KiB;
// TAB_ADV: over 4 KiB (folds a lane's chains)

__device__ __forceinline__ uint32_t gf_mul(uint32_t a, uint32_t b)   // a * b mod P, reflected representation (x^0 = 0x80000000)
{
	uint32_t p = 0;
	#pragma unroll
	for (int i = 31; i >= 0; --i)
	{
		p ^= (a >> i) & 1u ? b : 0u;
		b = (b >> 1) ^ ((b & 1u) ? CRC_POLY : 0u);
	}
	return p;
}

// x^(8 m) mod P: the map that advances a state over m zero bytes (square and multiply; m < 2^17)
__device__ __forceinline__ uint32_t gf_x8(uint32_t m)
{
	uint32_t r = 0x80000000u, sq = 0x00800000u;   // x^0, x^8
	for (int i = 0; i < 17; ++i)
	{
		if ((m >> i) & 1u) r = gf_mul(r, sq);
		sq = gf_mul(sq, sq);
	}
	return r;
}

const uint32_t* crc_device_tables();   // TAB_TOTAL words on the current device (crc.hip)

} // namespace ngsqc
