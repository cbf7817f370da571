// The decision of BamCleanHaloplex for one record (src/BamCleanHaloplex/main.cpp:44-58): the candidate test, the sum of the CIGAR's M lengths, the verdict byte
// and the flag bits of a failed record - the text csrc/haloplex.hip compiles into its kernels, kept free of HIP so that tests/emul/haloplex_emul.cpp runs the
// same text on the CPU against the Python restatement (NGSQC_REC_ON_CPU). Plain integer code over RecView.
#pragma once
#include "rec.h"

namespace ngsqc {
namespace {
constexpr uint8_t HX_NOT_CANDIDATE = 0, HX_KEPT = 1, HX_FAILED = 2;   // the verdict byte
constexpr uint32_t HX_EXCLUDING = 0x4u | 0x100u | 0x400u | 0x800u;    // unmapped, secondary, duplicate, supplementary (:44)
constexpr uint32_t HX_FAIL_FLAGS = 0x4u | 0x100u;                     // setIsUnmapped(true), setIsSecondaryAlignment(true) (:56-57): a candidate has neither bit

// A CIGAR of at most HX_LANE_OPS operations is summed by the lane that owns the record; a longer one goes to a wave (csrc/haloplex.hip)
constexpr uint32_t HX_LANE_OPS = 32;

__device__ __forceinline__ bool hx_candidate(uint32_t flag) { return !(flag & HX_EXCLUDING); }

// The lengths of the M operations (op 0 alone: '=' and 'X' do not count, :51) among the operations first, first + step, first + 2 step, ... below n of the
// CIGAR at `cigar`. (0, 1) is the whole CIGAR; (lane, 64) is a lane's share of a wave's. 64 bits: fewer than 2^29 operations of less than 2^28 each.
__device__ __forceinline__ long long hx_match_sum(const uint8_t* cigar, uint32_t n, uint32_t first, uint32_t step)
{
	long long sum = 0;
	for (uint32_t k = first; k < n; k += step)
	{
		const uint32_t c = ld32(cigar + 4ull * k);
		sum += (c & 15u) == 0u ? (long long)(c >> 4) : 0ll;
	}
	return sum;
}

__device__ __forceinline__ uint8_t hx_verdict(bool candidate, long long sum_m, int32_t min_match)
{
	return !candidate ? HX_NOT_CANDIDATE : sum_m < (long long)min_match ? HX_FAILED : HX_KEPT;
}

// what is OR-ed into the flag word of the written record
__device__ __forceinline__ uint32_t hx_flag_mask(uint8_t verdict) { return verdict == HX_FAILED ? HX_FAIL_FLAGS : 0u; }

// the whole decision by one thread: r as load_rec gives it
__device__ __forceinline__ uint8_t hx_visit(const RecView& r, int32_t min_match)
{
	if (!hx_candidate(r.flag)) return HX_NOT_CANDIDATE;
	RecView e = r; rec_apply_cg(e);
	return hx_verdict(true, hx_match_sum(e.cigar, e.n_cigar, 0, 1), min_match);
}
} // namespace
} // namespace ngsqc
