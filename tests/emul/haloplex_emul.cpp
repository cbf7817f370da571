// BamCleanHaloplex's decision for a record (ngs-bits_amd/csrc/haloplex_visit.h: the text the GPU library compiles into its verdict kernels) on the CPU:
// tests/test_cpu_bamcleanhaloplex_emul.py runs it over BAM records against the Python restatement. Test infrastructure, never linked into the library.
#include <cstddef>
#include <cstdint>
#include <cstring>
#define NGSQC_REC_ON_CPU
#include "device_on_cpu.h"
#include "../../ngs-bits_amd/csrc/haloplex_visit.h"

using namespace ngsqc;

extern "C" {

int32_t haloplex_lane_ops() { return (int32_t)HX_LANE_OPS; }

// Per record i at infl + recoff[i]: verdict[i] by one thread (hx_visit); sum_whole[i] / sum_sliced[i]: the M sum of the effective CIGAR taken whole and as the
// 64 strided slices of a wave's lanes added up (-1 for a record that is no candidate); cut[i]: the verdict as the verdict kernel and the long kernel split the
// work (whole in the lane up to HX_LANE_OPS operations, sliced above). patched: the record's bytes with the flag word as the gather stores it (the source's
// layout: the mask OR-ed into bytes 18 and 19, one byte at a time), laid end to end.
void haloplex_emul(const uint8_t* infl, const int64_t* recoff, int64_t n, int32_t min_match, uint8_t* verdict, int64_t* sum_whole, int64_t* sum_sliced, uint8_t* cut, uint8_t* patched)
{
	size_t o = 0;
	for (int64_t i = 0; i < n; ++i)
	{
		const RecView r = load_rec(infl, recoff[i]);
		const size_t size = (size_t)r.bs + 4;
		verdict[i] = hx_visit(r, min_match);
		sum_whole[i] = sum_sliced[i] = -1; cut[i] = HX_NOT_CANDIDATE;
		if (hx_candidate(r.flag))
		{
			RecView e = r; rec_apply_cg(e);
			sum_whole[i] = hx_match_sum(e.cigar, e.n_cigar, 0, 1);
			long long s = 0;
			for (uint32_t lane = 0; lane < 64; ++lane) s += hx_match_sum(e.cigar, e.n_cigar, lane, 64);
			sum_sliced[i] = s;
			cut[i] = hx_verdict(true, e.n_cigar > HX_LANE_OPS ? s : sum_whole[i], min_match);
		}
		memcpy(patched + o, infl + recoff[i], size);
		const uint32_t mask = hx_flag_mask(verdict[i]);
		patched[o + 18] |= (uint8_t)mask; patched[o + 19] |= (uint8_t)(mask >> 8);
		o += size;
	}
}
}
