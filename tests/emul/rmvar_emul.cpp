// BamRemoveVariants' visit of a record (ngs-bits_amd/csrc/rmvar_visit.h: the text the GPU library compiles into its verdict and gather kernels) on the CPU:
// tests/test_cpu_bamremovevariants_emul.py runs it over BAM records against the Python restatement. Test infrastructure, never linked into the library.
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>
#define NGSQC_REC_ON_CPU
#include "device_on_cpu.h"
#include "../../ngs-bits_amd/csrc/rmvar_visit.h"

using namespace ngsqc;

extern "C" {

// v / maxend / tid_first: the table as the library lays it out (lines grouped by tid in file order, the running maximum of end, n_ref + 1 range starts).
// Per record i at infl + recoff[i]: verdict[i] (bit 0 passes, 1 modified, 2 skipped, 3 error; bits 4-5 the error code), ev[i] (line or base of the error), and with
// patched != null the record's bytes with the sequence as the gather kernel stores it (the source's layout), laid end to end.
void rmvar_emul(const uint8_t* infl, const int64_t* recoff, int64_t n, const ngsqc_rm_variant* v, const int32_t* maxend, const int32_t* tid_first, int32_t n_ref,
                int32_t mask, int32_t keep_indels, uint8_t* verdict, int32_t* ev, uint8_t* patched)
{
	const RmTable T{v, maxend, tid_first, n_ref};
	const RmMode m{mask, 0, keep_indels};
	size_t o = 0;
	for (int64_t i = 0; i < n; ++i)
	{
		const RecView raw = load_rec(infl, recoff[i]);
		const size_t size = (size_t)raw.bs + 4;
		if (patched) memcpy(patched + o, infl + recoff[i], size);
		if (raw.flag & 0x900) { verdict[i] = V_SKIP; ev[i] = -1; o += size; continue; }
		RecView r = raw; rec_apply_cg(r);
		const Verdict vd = visit_seq(r, T, m);
		verdict[i] = (uint8_t)vd.bits; ev[i] = vd.ev;
		Span sp;
		if (patched && (vd.bits & V_MOD) && rec_span(r, T, sp))
		{
			int bad = -1;
			const size_t seq = 36 + raw.l_name + 4ull * raw.n_cigar_raw;
			for (int32_t q = sp.a; q < vd.E; ++q)
			{
				const LineOut lo = eval_line(r, T, sp, q, m, bad);
				if (lo.code == L_SNV) patched[o + seq + (size_t)(lo.ap >> 1)] = patched_byte(r, T, sp, vd.E, lo.ap);
			}
		}
		o += size;
	}
}
}
