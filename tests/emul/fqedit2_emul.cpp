// The per-entry text of FastqExtractBarcode, FastqAddBarcode, FastqDownsample and FastqConcat (ngs-bits_amd/csrc/fqedit_visit.h: what the GPU library compiles
// into the kernels of csrc/fqedit.hip) on the CPU: tests/test_cpu_fqedit2_emul.py runs it over FASTQ texts against the Python model (tests/fqedit2_oracle.py).
// The work is cut as the kernels cut it - a lane per entry for the plan, stream k reading the side fe_shape names, the output text put together byte by byte
// with fe_entry_byte as fe_format_kernel does, the kept headers by sizes, exclusive positions and copy as fe_header_sizes_kernel / fe_header_copy_kernel do.
// One call is one feed that ends a file. The keep bytes come from the caller: the generator is the device's (csrc/downsample.hip) and is tested there.
// Test infrastructure, never linked into the library.
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>
#include "../../ngs-bits_amd/csrc/fqedit_visit.h"

using namespace ngsqc;

namespace {
struct Lines { std::vector<uint32_t> at; uint64_t L = 0; };
Lines index_lines(const uint8_t* t, int64_t n)
{
	Lines l; l.at.push_back(0);
	for (int64_t i = 0; i < n; ++i) if (t[i] == '\n') l.at.push_back((uint32_t)(i + 1));
	l.L = l.at.size() - 1; l.at.push_back((uint32_t)n);
	return l;
}
struct Sides
{
	FeShape sh; const uint8_t* text[FE_MAX_SIDES]; Lines ln[FE_MAX_SIDES];
	Sides(int op, const uint8_t* const* t, const int64_t* n) : sh(fe_shape(op)) { for (int k = 0; k < sh.sides; ++k) { text[k] = t[k]; ln[k] = index_lines(t[k], n[k]); } }
	FqEntry entry(int side, uint64_t r) const { return fq_entry(text[side], ln[side].at.data(), ln[side].L, r); }
};
FeIns ins_of(const Sides& s, int op, uint64_t r) { return op == FE_OP_BARCODE_ADD ? fe_ins_barcode(s.text[2], s.entry(2, r)) : FeIns{}; }
}

// t, n: the texts of the op's sides, each the last piece of its file. cut: BARCODE_CUT. keep: one byte per entry (DOWNSAMPLE). plan: [cap][streams][8].
// out: entries, then the entries of every side. -1: plan too small.
extern "C" int32_t fqedit2_emul(const uint8_t* const* t, const int64_t* n, int32_t op, int32_t cut, const uint8_t* keep, int32_t* plan, int64_t cap, uint64_t* out)
{
	const Sides s(op, t, n);
	uint64_t m = ~0ull;
	for (int k = 0; k < s.sh.sides; ++k) { out[1 + k] = (s.ln[k].L + 3) / 4; m = std::min(m, out[1 + k]); }
	if ((int64_t)m > cap) return -1;
	for (uint64_t r = 0; r < m; ++r)
	{
		const FqEntry e = s.entry(0, r);
		int32_t* row = plan + (uint64_t)FE_PLAN * s.sh.streams * r;
		if (op == FE_OP_COPY) fe_plan_keep(row, 1u, e.bases.len, e.quals.len);
		else if (op == FE_OP_BARCODE_CUT)
		{
			fe_plan_barcode_main(row, (uint32_t)cut, e.bases.len, e.quals.len);
			fe_plan_barcode_index(row + FE_PLAN, (uint32_t)cut, e.bases.len, e.quals.len);
		}
		else if (op == FE_OP_DOWNSAMPLE)
		{
			const FqEntry e2 = s.entry(1, r);
			fe_plan_keep(row, keep[r], e.bases.len, e.quals.len);
			fe_plan_keep(row + FE_PLAN, keep[r], e2.bases.len, e2.quals.len);
		}
		else if (op == FE_OP_BARCODE_ADD)
		{
			const uint32_t len3 = s.entry(2, r).bases.len;
			fe_plan_addbarcode(row, s.text[0], e, len3);
			fe_plan_addbarcode(row + FE_PLAN, s.text[1], s.entry(1, r), len3);
		}
		else return -2;
	}
	out[0] = m;
	return 0;
}

// the text of output stream k: -> its length, -1 when it does not fit
extern "C" int64_t fqedit2_format(const uint8_t* const* t, const int64_t* n, int32_t op, const int32_t* plan, int64_t entries, int32_t k, uint8_t* buf, int64_t cap)
{
	const Sides s(op, t, n);
	const int side = s.sh.src[k];
	int64_t at = 0;
	for (int64_t r = 0; r < entries; ++r)
	{
		const FqEntry e = s.entry(side, (uint64_t)r);
		const int32_t* row = plan + FE_PLAN * ((int64_t)s.sh.streams * r + k);
		const uint64_t size = fe_entry_bytes(row, e);
		if (at + (int64_t)size > cap) return -1;
		const FeIns u = ins_of(s, op, (uint64_t)r);
		for (uint64_t x = 0; x < size; ++x) buf[at + (int64_t)x] = fe_entry_byte(s.text[side], e, row, x, u);
		at += (int64_t)size;
	}
	return at;
}

// the header lines of the kept pairs: sizes, exclusive positions, then the 64 lanes of a wave copy each line. -> the length, -1 when it does not fit
extern "C" int64_t fqedit2_headers(const uint8_t* const* t, const int64_t* n, int32_t op, const int32_t* plan, int64_t entries, uint8_t* buf, int64_t cap)
{
	const Sides s(op, t, n);
	std::vector<uint64_t> hsz((size_t)entries), hoff((size_t)entries);
	uint64_t tot = 0;
	for (int64_t r = 0; r < entries; ++r) { hsz[(size_t)r] = fe_header_bytes(plan + FE_PLAN * (int64_t)s.sh.streams * r, s.entry(0, (uint64_t)r)); hoff[(size_t)r] = tot; tot += hsz[(size_t)r]; }
	if ((int64_t)tot > cap) return -1;
	for (int64_t r = 0; r < entries; ++r)
	{
		const FqEntry e = s.entry(0, (uint64_t)r);
		for (uint64_t lane = 0; lane < 64; ++lane)
			for (uint64_t x = lane; x < hsz[(size_t)r]; x += 64) buf[hoff[(size_t)r] + x] = fe_header_byte(s.text[0], e, x);
	}
	return (int64_t)tot;
}
