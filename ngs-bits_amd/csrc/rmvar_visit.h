// The visit of one record to the variant lines it overlaps, as BamRemoveVariants' alignment_pass / mask_alignment make it (src/BamRemoveVariants/main.cpp:34-110):
// the text csrc/rmvar.hip compiles into its kernels, kept free of HIP so that tests/emul/rmvar_emul.cpp runs the same text on the CPU against the Python
// restatement (NGSQC_REC_ON_CPU). One thread's work throughout; the wave-wide forms and the kernels are rmvar.hip's.
#pragma once
#include "rec.h"
#include "../../include/ngsqc.h"

namespace ngsqc {
namespace {
struct RmTable { const ngsqc_rm_variant* v; const int32_t* maxend; const int32_t* tid_first; int32_t n_ref; };
struct RmMode { int32_t mask, single_end, keep_indels; };
struct Span { int32_t a, last; long long rs, re; bool only_ins; };   // candidate lines [a, last) (those with beg <= re), the record's [start, end] 1-based
enum { L_NONE = 0, L_SNV = 1, L_OTHER = 2, L_ERR = 4 };
struct LineOut { int code, err, ap; uint32_t old_nib, ref_nib; };
constexpr uint8_t V_PASS = 1, V_MOD = 2, V_SKIP = 4, V_ERR = 8;   // (bits 4-5 of the device's byte: the error code)

__device__ __forceinline__ uint32_t base_nib(uint8_t c) { return c == 'A' ? 1u : c == 'C' ? 2u : c == 'G' ? 4u : c == 'T' ? 8u : 0u; }
__device__ __forceinline__ const uint8_t* rec_seq(const RecView& r) { return r.core + 32 + r.l_name + 4ull * r.n_cigar_raw; }
__device__ __forceinline__ uint32_t seq_nib(const RecView& r, int i) { return (rec_seq(r)[i >> 1] >> ((~i & 1) << 2)) & 15u; }

// the record's span (bam_endpos) and its candidate lines; false: it overlaps nothing
__device__ bool rec_span(const RecView& r, const RmTable& T, Span& sp)
{
	if (r.tid < 0 || r.tid >= T.n_ref || r.pos < 0) return false;
	const int32_t first = T.tid_first[r.tid], last = T.tid_first[r.tid + 1];
	if (first >= last) return false;
	// one pass over the CIGAR with a fixed trip count (a walk that left the loop at the first other operation gave wrong answers on the device): the reference length (bam_endpos: 0 with flag 4) and cigarIsOnlyInsertion (BamReader.cpp:90-100: I and S alone; true without a CIGAR)
	long long ref_len = 0; uint32_t other = 0;
	for (uint32_t k = 0; k < r.n_cigar; ++k)
	{
		const uint32_t c = ld32(r.cigar + 4ull * k), op = c & 15u;
		if ((0x18Du >> op) & 1u) ref_len += c >> 4;
		other |= (op != 1u && op != 4u) ? 1u : 0u;
	}
	if (r.flag & 4) ref_len = 0;
	sp.only_ins = other == 0;
	sp.rs = (long long)r.pos + 1; sp.re = (long long)r.pos + (ref_len > 0 ? ref_len : 1);
	int32_t lo = first, hi = last;
	while (lo < hi) { const int32_t m = (lo + hi) >> 1; if (T.maxend[m] < sp.rs) lo = m + 1; else hi = m; }
	sp.a = lo; sp.last = last;
	return lo < last && T.v[lo].beg <= sp.re;
}

// extractBaseByCIGAR (BamReader.cpp:307-374): the read index of 1-based genome position pos; -1: no base ('~', '-', or an index outside the read); -2: the walk ends in front of pos (:373)
__device__ int snv_index(const RecView& r, bool only_ins, long long pos)
{
	if (only_ins) return -1;
	long long rp = 0, gp = r.pos;
	for (uint32_t k = 0; k < r.n_cigar; ++k)
	{
		const uint32_t c = ld32(r.cigar + 4ull * k), op = c & 15u; const long long len = c >> 4;
		if (op == 0u || op == 7u || op == 8u) { gp += len; rp += len; }
		else if (op == 1u) rp += len;
		else if (op == 2u || op == 3u) { gp += len; if (gp >= pos) return -1; }
		else if (op == 4u) { rp += len; if (rp >= r.l_seq) return -1; }
		if (gp >= pos) { const long long ap = rp - (gp + 1 - pos); return ap >= 0 && ap < r.l_seq ? (int)ap : -1; }
	}
	return -2;
}

// extractIndelsByCIGAR(pos, 50) is non-empty (BamReader.cpp:376-439)
__device__ bool has_indel(const RecView& r, long long pos)
{
	const long long ws = pos - 50, we = pos + 50;
	long long gp = (long long)r.pos + 1;
	for (uint32_t k = 0; k < r.n_cigar; ++k)
	{
		const uint32_t c = ld32(r.cigar + 4ull * k), op = c & 15u; const long long len = c >> 4;
		if (op == 0u || op == 7u || op == 8u || op == 3u) gp += len;
		else if (op == 1u || op == 2u) { if (gp >= ws && gp <= we) return true; if (op == 2u) gp += len; }
		if (gp > we) break;
	}
	return false;
}

// the base at read index p as line k of a -mask visit finds it: the source's, then what the carried SNV lines in front of k stored there
__device__ uint32_t nib_at(const RecView& r, const RmTable& T, const Span& sp, int32_t k, int p)
{
	uint32_t nib = seq_nib(r, p);
	for (int32_t j = sp.a; j < k; ++j)
	{
		const ngsqc_rm_variant v = T.v[j];
		if (v.kind != NGSQC_RMVAR_SNV || v.end < sp.rs) continue;
		if (snv_index(r, sp.only_ins, v.start) == p && nib == base_nib(v.obs)) nib = base_nib(v.ref);
	}
	return nib;
}

// setBases (BamReader.cpp:161-168) stores A, C, G, T, N alone: the first other base of the read, or -1
__device__ int first_bad_base(const RecView& r)
{
	for (int i = 0; i < r.l_seq; ++i) { const uint32_t b = seq_nib(r, i); if (b != 1u && b != 2u && b != 4u && b != 8u && b != 15u) return i; }
	return -1;
}

// line k of the visit (beg <= re is the caller's); bad: the cached first_bad_base (-2: not looked up yet)
__device__ LineOut eval_line(const RecView& r, const RmTable& T, const Span& sp, int32_t k, const RmMode& m, int& bad)
{
	LineOut o{L_NONE, 0, -1, 0, 0};
	const ngsqc_rm_variant v = T.v[k];
	if (v.end < sp.rs) return o;
	if (v.kind == NGSQC_RMVAR_INVALID) { o.code = L_ERR; o.err = NGSQC_RMERR_INVALID_LINE; o.ap = k; return o; }
	if (v.kind == NGSQC_RMVAR_OTHER) { if (has_indel(r, v.start)) o.code = L_OTHER; return o; }
	const int ap = snv_index(r, sp.only_ins, v.start);
	if (ap == -2) { o.code = L_ERR; o.err = NGSQC_RMERR_POS_NOT_FOUND; o.ap = k; return o; }
	if (ap < 0) return o;
	const uint32_t nib = m.mask ? nib_at(r, T, sp, k, ap) : seq_nib(r, ap);
	if (nib != base_nib(v.obs)) return o;
	if (m.mask)
	{
		if (bad == -2) bad = first_bad_base(r);
		if (bad >= 0) { o.code = L_ERR; o.err = NGSQC_RMERR_BAD_BASE; o.ap = bad; return o; }
	}
	o.code = L_SNV; o.ap = ap; o.old_nib = nib; o.ref_nib = base_nib(v.ref);
	return o;
}

struct Verdict { uint32_t bits; int32_t ev; int32_t E; };   // bits: V_*, the error code << 4; ev: the line (BAD_BASE: the base) of the error; E: the visit covered the lines [a, E)

// the visit of one record by one thread
__device__ Verdict visit_seq(const RecView& r, const RmTable& T, const RmMode& m)
{
	Verdict out{V_PASS, -1, 0};
	Span sp;
	if (!rec_span(r, T, sp)) return out;
	bool pass = true; int eff = 0, bad = -2; int32_t k = sp.a;
	for (; k < sp.last && T.v[k].beg <= sp.re; ++k)
	{
		const LineOut o = eval_line(r, T, sp, k, m, bad);
		if (o.code == L_ERR) { out.bits = V_ERR | (uint32_t)o.err << 4; out.ev = o.ap; out.E = k; return out; }
		if (o.code == L_SNV) { if (!m.mask) { pass = false; break; } if (o.old_nib != o.ref_nib) ++eff; }
		else if (o.code == L_OTHER) { pass = m.mask && m.keep_indels; break; }
	}
	out.E = k;
	bool mod = eff == 1;
	if (eff > 1)   // (a base may have been set twice, back to what it was: the reference compares the whole sequence, :159, :199, :239)
		for (int32_t q = sp.a; q < k && !mod; ++q)
		{
			const LineOut o = eval_line(r, T, sp, q, m, bad);
			mod = o.code == L_SNV && nib_at(r, T, sp, k, o.ap) != seq_nib(r, o.ap);
		}
	out.bits = (pass ? V_PASS : 0) | (mod ? V_MOD : 0);
	return out;
}

// the byte of the sequence that holds read index ap once the visit has covered the lines [a, E): both nibbles from the source and the lines, never from a copy
__device__ uint8_t patched_byte(const RecView& r, const RmTable& T, const Span& sp, int32_t E, int ap)
{
	const int p0 = ap & ~1, p1 = ap | 1;
	const uint32_t hi = nib_at(r, T, sp, E, p0), lo = p1 < r.l_seq ? nib_at(r, T, sp, E, p1) : (rec_seq(r)[p0 >> 1] & 15u);
	return (uint8_t)(hi << 4 | lo);
}
} // namespace
} // namespace ngsqc
