// The bytes BamWriter::writeAlignment writes for a record (src/cppNGS/BamWriter.cpp over htslib's bam_write1), shared by the tools that gather records into a
// BAM output stream (BamFilter: pairs.hip, BamDownsample: downsample.hip, and the writers after them): the size a record takes in the output and the wave-wide
// copy into a window, with bits OR-ed into the copy's flag word where a tool asks for it (BamCleanHaloplex: haloplex.hip).
#pragma once
#include "join.h"

namespace ngsqc {
namespace {
// bin of htslib's hts_reg2bin(beg, end, 14, 5)
__device__ __forceinline__ uint32_t reg2bin(int64_t beg, int64_t end)
{
	--end;
	if (beg >> 14 == end >> 14) return (uint32_t)(((1 << 15) - 1) / 7 + (beg >> 14));
	if (beg >> 17 == end >> 17) return (uint32_t)(((1 << 12) - 1) / 7 + (beg >> 17));
	if (beg >> 20 == end >> 20) return (uint32_t)(((1 << 9) - 1) / 7 + (beg >> 20));
	if (beg >> 23 == end >> 23) return (uint32_t)(((1 << 6) - 1) / 7 + (beg >> 23));
	if (beg >> 26 == end >> 26) return (uint32_t)(((1 << 3) - 1) / 7 + (beg >> 26));
	return 0;
}

// A record whose CIGAR comes from its CG tag (rec_apply_cg) is written as htslib's bam_write1 writes what bam_read1 made of it: up to 65535 operations inline and
// without the tag, more as the placeholder "l_seq S, ref_len N" with CG:B,I appended behind the other tags; bin from the real span in both cases.
struct CgInfo { const uint8_t* ops; uint32_t n; const uint8_t* tag; };   // ops: the tag's array; tag: the tag's first byte (its length is 8 + 4 n)
__device__ __forceinline__ bool cg_of(const RecView& r, CgInfo& g)
{
	RecView e = r; rec_apply_cg(e);
	if (e.cigar == r.cigar) return false;
	g.ops = e.cigar; g.n = e.n_cigar; g.tag = e.cigar - 8;
	return true;
}
// e: r behind rec_apply_cg (a caller that needs the effective CIGAR anyway scans the tags once)
__device__ __forceinline__ uint32_t out_size(const RecView& r, const RecView& e)
{
	if (e.cigar == r.cigar) return r.bs + 4;
	return e.n_cigar <= 65535 ? r.bs + 4 - 4 * r.n_cigar_raw - 8 : r.bs + 4 - 4 * r.n_cigar_raw + 8;
}
__device__ __forceinline__ uint32_t out_size(const RecView& r)
{
	RecView e = r; rec_apply_cg(e);
	return out_size(r, e);
}

// one record into the output window at pos (wave-wide). flag_or: bits OR-ed into the flag word of the copy (bytes 18-19 of the record, block_size included); each
// of the two bytes is stored by whoever stores that byte of the copy, and only where it lies inside the window: a record that straddles two windows gets its
// low flag byte in one launch and its high one in the other. 0 (the default): the copy is the source's bytes
__device__ void write_record(const uint8_t* __restrict__ s, const Win& w, int64_t pos, int lane, uint32_t flag_or = 0)
{
	const RecView r = load_rec(s, 0);
	CgInfo g;
	if (!cg_of(r, g))
	{
		const int64_t n = (int64_t)r.bs + 4, a = max<int64_t>(0, w.lo - pos), b = min<int64_t>(n, w.hi - pos);
		if (!flag_or) { for (int64_t i = a + lane; i < b; i += 64) w.base[pos + i] = s[i]; return; }
		for (int64_t i = a + lane; i < b; i += 64) w.base[pos + i] = (uint8_t)(s[i] | (i == 18 ? flag_or : i == 19 ? flag_or >> 8 : 0u));
		return;
	}
	if (lane) return;   // (rare: long reads only)
	const uint32_t osz = out_size(r);
	uint32_t rlen = 0;
	for (uint32_t i = 0; i < g.n; ++i) { const uint32_t c = ld32(g.ops + 4ull * i), op = c & 15u; if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) rlen += c >> 4; }
	const int64_t end = (int64_t)r.pos + ((r.flag & 4) || rlen == 0 ? 1 : rlen);
	const bool inl = g.n <= 65535;
	const uint32_t bs = osz - 4, bin = reg2bin(r.pos, end), nc = inl ? g.n : 2;
	uint8_t fixed[36];
	for (int i = 0; i < 36; ++i) fixed[i] = s[i];
	for (int i = 0; i < 4; ++i) fixed[i] = (uint8_t)(bs >> (8 * i));
	fixed[14] = (uint8_t)bin; fixed[15] = (uint8_t)(bin >> 8); fixed[16] = (uint8_t)nc; fixed[17] = (uint8_t)(nc >> 8);
	fixed[18] |= (uint8_t)flag_or; fixed[19] |= (uint8_t)(flag_or >> 8);   // (put() keeps each byte to the window)
	int64_t o = pos;
	for (int i = 0; i < 36; ++i) put(w, o, fixed[i]);
	for (uint32_t i = 0; i < r.l_name; ++i) put(w, o, s[36 + i]);
	if (inl) for (uint32_t i = 0; i < 4 * g.n; ++i) put(w, o, g.ops[i]);
	else
	{
		const uint32_t c0 = (uint32_t)r.l_seq << 4 | 4u, c1 = rlen << 4 | 3u;
		for (int i = 0; i < 4; ++i) put(w, o, (uint8_t)(c0 >> (8 * i)));
		for (int i = 0; i < 4; ++i) put(w, o, (uint8_t)(c1 >> (8 * i)));
	}
	const uint8_t* sq = r.cigar + 4ull * r.n_cigar_raw;   // seq, qual, aux
	const uint8_t* tag0 = g.tag; const uint8_t* tag1 = g.tag + 8 + 4ull * g.n; const uint8_t* e = rec_end(r);
	for (const uint8_t* x = sq; x < tag0; ++x) put(w, o, *x);
	for (const uint8_t* x = tag1; x < e; ++x) put(w, o, *x);
	if (!inl) for (const uint8_t* x = tag0; x < tag1; ++x) put(w, o, *x);
}
} // namespace
} // namespace ngsqc
