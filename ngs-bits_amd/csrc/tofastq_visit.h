// BamToFastq's decisions for one record and the bytes of one FASTQ entry (src/BamToFastq/main.cpp:77-214): the region rule, the entry's size with the NUL
// cut-off of gzputs and the "would throw" bit, the entry byte by byte, and a lane's share of the entry inside an output window - the text csrc/fastq.hip
// compiles into its kernels, kept free of HIP so that tests/emul/tofastq_emul.cpp runs the same text on the CPU against the Python restatement
// (NGSQC_REC_ON_CPU; the CPU build supplies __constant__, max and min). The name of the "@" line is join_visit.h's: the bytes in front of the first NUL.
#pragma once
#include "join_visit.h"

namespace ngsqc {
namespace {
constexpr uint32_t INFO_KEPT = 0x80000000u, INFO_THROWS = 0x40000000u, INFO_SIZE = 0x3fffffffu;

__constant__ char c_nt16[16] = {'=', 'A', 'C', 'M', 'G', 'R', 'S', 'V', 'T', 'W', 'Y', 'H', 'K', 'D', 'B', 'N'};
__constant__ char c_comp16[16] = {'N', 'T', 'G', 'N', 'C', 'N', 'N', 'N', 'A', 'N', 'N', 'N', 'N', 'N', 'N', 'N'};   // (only ACGTN have a complement: the rest throws)

__device__ __forceinline__ int base_code(const uint8_t* seq, int j) { return (seq[j >> 1] >> ((~j & 1) << 2)) & 15; }
__device__ __forceinline__ bool has_complement(int c) { return c == 1 || c == 2 || c == 4 || c == 8 || c == 15; }

// bam_endpos of htslib (the effective CIGAR; an unmapped record or an empty span counts one base)
__device__ int64_t rec_endpos(RecView r)
{
	rec_apply_cg(r);
	int64_t rlen = 0;
	if (!(r.flag & 4))
		for (uint32_t i = 0; i < r.n_cigar; ++i) { const uint32_t c = ld32(r.cigar + 4ull * i), op = c & 15u; if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) rlen += c >> 4; }
	return (int64_t)r.pos + (rlen ? rlen : 1);
}

// htslib's iterator rule for -reg (sam_itr_queryi(idx, tid, start - 1, end)): the region 1-based closed
__device__ __forceinline__ bool fq_in_region(const RecView& r, int32_t reg_tid, int32_t reg_start, int32_t reg_end)
{
	return r.tid == reg_tid && r.pos < reg_end && rec_endpos(r) > (int64_t)reg_start - 1;
}

// the info word of a record's entry: its size | INFO_KEPT | INFO_THROWS. The entry: header, bases (extended), "+", qualities up to the first NUL of the
// oriented, extended line; throws: a reverse-strand record with a base the complement does not know. nl: the name's length (name_len; the keys kernel has it
// from name_hash_z)
__device__ __forceinline__ uint32_t fq_entry_info(const RecView& r, int extend, int nl)
{
	const int L = max(r.l_seq, extend);
	const uint8_t* qu = rec_qual(r); const uint8_t* sq = r.cigar + 4ull * r.n_cigar_raw;
	const bool rev = (r.flag & 0x10) != 0;
	int qcut = L;
	if (!rev) { for (int j = 0; j < r.l_seq; ++j) if (qu[j] == 223) { qcut = j; break; } }
	else { for (int j = r.l_seq - 1; j >= 0; --j) if (qu[j] == 223) { qcut = r.l_seq - 1 - j; break; } }
	bool throws = false;
	if (rev) for (int j = 0; j < r.l_seq && !throws; ++j) throws = !has_complement(base_code(sq, j));
	return (uint32_t)(nl + L + qcut + 6) | INFO_KEPT | (throws ? INFO_THROWS : 0u);
}

// the bytes of an entry: "@name\n" BASES "\n+\n" QUALS "\n"; qcut: the quality bytes gzputs writes (up to the first NUL)
struct FqEntry { const uint8_t* name; const uint8_t* seq; const uint8_t* qual; int nl, lseq, L, qcut; bool rev; };
__device__ __forceinline__ FqEntry fq_entry(const uint8_t* rec, uint32_t size, int extend)
{
	const RecView r = load_rec(rec, 0);
	FqEntry e;
	e.nl = name_len(r.core + 32, r.l_name); e.name = r.core + 32; e.lseq = r.l_seq; e.L = max(r.l_seq, extend);
	e.seq = r.cigar + 4ull * r.n_cigar_raw; e.qual = rec_qual(r); e.rev = (r.flag & 0x10) != 0;
	e.qcut = (int)size - (e.nl + e.L + 6);
	return e;
}
__device__ __forceinline__ uint8_t fq_byte(const FqEntry& e, int k)
{
	if (k == 0) return '@';
	k -= 1; if (k < e.nl) return e.name[k];
	k -= e.nl; if (k == 0) return '\n';
	k -= 1;
	if (k < e.L)
	{
		if (k >= e.lseq) return 'N';
		return e.rev ? (uint8_t)c_comp16[base_code(e.seq, e.lseq - 1 - k)] : (uint8_t)c_nt16[base_code(e.seq, k)];
	}
	k -= e.L;
	if (k == 0 || k == 2) return '\n';
	if (k == 1) return '+';
	k -= 3;
	if (k < e.qcut) return k >= e.lseq ? (uint8_t)'#' : (uint8_t)(e.qual[e.rev ? e.lseq - 1 - k : k] + 33);
	return '\n';
}

// the part [a, b) of an entry of `size` bytes at window position pos that falls inside the window [lo, hi), and its whole dwords [d0, d1)
struct FqSplit { int64_t a, d0, d1, b; };
__device__ __forceinline__ FqSplit fq_split(int64_t pos, int64_t size, int64_t lo, int64_t hi)
{
	FqSplit s;
	s.a = max(pos, lo); s.b = min(pos + size, hi);
	s.d0 = (s.a + 3) & ~3ll; s.d1 = s.b & ~3ll;
	return s;
}

// one lane of the wave that writes the entry (s.a < s.b): whole dwords where they can, single bytes at the ends; base is aligned to 4 bytes
__device__ __forceinline__ void fq_format_lane(const FqEntry& e, int64_t pos, const FqSplit& s, int lane, uint8_t* base)
{
	const int64_t a = s.a, b = s.b, d0 = s.d0, d1 = s.d1;
	if (d0 >= d1)
	{
		for (int64_t x = a + lane; x < b; x += 64) base[x] = fq_byte(e, (int)(x - pos));
		return;
	}
	if (lane < d0 - a) base[a + lane] = fq_byte(e, (int)(a + lane - pos));
	if (lane >= 8 && lane - 8 < b - d1) base[d1 + lane - 8] = fq_byte(e, (int)(d1 + lane - 8 - pos));
	uint32_t* dw = reinterpret_cast<uint32_t*>(base);
	for (int64_t x = d0 + 4 * lane; x < d1; x += 256)
	{
		const int k = (int)(x - pos);
		dw[x >> 2] = (uint32_t)fq_byte(e, k) | (uint32_t)fq_byte(e, k + 1) << 8 | (uint32_t)fq_byte(e, k + 2) << 16 | (uint32_t)fq_byte(e, k + 3) << 24;
	}
}
} // namespace
} // namespace ngsqc
