// The BAM record as the device kernels read it (scan.hip, indel.hip): the fixed fields, the effective CIGAR, the aux scan, a wave reduction.
#pragma once
#ifdef NGSQC_REC_ON_CPU   // tests/emul: the record view as plain C++
#include <cstdint>
#else
#include "common.h"
#endif

namespace ngsqc {

__device__ __forceinline__ uint32_t ld32(const uint8_t* p) { uint32_t v; __builtin_memcpy(&v, p, 4); return v; }
__device__ __forceinline__ uint16_t ld16(const uint8_t* p) { uint16_t v; __builtin_memcpy(&v, p, 2); return v; }

struct RecView
{
	const uint8_t* core;   // points at refID (record + 4)
	uint32_t bs; int32_t tid, pos; uint32_t l_name, mapq, n_cigar_raw, flag; int32_t l_seq, isize;
	const uint8_t* cigar; uint32_t n_cigar;  // effective CIGAR (may be the CG tag payload)
};

// the fixed part of a record as the chain walk keeps it one record ahead: block_size, refID, pos, (l_read_name | mapq | bin), (n_cigar_op | flag), l_seq, tlen
struct Hdr { uint32_t bs, tid, pos, w, w2, l_seq, isize; };
__device__ __forceinline__ Hdr load_hdr(const uint8_t* p)
{
	Hdr h; uint32_t a[4], b[2];
	__builtin_memcpy(a, p, 16); __builtin_memcpy(b, p + 16, 8);
	h.bs = a[0]; h.tid = a[1]; h.pos = a[2]; h.w = a[3]; h.w2 = b[0]; h.l_seq = b[1]; h.isize = ld32(p + 32);
	return h;
}
__device__ __forceinline__ RecView make_rec(const uint8_t* infl, int64_t off, const Hdr& h)
{
	RecView r; const uint8_t* p = infl + off;
	r.bs = h.bs; r.core = p + 4; r.tid = (int32_t)h.tid; r.pos = (int32_t)h.pos;
	r.l_name = h.w & 0xff; r.mapq = (h.w >> 8) & 0xff; r.n_cigar_raw = h.w2 & 0xffff; r.flag = h.w2 >> 16;
	r.l_seq = (int32_t)h.l_seq; r.isize = (int32_t)h.isize;
	r.cigar = p + 36 + r.l_name; r.n_cigar = r.n_cigar_raw;
	return r;
}
__device__ __forceinline__ RecView load_rec(const uint8_t* infl, int64_t off)
{
	RecView r; const uint8_t* p = infl + off;
	r.bs = ld32(p); r.core = p + 4;
	r.tid = (int32_t)ld32(p + 4); r.pos = (int32_t)ld32(p + 8);
	uint32_t w = ld32(p + 12), w2 = ld32(p + 16);
	r.l_name = w & 0xff; r.mapq = (w >> 8) & 0xff; r.n_cigar_raw = w2 & 0xffff; r.flag = w2 >> 16;
	r.l_seq = (int32_t)ld32(p + 20); r.isize = (int32_t)ld32(p + 32);
	r.cigar = p + 36 + r.l_name; r.n_cigar = r.n_cigar_raw;
	return r;
}
__device__ __forceinline__ const uint8_t* rec_qual(const RecView& r) { return r.core + 32 + r.l_name + 4ull * r.n_cigar_raw + ((uint32_t)r.l_seq + 1) / 2; }
__device__ __forceinline__ const uint8_t* rec_aux(const RecView& r) { return rec_qual(r) + (uint32_t)r.l_seq; }
__device__ __forceinline__ const uint8_t* rec_end(const RecView& r) { return r.core + r.bs; }

// linear aux scan (what htslib's bam_aux_get does); returns pointer to the type byte or nullptr
__device__ static const uint8_t* aux_find(const uint8_t* p, const uint8_t* end, uint8_t t0, uint8_t t1)
{
	while (p + 3 <= end)
	{
		const uint8_t* t = p + 2;
		if (p[0] == t0 && p[1] == t1) return t;
		uint8_t type = *t; const uint8_t* v = t + 1; size_t sz;
		switch (type)
		{
			case 'A': case 'c': case 'C': sz = 1; break;
			case 's': case 'S': sz = 2; break;
			case 'i': case 'I': case 'f': sz = 4; break;
			case 'd': sz = 8; break;
			case 'Z': case 'H': { const uint8_t* q = v; while (q < end && *q) ++q; sz = (size_t)(q - v) + 1; break; }
			case 'B': { if (v + 5 > end) return nullptr; uint8_t st = v[0]; uint32_t n = ld32(v + 1); size_t es = (st == 'c' || st == 'C') ? 1 : (st == 's' || st == 'S') ? 2 : 4; sz = 5 + es * (size_t)n; break; }
			default: return nullptr;
		}
		p = v + sz;
	}
	return nullptr;
}

// BamAlignment::tagi (src/cppNGS/BamReader.cpp:286-297: bam_aux2i): a missing tag and a tag of a non-integer type count as 0
__device__ static int aux_tagi(const RecView& r, uint8_t t0, uint8_t t1)
{
	const uint8_t* t = aux_find(rec_aux(r), rec_end(r), t0, t1);
	if (!t) return 0;
	switch (*t)
	{
		case 'c': return (int8_t)t[1];
		case 'C': return t[1];
		case 's': return (int16_t)ld16(t + 1);
		case 'S': return ld16(t + 1);
		case 'i': return (int32_t)ld32(t + 1);
		case 'I': return (int)ld32(t + 1);
		default: return 0;
	}
}

#ifndef NGSQC_REC_ON_CPU
__device__ __forceinline__ long long wave_sum(long long v)
{
	for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
	return v;
}
#endif

// CG:B,I long CIGAR (htslib bam_tag2cigar): on a placed record (tid >= 0 and pos >= 0), behind a first operation kS with k == l_seq, the tag's array replaces the
// CIGAR when it holds at least n_cigar operations (the oracle's parse_rec, oracle/bamio.hpp). rec_cg_tag looks the tag up (the caller has checked the first operation): the array, or null; rec_apply_cg does both for one record
__device__ __forceinline__ const uint8_t* rec_cg_tag(const RecView& r, uint32_t& n)
{
	const uint8_t* t = aux_find(rec_aux(r), rec_end(r), 'C', 'G');
	if (t && t[0] == 'B' && t[1] == 'I') { n = ld32(t + 2); if (n >= r.n_cigar_raw && n < (1u << 29)) return t + 6; }
	return nullptr;
}
__device__ __forceinline__ void rec_apply_cg(RecView& r)
{
	if (r.n_cigar_raw == 0 || r.tid < 0 || r.pos < 0) return;
	const uint32_t c0 = ld32(r.cigar);
	if ((c0 & 15u) != 4 || (int32_t)(c0 >> 4) != r.l_seq) return;
	uint32_t n = 0; const uint8_t* cg = rec_cg_tag(r, n);
	if (cg) { r.cigar = cg; r.n_cigar = n; }
}

} // namespace ngsqc
