// The mate join's decisions for one record and for one run of equal hashes: what a read name is, its hash, the comparison of two names, the pairing of a run
// and the bytes a held entry keeps - the text csrc/join.h compiles into its kernels (and the tools into their keys kernels), kept free of HIP so that
// tests/emul/join_emul.cpp runs the same text on the CPU against the Python restatements (NGSQC_REC_ON_CPU; the CPU build supplies atomicAdd).
//
// A read name is BamAlignment::name() (src/cppNGS/BamReader.h:69-72): bam_get_qname read as a C string - the bytes of the name field in front of its first
// NUL, at most l_read_name of them. Everything that keys by the name (hash, comparison, the -fix set, the "@" line, the KEPT lines) takes its length from
// name_len; the bytes a record carries (held bytes, written records) stay the whole field.
#pragma once
#include "rec.h"

namespace ngsqc {
namespace {
constexpr uint64_t KEY_NONE = ~0ull;

// the bytes of the name field `name` (l_name bytes) in front of its first NUL. Eight bytes a load while eight are left in the field (a lane's byte loads each
// fetch a cache line of their own: the walk is paid in loads), the first zero byte of a word by the carry trick: its lowest flagged byte is exact
__device__ __forceinline__ int name_len(const uint8_t* name, uint32_t l_name)
{
	uint32_t n = 0;
	for (; n + 8 <= l_name; n += 8)
	{
		uint64_t w; __builtin_memcpy(&w, name + n, 8);
		const uint64_t z = (w - 0x0101010101010101ull) & ~w & 0x8080808080808080ull;
		if (z) return (int)(n + ((uint32_t)__builtin_ctzll(z) >> 3));
	}
	while (n < l_name && name[n]) ++n;
	return (int)n;
}
__device__ __forceinline__ int rec_name_len(const uint8_t* rec) { return name_len(rec + 36, rec[12]); }   // rec: the record, block_size included

__device__ __forceinline__ uint64_t name_hash(const uint8_t* p, int n)   // FNV-1a, then a 64-bit finaliser (splitmix64)
{
	uint64_t h = 0xcbf29ce484222325ull;
	for (int i = 0; i < n; ++i) h = (h ^ p[i]) * 0x100000001b3ull;
	h ^= h >> 30; h *= 0xbf58476d1ce4e5b9ull; h ^= h >> 27; h *= 0x94d049bb133111ebull; h ^= h >> 31;
	return h;
}
// name_hash(p, name_len(p, l_name)) in one walk, eight bytes a load: the hash of a record's name and, in n, the name's length
__device__ __forceinline__ uint64_t name_hash_z(const uint8_t* p, uint32_t l_name, int& n)
{
	uint64_t h = 0xcbf29ce484222325ull;
	uint32_t i = 0; bool open = true;
	while (open && i + 8 <= l_name)
	{
		uint64_t w; __builtin_memcpy(&w, p + i, 8);
		for (int k = 0; k < 8 && open; ++k, w >>= 8) { const uint8_t c = (uint8_t)w; if (c) { h = (h ^ c) * 0x100000001b3ull; ++i; } else open = false; }
	}
	for (; open && i < l_name; ++i) { const uint8_t c = p[i]; if (!c) break; h = (h ^ c) * 0x100000001b3ull; }
	n = (int)i;
	h ^= h >> 30; h *= 0xbf58476d1ce4e5b9ull; h ^= h >> 27; h *= 0x94d049bb133111ebull; h ^= h >> 31;
	return h;
}
__device__ __forceinline__ uint64_t rec_name_hash(const RecView& r) { int n; return name_hash_z(r.core + 32, r.l_name, n); }

// test hook NGSQC_NAME_HASH_BITS (CallSwitches::name_hash_bits, 1 .. 63): fewer hash bits, collisions everywhere
inline uint64_t name_hash_mask(int bits) { return bits >= 63 ? (~0ull >> 1) : ((1ull << bits) - 1); }

// two records (block_size included) carry the same name: both names end at the same place, with the same bytes in front
__device__ __forceinline__ bool same_name(const uint8_t* a, const uint8_t* b)
{
	const uint32_t la = a[12], lb = b[12], n = la < lb ? la : lb;
	for (uint32_t i = 0; i < n; ++i)
	{
		const uint8_t c = a[36 + i];
		if (c != b[36 + i]) return false;
		if (!c) return true;
	}
	return la == lb || (la > n ? a[36 + n] : b[36 + n]) == 0;   // the shorter field ran out without a NUL: the longer name must end there
}

struct ResolveOut { int64_t* close_of; uint8_t* held; uint8_t* st; unsigned long long* counts; };   // close_of[tile record] = opener entry << 1 | kept; held / st: per sorted position

__device__ __forceinline__ void close_pair(const ResolveOut& o, const uint32_t* info, int64_t H, uint32_t oe, uint32_t ce)
{
	const bool kept = (info[oe] >> 31) && (info[ce] >> 31);
	o.close_of[ce - H] = (int64_t)oe << 1 | (kept ? 1 : 0);   // (a closer is always a tile record: every held entry lies before the tile)
	atomicAdd(&o.counts[kept ? 0 : 1], 1ull);
}

// the run of equal hashes that starts at sorted position j (the caller has checked that it starts there and that its key is not KEY_NONE)
__device__ __forceinline__ void join_resolve_run(const uint64_t* __restrict__ ks, const uint32_t* __restrict__ vs, int64_t N, int64_t H, const uint64_t* __restrict__ src,
                                                 const uint32_t* __restrict__ info, const ResolveOut& o, int64_t j)
{
	const uint64_t k = ks[j];
	int64_t e = j + 1;
	while (e < N && ks[e] == k) ++e;
	const uint8_t* first = (const uint8_t*)(uintptr_t)src[vs[j]];
	bool same = true;
	for (int64_t q = j + 1; q < e && same; ++q) same = same_name(first, (const uint8_t*)(uintptr_t)src[vs[q]]);
	if (same)
	{
		int64_t q = j;
		for (; q + 1 < e; q += 2) close_pair(o, info, H, vs[q], vs[q + 1]);
		if (q < e) o.held[q] = 1;
	}
	else   // a hash collision: pair name by name, in file order
	{
		for (int64_t q = j; q < e; ++q)
		{
			const uint8_t* a = (const uint8_t*)(uintptr_t)src[vs[q]];
			int64_t f = -1;
			for (int64_t r = j; r < q && f < 0; ++r) if (o.st[r] == 1 && same_name((const uint8_t*)(uintptr_t)src[vs[r]], a)) f = r;
			if (f >= 0) { o.st[f] = 2; o.st[q] = 2; close_pair(o, info, H, vs[f], vs[q]); }
			else o.st[q] = 1;
		}
		for (int64_t q = j; q < e; ++q) o.held[q] = o.st[q] == 1 ? 1 : 0;
	}
}

// the bytes a held entry keeps: the whole record when it passes, else the fixed part and the name field (all a later name comparison reads)
__device__ __forceinline__ uint64_t held_entry_bytes(const uint8_t* s, bool passes) { return passes ? (uint64_t)ld32(s) + 4 : 36ull + s[12]; }
} // namespace
} // namespace ngsqc
