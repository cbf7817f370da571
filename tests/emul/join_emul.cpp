// The mate join's own text (ngs-bits_amd/csrc/join_visit.h: what the GPU library compiles into join_resolve_kernel, held_bytes_kernel and the tools' keys
// kernels) on the CPU: a sequential driver plays NameJoin's tiles, held set and two pools over designed records (tests/join_cases.py), and
// tests/test_cpu_join_designed.py compares the pairs, counts and open names with the Python restatements. Test infrastructure, never linked into the library.
//
// The driver keeps the device's lifetimes: a tile's records lie in a heap buffer of exactly their size that is overwritten and freed behind the tile, a held
// entry's bytes in a pool of exactly the bytes held_entry_bytes announces, freed once the next pool is filled. A read of a tile that is gone, or behind what a
// held entry kept, meets 0xEE bytes here and ends the run of the stand-alone program under AddressSanitizer (join_emul_main.cpp).
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <numeric>
#include <vector>
#define NGSQC_REC_ON_CPU
#include "device_on_cpu.h"
static inline unsigned long long atomicAdd(unsigned long long* p, unsigned long long v) { const unsigned long long o = *p; *p += v; return o; }
#include "join_visit.h"

using namespace ngsqc;

extern "C" {

uint64_t join_name_hash(const uint8_t* p, int32_t n) { return name_hash(p, n); }
uint64_t join_name_hash_mask(int32_t bits) { return name_hash_mask(bits); }
int32_t join_name_len(const uint8_t* field, uint32_t l_name) { return name_len(field, l_name); }
// the hash of the name of the field as the keys kernels take it (one walk), its length in *n
uint64_t join_name_hash_z(const uint8_t* field, uint32_t l_name, int32_t* n) { int k = -1; const uint64_t h = name_hash_z(field, l_name, k); *n = k; return h; }
int32_t join_same_name(const uint8_t* a, const uint8_t* b) { return same_name(a, b) ? 1 : 0; }

// recs: the records laid end to end, record i at recoff[i] (recoff[n]: the end), in tile tile_of[i] (ascending, below n_tiles). part[i]: the record takes part
// in the join (else KEY_NONE); pass[i]: bit 31 of its info word. Out: opener_of[i] = the record that i closes, or -1; kept[i]: both pass; h_after[t] /
// pool_after[t]: the held entries and their bytes behind tile t; open_idx: the records still open at the end, in held order; counts[0 / 1]: pairs kept / not.
// Returns the number of open records, or -1 - t when the held arrays behind tile t are not what the scans announced.
int64_t join_emul(const uint8_t* recs, const int64_t* recoff, const int32_t* tile_of, int64_t n_all, int32_t n_tiles, const uint8_t* part, const uint8_t* pass, uint64_t mask,
                  int64_t* opener_of, uint8_t* kept, int64_t* h_after, int64_t* pool_after, int64_t* open_idx, unsigned long long* counts)
{
	std::vector<uint8_t> pool[2]; int cur_pool = 0;
	std::vector<uint64_t> hk, hs; std::vector<uint32_t> hi; std::vector<int64_t> hord;
	int64_t H = 0, first = 0;
	counts[0] = counts[1] = counts[2] = counts[3] = 0;
	for (int64_t i = 0; i < n_all; ++i) { opener_of[i] = -1; kept[i] = 0; }
	for (int32_t t = 0; t < n_tiles; ++t)
	{
		int64_t last = first;
		while (last < n_all && tile_of[last] == t) ++last;
		const int64_t n = last - first, N = H + n;
		// the tile buffer: exactly the tile's bytes
		std::vector<uint8_t>* tile = new std::vector<uint8_t>(recs + recoff[first], recs + recoff[last]);
		std::vector<uint64_t> key(N + 1), skey(N + 1), src(N + 1), nb(N + 1), boff(N + 1), hpos(N + 1); std::vector<uint32_t> val(N + 1), sval(N + 1), info(N + 1);
		std::vector<int64_t> close_of(n + 1, -1), ord(N + 1); std::vector<uint8_t> held(N + 1, 0), st(N + 1, 0xCC);
		for (int64_t e = 0; e < H; ++e) { key[e] = hk[e]; src[e] = hs[e]; info[e] = hi[e]; ord[e] = hord[e]; }
		for (int64_t e = 0; e < N; ++e)   // the keys kernel
		{
			val[e] = (uint32_t)e;
			if (e < H) continue;
			const int64_t i = first + (e - H), off = recoff[i] - recoff[first];
			const RecView r = load_rec(tile->data(), off);
			src[e] = (uint64_t)(uintptr_t)(tile->data() + off); ord[e] = i;
			if (!part[i]) { key[e] = KEY_NONE; info[e] = 0; continue; }
			key[e] = rec_name_hash(r) & mask;
			info[e] = (r.bs + 4) | (pass[i] ? 0x80000000u : 0u);
		}
		std::vector<uint32_t> order(N); std::iota(order.begin(), order.end(), 0u);
		std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return key[a] < key[b]; });
		for (int64_t j = 0; j < N; ++j) { skey[j] = key[order[j]]; sval[j] = val[order[j]]; }
		const ResolveOut o{close_of.data(), held.data(), st.data(), counts};
		for (int64_t j = 0; j < N; ++j)   // join_resolve_kernel
		{
			const uint64_t k = skey[j];
			if (k == KEY_NONE || (j > 0 && skey[j - 1] == k)) continue;
			join_resolve_run(skey.data(), sval.data(), N, H, src.data(), info.data(), o, j);
		}
		for (int64_t i = 0; i < n; ++i)
			if (close_of[i] >= 0) { opener_of[first + i] = ord[close_of[i] >> 1]; kept[first + i] = (uint8_t)(close_of[i] & 1); }
		// keep_open: held_bytes_kernel, the two scans, held_store_kernel into the other pool
		uint64_t bytes = 0, cnt = 0;
		for (int64_t j = 0; j < N; ++j)
		{
			nb[j] = held[j] ? held_entry_bytes((const uint8_t*)(uintptr_t)src[sval[j]], (info[sval[j]] >> 31) != 0) : 0;
			boff[j] = bytes; hpos[j] = cnt; bytes += nb[j]; cnt += held[j] ? 1 : 0;
		}
		std::vector<uint8_t>& np = pool[cur_pool ^ 1];
		np.assign((size_t)bytes, 0xEE); np.shrink_to_fit();
		std::vector<uint64_t> nk(cnt), ns(cnt); std::vector<uint32_t> ni(cnt); std::vector<int64_t> nord(cnt);
		for (int64_t j = 0; j < N; ++j)
		{
			if (!held[j]) continue;
			const uint8_t* s = (const uint8_t*)(uintptr_t)src[sval[j]];
			uint8_t* d = np.data() + boff[j];
			for (uint64_t i = 0; i < nb[j]; ++i) d[i] = s[i];
			nk[hpos[j]] = skey[j]; ns[hpos[j]] = (uint64_t)(uintptr_t)d; ni[hpos[j]] = info[sval[j]]; nord[hpos[j]] = ord[sval[j]];
		}
		// end_tile: the tile's bytes and the old pool are gone
		std::fill(tile->begin(), tile->end(), (uint8_t)0xEE); delete tile;
		std::fill(pool[cur_pool].begin(), pool[cur_pool].end(), (uint8_t)0xEE); std::vector<uint8_t>().swap(pool[cur_pool]);
		cur_pool ^= 1; H = (int64_t)cnt; hk.swap(nk); hs.swap(ns); hi.swap(ni); hord.swap(nord);
		for (int64_t e = 1; e < H; ++e) if (hk[e - 1] > hk[e] || (hk[e - 1] == hk[e] && hord[e - 1] > hord[e])) return -1 - t;   // (hash, ordinal) order
		h_after[t] = H; pool_after[t] = (int64_t)bytes;
		first = last;
	}
	for (int64_t e = 0; e < H; ++e) open_idx[e] = hord[e];
	return H;
}
}
