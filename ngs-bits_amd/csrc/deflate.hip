// BGZF deflate on the device: the writer of every BAM-producing tool (BamFilter first, host/BamFilter.cpp) and ngsqc_bgzf_compress.
//
// The input is cut into pieces of BGZF_PIECE (0xff00) bytes, as htslib's bgzf_write cuts it; each piece becomes one BGZF member (a gzip member with the BC extra
// field) in a 64 KiB slot, and a scan over the member sizes compacts the slots. ONE WORKGROUP PER MEMBER, the piece in LDS:
//   1. CRC32: every thread a 255-byte slice, bytewise with crc.hip's table; the slice states are folded with x^(8 m) (crc_dev.h) and XORed.
//   2. Hash chains: positions are taken in rounds of 256. A position's predecessor is the nearest earlier position of the round with the same 3-byte hash
//      (looked for among the 32 positions before it), else the latest position of an earlier round with that hash (a head table, updated by atomicMax after
//      each round: the maximum does not depend on the order of the atomics). The chain (u16 per position) goes to a per-workgroup scratch in global memory.
//   3. Parse: the piece is cut into NSEG segments; one thread parses each, greedy with zlib's lazy step, walking the chain for matches up to 32 KiB back
//      (anywhere in the piece) but not past the end of its segment. Tokens go to the scratch, symbol counts to LDS histograms (atomic adds).
//   4. Dynamic Huffman codes (lengths limited to 15, the code-length code to 7): symbols ranked in parallel, then one thread builds the lengths (Moffat and
//      Katajainen's in-place method, then miniz's length limit) and the canonical codes.
//   5. Bits: each segment sums the bit length of its tokens, an exclusive scan gives its offset, and every thread ORs its bits into the LDS output (atomicOr:
//      the result does not depend on the order either). One dynamic block per member; a member whose encoding would not beat a stored block is stored.
// Nothing depends on timing or the order of atomics, so the same input gives the same bytes on every run and device.
#include "common.h"
#include "crc_dev.h"
#include "handle.h"
#include <rocprim/device/device_scan.hpp>
#include <mutex>

namespace ngsqc {

namespace {
constexpr int NT = 256;                    // threads of a member's workgroup
constexpr int PIECE = 0xff00;              // 65280 bytes = NT x 255 (BGZF_PIECE)
constexpr int SLICE = PIECE / NT;          // CRC slice of a thread
constexpr int HBITS = 12, HSIZE = 1 << HBITS;
constexpr int LOOKBACK = 32;               // positions of the same round searched for a predecessor
constexpr int NSEG = 128, SEGLEN = PIECE / NSEG;   // parse segments (510 bytes)
constexpr int MAX_CHAIN = 48, NICE = 128, LAZY = 32, WINDOW = 32768;
constexpr int SLOT = 65536;                // a member's slot (the largest BGZF member)
constexpr int HDR = 18, TRL = 8;

__constant__ uint16_t c_len_base[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
__constant__ uint8_t c_len_extra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
__constant__ uint16_t c_dist_base[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
__constant__ uint8_t c_dist_extra[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
__constant__ uint8_t c_cl_order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

__device__ __forceinline__ int len_code(int len)   // 3..258 -> 0..28 (symbol 257 + code)
{
	int c = 0;
	while (c < 28 && c_len_base[c + 1] <= len) ++c;
	return len == 258 ? 28 : c;
}
__device__ __forceinline__ int dist_code(int d)    // 1..32768 -> 0..29
{
	if (d <= 4) return d - 1;
	const int b = 31 - __clz(d - 1);               // d - 1 in [2^b, 2^(b+1))
	return 2 * b + (((d - 1) >> (b - 1)) & 1);
}
__device__ __forceinline__ uint32_t rev_bits(uint32_t c, int n) { return __builtin_bitreverse32(c) >> (32 - n); }

// a token: literal byte b (bit 31 clear), or (1 << 31) | (len - 3) << 16 | (dist - 1)
__device__ __forceinline__ uint32_t tok_match(int len, int dist) { return 0x80000000u | (uint32_t)(len - 3) << 16 | (uint32_t)(dist - 1); }

struct Lds
{
	uint32_t buf[SLOT / 4 + 2];       // the piece (bytes), later the DEFLATE stream (bits, LSB first)
	uint32_t head[HSIZE];             // position + 1 of the latest earlier-round position per hash (0: none)
	uint32_t crc_tab[256];
	uint32_t rh[NT];                  // hashes of the round
	uint32_t freq[288 + 32];          // lit/len symbols, then distance symbols
	uint32_t clfreq[19];
	uint32_t rank[288], A[288];
	uint8_t len[288 + 32];            // code lengths (lit/len, then dist)
	uint16_t code[288 + 32];          // bit-reversed canonical codes
	uint8_t cllen[19]; uint16_t clcode[19];
	uint16_t rle[288 + 32];           // code-length sequence: symbol | extra << 5
	uint8_t seq[288 + 32]; uint32_t cnt[33];   // (thread 0's scratch)
	uint32_t seg_ntok[NSEG], seg_bits[NSEG + 1];
	uint32_t crc, n_rle, hlit, hdist, hclen, hdr_bits, total_bits, stored;
};

__device__ __forceinline__ uint8_t in_byte(const Lds& S, int i) { return reinterpret_cast<const uint8_t*>(S.buf)[i]; }

// code lengths of n symbols with counts f (at least two non-zero) limited to maxbits; rank / A are scratch. Called by the whole workgroup.
__device__ void build_lengths(Lds& S, const uint32_t* f, int n, int maxbits, uint8_t* len, uint32_t* A /* >= n */)
{
	// rank of every used symbol by (count, symbol): the used symbols in ascending order of count
	for (int i = threadIdx.x; i < n; i += NT)
	{
		const uint32_t fi = f[i];
		if (!fi) { len[i] = 0; continue; }
		int r = 0;
		for (int j = 0; j < n; ++j) { const uint32_t fj = f[j]; r += fj && (fj < fi || (fj == fi && j < i)); }
		S.rank[r] = (uint32_t)i;
	}
	__syncthreads();
	if (threadIdx.x == 0)
	{
		int m = 0;
		for (int i = 0; i < n; ++i) m += f[i] != 0;
		for (int i = 0; i < m; ++i) A[i] = f[S.rank[i]];
		// Moffat & Katajainen, "In-place calculation of minimum-redundancy codes" (1995): A[i] becomes the code length of the i-th symbol
		A[0] += A[1]; int root = 0, leaf = 2, next;
		for (next = 1; next < m - 1; ++next)
		{
			if (leaf >= m || A[root] < A[leaf]) { A[next] = A[root]; A[root++] = next; } else A[next] = A[leaf++];
			if (leaf >= m || (root < next && A[root] < A[leaf])) { A[next] += A[root]; A[root++] = next; } else A[next] += A[leaf++];
		}
		A[m - 2] = 0;
		for (next = m - 3; next >= 0; --next) A[next] = A[A[next]] + 1;
		int avbl = 1, used = 0, dpth = 0; root = m - 2; next = m - 1;
		while (avbl > 0)
		{
			while (root >= 0 && (int)A[root] == dpth) { ++used; --root; }
			while (avbl > used) { A[next--] = dpth; --avbl; }
			avbl = 2 * used; ++dpth; used = 0;
		}
		// the length limit (miniz's tdefl_huffman_enforce_max_code_size): counts per length, then the Kraft sum brought back to one
		uint32_t* cnt = S.cnt;
		for (int i = 0; i < 33; ++i) cnt[i] = 0;
		for (int i = 0; i < m; ++i) cnt[min((int)A[i], 32)]++;
		for (int i = maxbits + 1; i <= 32; ++i) { cnt[maxbits] += cnt[i]; cnt[i] = 0; }
		uint32_t total = 0;
		for (int i = maxbits; i > 0; --i) total += cnt[i] << (maxbits - i);
		while (total != (1u << maxbits))
		{
			cnt[maxbits]--;
			for (int i = maxbits - 1; i > 0; --i) if (cnt[i]) { cnt[i]--; cnt[i + 1] += 2; break; }
			total--;
		}
		// the most frequent symbols get the shortest codes
		int k = m - 1;
		for (int l = 1; l <= maxbits; ++l) for (uint32_t j = cnt[l]; j > 0; --j) len[S.rank[k--]] = (uint8_t)l;
	}
	__syncthreads();
}

__device__ void canonical(const uint8_t* len, uint16_t* code, int n)   // one thread
{
	uint32_t bl[16] = {0}, next[16];
	for (int i = 0; i < n; ++i) bl[len[i]]++;
	bl[0] = 0; uint32_t c = 0;
	for (int b = 1; b < 16; ++b) { c = (c + bl[b - 1]) << 1; next[b] = c; }
	for (int i = 0; i < n; ++i) code[i] = len[i] ? (uint16_t)rev_bits(next[len[i]]++, len[i]) : 0;
}

__device__ __forceinline__ void put_bits(Lds& S, uint32_t pos, uint32_t v, int nb)   // nb <= 32; v < 2^nb
{
	if (!nb) return;
	const uint32_t w = pos >> 5, sh = pos & 31;
	atomicOr(&S.buf[w], v << sh);
	if (sh + nb > 32) atomicOr(&S.buf[w + 1], v >> (32 - sh));
}

// the bits of one token (or of EOB for t == ~0u); returns the count, writes them at pos when emit
__device__ __forceinline__ int token_bits(Lds& S, uint32_t t, bool emit, uint32_t pos)
{
	if (!(t >> 31))
	{
		const int l = S.len[t]; if (emit) put_bits(S, pos, S.code[t], l);
		return l;
	}
	const int len = (int)((t >> 16) & 255) + 3, dist = (int)(t & 0xffff) + 1;
	const int lc = len_code(len), dc = dist_code(dist);
	const int l1 = S.len[257 + lc], e1 = c_len_extra[lc], l2 = S.len[288 + dc], e2 = c_dist_extra[dc];
	if (emit)
	{
		put_bits(S, pos, S.code[257 + lc] | (uint32_t)(len - c_len_base[lc]) << l1, l1 + e1);
		put_bits(S, pos + l1 + e1, S.code[288 + dc] | (uint32_t)(dist - c_dist_base[dc]) << l2, l2 + e2);
	}
	return l1 + e1 + l2 + e2;
}

// longest match at p (limit: bytes that may be matched) along the chain, at most CHAIN candidates; returns len (0: none) and dist
template <int CHAIN, int NICE_LEN>
__device__ __forceinline__ int find_match(const Lds& S, const uint16_t* __restrict__ prev, int p, int limit, int& dist)
{
	if (limit < 3) return 0;
	limit = min(limit, 258);
	int best = 2, bd = 0, c = prev[p], depth = 0;
	while (c && depth++ < CHAIN)
	{
		const int q = c - 1;
		if (p - q > WINDOW) break;
		if (in_byte(S, q + best) == in_byte(S, p + best) && in_byte(S, q) == in_byte(S, p))
		{
			int l = 0;
			while (l < limit && in_byte(S, q + l) == in_byte(S, p + l)) ++l;
			if (l > best) { best = l; bd = p - q; if (l >= NICE_LEN || l == limit) break; }
		}
		c = prev[q];
	}
	if (best < 3 || (best == 3 && bd > 4096)) return 0;   // (zlib's TOO_FAR: a 3-byte match that far back costs more than its literals)
	dist = bd; return best;
}

// The parse of a compression level (ngsqc_bgzf_compress_level): CHAIN candidates per position, a match of NICE_LEN bytes ends the search, LAZY_STEP: zlib's lazy
// step; STORE: stored blocks only (level 0). Levels 4-9 and the default are <MAX_CHAIN, NICE, true, false> (the parse of ngsqc_bgzf_compress).
template <int CHAIN, int NICE_LEN, bool LAZY_STEP, bool STORE>
__global__ __launch_bounds__(NT) void bgzf_deflate_kernel(const uint8_t* __restrict__ in, int64_t n_total, int64_t n_members, uint8_t* __restrict__ slots, uint32_t* __restrict__ sizes,
                                                            uint16_t* __restrict__ prev_all, uint32_t* __restrict__ tok_all, const uint32_t* __restrict__ tabs)
{
	__shared__ Lds S;
	const int t = threadIdx.x;
	uint16_t* prev = prev_all + (size_t)blockIdx.x * PIECE;
	uint32_t* tok = tok_all + (size_t)blockIdx.x * PIECE;
	for (int i = t; i < 256; i += NT) S.crc_tab[i] = tabs[TAB_SLICE + i];
	for (int64_t m = blockIdx.x; m < n_members; m += gridDim.x)
	{
		const int64_t base = m * (int64_t)PIECE;
		const int n = (int)min<int64_t>(PIECE, n_total - base);
		const uint8_t* src = in + base;
		uint8_t* dst = slots + m * (int64_t)SLOT;
		// ---- the piece into LDS, tables cleared ----
		uint8_t* b8 = reinterpret_cast<uint8_t*>(S.buf);
		for (int i = 16 * t; i < n; i += 16 * NT)
		{
			if (i + 16 <= n && !((uintptr_t)(src + i) & 15)) *reinterpret_cast<uint4*>(b8 + i) = *reinterpret_cast<const uint4*>(src + i);
			else for (int k = i; k < min(n, i + 16); ++k) b8[k] = src[k];
		}
		for (int i = t; i < HSIZE; i += NT) S.head[i] = 0;
		for (int i = t; i < 288 + 32; i += NT) S.freq[i] = 0;
		if (t < 19) S.clfreq[t] = 0;
		if (t == 0) S.crc = 0;
		__syncthreads();
		// ---- 1. CRC32 ----
		{
			const int lo = t * SLICE, hi = min(n, lo + SLICE);
			uint32_t s = 0;
			for (int i = lo; i < hi; ++i) s = S.crc_tab[(s ^ in_byte(S, i)) & 255u] ^ (s >> 8);
			uint32_t v = lo < hi ? gf_mul(s, gf_x8((uint32_t)(n - hi))) : 0u;
			for (int o = 32; o > 0; o >>= 1) v ^= (uint32_t)__shfl_xor((int)v, o);
			if ((t & 63) == 0) atomicXor(&S.crc, v);
		}
		if constexpr (STORE) { if (t == 0) S.stored = 1u; }
		else {
		// ---- 2. hash chains ----
		for (int r0 = 0; r0 < n; r0 += NT)
		{
			const int p = r0 + t;
			uint32_t h = 0xffffffffu;
			if (p + 2 < n) h = ((uint32_t)in_byte(S, p) << 16 | (uint32_t)in_byte(S, p + 1) << 8 | in_byte(S, p + 2)) * 2654435761u >> (32 - HBITS);
			S.rh[t] = h;
			__syncthreads();
			if (p < n)
			{
				uint32_t c = 0;
				if (h != 0xffffffffu)
				{
					for (int j = t - 1; j >= max(0, t - LOOKBACK); --j) if (S.rh[j] == h) { c = (uint32_t)(r0 + j + 1); break; }
					if (!c) c = S.head[h];
				}
				prev[p] = (uint16_t)c;
			}
			__syncthreads();
			if (h != 0xffffffffu) atomicMax(&S.head[h], (uint32_t)(p + 1));
		}
		__syncthreads();
		// ---- 3. parse ----
		if (t < NSEG)
		{
			const int s0 = t * SEGLEN, s1 = min(n, s0 + SEGLEN);
			uint32_t* o = tok + s0; int k = 0;
			int p = s0, dist = 0, len = p < s1 ? find_match<CHAIN, NICE_LEN>(S, prev, p, s1 - p, dist) : 0;
			while (p < s1)
			{
				if (len >= 3)
				{
					if (LAZY_STEP && len < LAZY && p + 1 < s1)
					{
						int d1 = 0; const int l1 = find_match<CHAIN, NICE_LEN>(S, prev, p + 1, s1 - p - 1, d1);
						if (l1 > len)
						{
							o[k++] = in_byte(S, p); atomicAdd(&S.freq[in_byte(S, p)], 1u);
							++p; len = l1; dist = d1; continue;
						}
					}
					o[k++] = tok_match(len, dist);
					atomicAdd(&S.freq[257 + len_code(len)], 1u); atomicAdd(&S.freq[288 + dist_code(dist)], 1u);
					p += len;
				}
				else { o[k++] = in_byte(S, p); atomicAdd(&S.freq[in_byte(S, p)], 1u); ++p; }
				len = p < s1 ? find_match<CHAIN, NICE_LEN>(S, prev, p, s1 - p, dist) : 0;
			}
			S.seg_ntok[t] = (uint32_t)k;
		}
		__syncthreads();
		// ---- 4. Huffman codes ----
		if (t == 0)
		{
			S.freq[256] = 1;                                   // EOB
			int used = 0; for (int i = 0; i < 30; ++i) used += S.freq[288 + i] != 0;
			for (int i = 0; used < 2; ++i) if (!S.freq[288 + i]) { S.freq[288 + i] = 1; ++used; }   // a complete distance code of at least two symbols (every inflater takes it)
		}
		__syncthreads();
		build_lengths(S, S.freq, 286, 15, S.len, S.A);
		build_lengths(S, S.freq + 288, 30, 15, S.len + 288, S.A);
		if (t == 0)
		{
			for (int i = 286; i < 288; ++i) S.len[i] = 0;
			int hlit = 286; while (hlit > 257 && !S.len[hlit - 1]) --hlit;
			int hdist = 30; while (hdist > 1 && !S.len[288 + hdist - 1]) --hdist;
			// the run-length coded sequence of the hlit + hdist lengths (16: repeat the previous 3-6 times, 17: 3-10 zeros, 18: 11-138 zeros)
			uint8_t* seq = S.seq; int ns = 0;
			for (int i = 0; i < hlit; ++i) seq[ns++] = S.len[i];
			for (int i = 0; i < hdist; ++i) seq[ns++] = S.len[288 + i];
			int nr = 0;
			for (int i = 0; i < ns;)
			{
				const int v = seq[i]; int run = 1;
				while (i + run < ns && seq[i + run] == v) ++run;
				if (v == 0 && run >= 3)
				{
					int r = run;
					while (r >= 11) { const int c = min(r, 138); S.rle[nr++] = (uint16_t)(18 | (c - 11) << 5); S.clfreq[18]++; r -= c; }
					if (r >= 3) { S.rle[nr++] = (uint16_t)(17 | (r - 3) << 5); S.clfreq[17]++; r = 0; }
					while (r-- > 0) { S.rle[nr++] = 0; S.clfreq[0]++; }
				}
				else if (v != 0 && run >= 4)
				{
					S.rle[nr++] = (uint16_t)v; S.clfreq[v]++; int r = run - 1;
					while (r >= 3) { const int c = min(r, 6); S.rle[nr++] = (uint16_t)(16 | (c - 3) << 5); S.clfreq[16]++; r -= c; }
					while (r-- > 0) { S.rle[nr++] = (uint16_t)v; S.clfreq[v]++; }
				}
				else for (int k = 0; k < run; ++k) { S.rle[nr++] = (uint16_t)v; S.clfreq[v]++; }
				i += run;
			}
			int cu = 0; for (int i = 0; i < 19; ++i) cu += S.clfreq[i] != 0;
			for (int i = 0; cu < 2; ++i) if (!S.clfreq[i]) { S.clfreq[i] = 1; ++cu; }
			S.n_rle = (uint32_t)nr; S.hlit = (uint32_t)hlit; S.hdist = (uint32_t)hdist;
		}
		__syncthreads();
		build_lengths(S, S.clfreq, 19, 7, S.cllen, S.A);
		if (t == 0)
		{
			canonical(S.len, S.code, 288); canonical(S.len + 288, S.code + 288, 30); canonical(S.cllen, S.clcode, 19);
			int hclen = 19; while (hclen > 4 && !S.cllen[c_cl_order[hclen - 1]]) --hclen;
			S.hclen = (uint32_t)hclen;
			uint32_t bits = 3 + 5 + 5 + 4 + 3 * hclen;
			for (uint32_t i = 0; i < S.n_rle; ++i) { const int sym = S.rle[i] & 31; bits += S.cllen[sym] + (sym == 16 ? 2 : sym == 17 ? 3 : sym == 18 ? 7 : 0); }
			S.hdr_bits = bits;
		}
		__syncthreads();
		// ---- 5. bits ----
		if (t < NSEG)
		{
			uint32_t b = 0; const uint32_t* o = tok + t * SEGLEN;
			for (uint32_t k = 0; k < S.seg_ntok[t]; ++k) b += (uint32_t)token_bits(S, o[k], false, 0);
			S.seg_bits[t] = b;
		}
		__syncthreads();
		if (t == 0)
		{
			uint32_t acc = S.hdr_bits;
			for (int i = 0; i < NSEG; ++i) { const uint32_t b = S.seg_bits[i]; S.seg_bits[i] = acc; acc += b; }
			acc += S.len[256];
			S.seg_bits[NSEG] = acc; S.total_bits = acc;
			S.stored = (acc + 7) / 8 >= (uint32_t)n + 5 ? 1u : 0u;   // (a stored block: 5 bytes of framing; PIECE + 5 + 26 <= SLOT)
		}
		}   // (!STORE)
		__syncthreads();
		const bool stored = S.stored != 0;
		uint32_t zbytes;
		if (!STORE && !stored)
		{
			for (int i = t; i < SLOT / 4 + 2; i += NT) S.buf[i] = 0;
			__syncthreads();
			if (t == 0)
			{
				uint32_t pos = 0;
				put_bits(S, pos, 1u | 2u << 1, 3); pos += 3;     // BFINAL, BTYPE = 2 (dynamic)
				put_bits(S, pos, S.hlit - 257, 5); pos += 5; put_bits(S, pos, S.hdist - 1, 5); pos += 5; put_bits(S, pos, S.hclen - 4, 4); pos += 4;
				for (uint32_t i = 0; i < S.hclen; ++i) { put_bits(S, pos, S.cllen[c_cl_order[i]], 3); pos += 3; }
				for (uint32_t i = 0; i < S.n_rle; ++i)
				{
					const int sym = S.rle[i] & 31, ex = S.rle[i] >> 5, eb = sym == 16 ? 2 : sym == 17 ? 3 : sym == 18 ? 7 : 0;
					put_bits(S, pos, S.clcode[sym] | (uint32_t)ex << S.cllen[sym], S.cllen[sym] + eb); pos += S.cllen[sym] + eb;
				}
				put_bits(S, S.seg_bits[NSEG] - S.len[256], S.code[256], S.len[256]);
			}
			if (t < NSEG)
			{
				uint32_t pos = S.seg_bits[t]; const uint32_t* o = tok + t * SEGLEN;
				for (uint32_t k = 0; k < S.seg_ntok[t]; ++k) pos += (uint32_t)token_bits(S, o[k], true, pos);
			}
			__syncthreads();
			zbytes = (S.total_bits + 7) / 8;
			const uint8_t* z = reinterpret_cast<const uint8_t*>(S.buf);
			for (uint32_t i = t; i < zbytes; i += NT) dst[HDR + i] = z[i];
		}
		else
		{
			zbytes = (uint32_t)n + 5;
			if (t == 0) { dst[HDR] = 1; dst[HDR + 1] = (uint8_t)n; dst[HDR + 2] = (uint8_t)(n >> 8); dst[HDR + 3] = (uint8_t)~n; dst[HDR + 4] = (uint8_t)(~n >> 8); }
			for (int i = t; i < n; i += NT) dst[HDR + 5 + i] = src[i];
		}
		if (t == 0)
		{
			const uint32_t total = HDR + zbytes + TRL, crc = S.crc ^ tabs[TAB_INIT + n] ^ 0xFFFFFFFFu;
			const uint32_t h[4] = {0x04088b1fu, 0u, 0x0006ff00u, 0x00024342u};   // ID1 ID2 CM FLG, MTIME, XFL OS XLEN, 'B' 'C' SLEN
			for (int i = 0; i < 16; ++i) dst[i] = (uint8_t)(h[i >> 2] >> (8 * (i & 3)));
			dst[16] = (uint8_t)(total - 1); dst[17] = (uint8_t)((total - 1) >> 8);
			uint8_t* tr = dst + HDR + zbytes;
			for (int i = 0; i < 4; ++i) { tr[i] = (uint8_t)(crc >> (8 * i)); tr[4 + i] = (uint8_t)((uint32_t)n >> (8 * i)); }
			sizes[m] = total;
		}
		__syncthreads();
	}
}

// slots -> one contiguous stream at the exclusive prefix sums of the sizes
__global__ __launch_bounds__(256) void bgzf_compact_kernel(const uint8_t* __restrict__ slots, const uint32_t* __restrict__ sizes, const uint64_t* __restrict__ off, int64_t n_members, uint8_t* __restrict__ out)
{
	for (int64_t m = blockIdx.x; m < n_members; m += gridDim.x)
	{
		const uint32_t n = sizes[m]; const uint8_t* s = slots + m * (int64_t)SLOT; uint8_t* d = out + off[m];
		for (uint32_t i = threadIdx.x; i < n; i += 256) d[i] = s[i];
	}
}
} // namespace

// ---- host ----
namespace lib {
size_t bgzf_max_bytes(int64_t n) { return (size_t)((n + PIECE - 1) / PIECE) * SLOT; }

void BgzfDeflater::reserve(int64_t max_members, int device)
{
	int cu = 0; if (hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cu <= 0) cu = 256;
	grid = (int)std::min<int64_t>(std::max<int64_t>(max_members, 1), (int64_t)cu * 2);
	prev.ensure((size_t)grid * PIECE); tok.ensure((size_t)grid * PIECE);
	slots.ensure((size_t)std::max<int64_t>(max_members, 1) * SLOT); sizes.ensure((size_t)std::max<int64_t>(max_members, 1)); off.ensure((size_t)std::max<int64_t>(max_members, 1) + 1);
	size_t tb = 0;
	(void)rocprim::exclusive_scan(nullptr, tb, (uint32_t*)nullptr, (uint64_t*)nullptr, (uint64_t)0, (size_t)std::max<int64_t>(max_members, 1), rocprim::plus<uint64_t>());
	scan_tmp.ensure(tb + 16);
	cap_members = max_members;
}

// compresses n bytes at d_in (n <= cap_members pieces) into d_out (bgzf_max_bytes(n) bytes) at a compression level (0: stored, 1-3: the fast parse, anything else:
// the default parse); returns the compressed size (waits for the stream)
size_t BgzfDeflater::run(const uint8_t* d_in, int64_t n, uint8_t* d_out, hipStream_t s, int device, int level)
{
	if (n <= 0) return 0;
	const int64_t nm = (n + PIECE - 1) / PIECE;
	if (nm > cap_members || !grid) reserve(nm, device);
	const int g = (int)std::min<int64_t>(nm, grid);
	const uint32_t* tabs = crc_device_tables();
	if (level == 0) hipLaunchKernelGGL((bgzf_deflate_kernel<1, 1, false, true>), dim3(g), dim3(NT), 0, s, d_in, n, nm, slots.p, sizes.p, prev.p, tok.p, tabs);
	else if (level == 1) hipLaunchKernelGGL((bgzf_deflate_kernel<4, 32, false, false>), dim3(g), dim3(NT), 0, s, d_in, n, nm, slots.p, sizes.p, prev.p, tok.p, tabs);
	else if (level == 2) hipLaunchKernelGGL((bgzf_deflate_kernel<8, 64, false, false>), dim3(g), dim3(NT), 0, s, d_in, n, nm, slots.p, sizes.p, prev.p, tok.p, tabs);
	else if (level == 3) hipLaunchKernelGGL((bgzf_deflate_kernel<16, 64, false, false>), dim3(g), dim3(NT), 0, s, d_in, n, nm, slots.p, sizes.p, prev.p, tok.p, tabs);
	else hipLaunchKernelGGL((bgzf_deflate_kernel<MAX_CHAIN, NICE, true, false>), dim3(g), dim3(NT), 0, s, d_in, n, nm, slots.p, sizes.p, prev.p, tok.p, tabs);
	KCHECK();
	size_t tb = scan_tmp.n;
	if (rocprim::exclusive_scan(scan_tmp.p, tb, sizes.p, off.p, (uint64_t)0, (size_t)nm + 0, rocprim::plus<uint64_t>(), s) != hipSuccess) throw std::runtime_error("rocprim::exclusive_scan failed");
	hipLaunchKernelGGL(bgzf_compact_kernel, dim3((unsigned)std::min<int64_t>(nm, 4096)), dim3(256), 0, s, slots.p, sizes.p, off.p, nm, d_out); KCHECK();
	uint64_t last_off = 0; uint32_t last_size = 0;
	HIPCHK(hipMemcpyAsync(&last_off, off.p + nm - 1, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
	HIPCHK(hipMemcpyAsync(&last_size, sizes.p + nm - 1, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
	HIPCHK(hipStreamSynchronize(s));
	return (size_t)last_off + last_size;
}
} // namespace lib

} // namespace ngsqc

// BGZF members of 0xff00-byte pieces of the input, no EOF member (include/ngsqc.h)
namespace {
int bgzf_compress_impl(const void* in, size_t n, int device, int level, void* out, size_t cap, size_t* out_n)
{
	if ((n && !in) || !out_n || (cap && !out)) return NGSQC_E_ARG;
	*out_n = 0;
	if (n == 0) return NGSQC_OK;
	try
	{
		HIPCHK(hipSetDevice(device));
		// one stream per device for the process (a stream made and destroyed per call would move the runtime's hardware-queue assignment of every stream made later)
		static std::mutex mu; static hipStream_t streams[64] = {nullptr};
		if (device < 0 || device >= 64) return NGSQC_E_ARG;
		std::lock_guard<std::mutex> g(mu);
		if (!streams[device]) HIPCHK(hipStreamCreateWithFlags(&streams[device], hipStreamNonBlocking));
		hipStream_t s = streams[device];
		constexpr int64_t WIN = (int64_t)16384 * BGZF_PIECE;   // pieces per launch: the device memory stays bounded whatever n is
		BgzfDeflater z; DevBuf<uint8_t> d_in, d_out;
		d_in.alloc((size_t)std::min<int64_t>((int64_t)n, WIN)); d_out.alloc(bgzf_max_bytes(std::min<int64_t>((int64_t)n, WIN)));
		size_t done = 0; bool over = false;
		for (int64_t o = 0; o < (int64_t)n; o += WIN)
		{
			const int64_t k = std::min<int64_t>(WIN, (int64_t)n - o);
			HIPCHK(hipMemcpyAsync(d_in.p, (const uint8_t*)in + o, (size_t)k, hipMemcpyHostToDevice, s));
			const size_t z_n = z.run(d_in.p, k, d_out.p, s, device, level);
			over = over || done + z_n > cap;   // (past cap the windows are still compressed, for the size)
			if (!over)
			{
				HIPCHK(hipMemcpyAsync((uint8_t*)out + done, d_out.p, z_n, hipMemcpyDeviceToHost, s));
				HIPCHK(hipStreamSynchronize(s));
			}
			done += z_n;
		}
		*out_n = done;
		return over ? NGSQC_E_ARG : NGSQC_OK;
	}
	catch (std::exception& e) { fprintf(stderr, "ngsqc_bgzf_compress: %s\n", e.what()); return NGSQC_E_DEVICE; }
}
} // namespace

int ngsqc_bgzf_compress(const void* in, size_t n, int device, void* out, size_t cap, size_t* out_n) { return bgzf_compress_impl(in, n, device, -1, out, cap, out_n); }

int ngsqc_bgzf_compress_level(const void* in, size_t n, int device, int level, void* out, size_t cap, size_t* out_n)
{
	if (level < 0 || level > 9) return NGSQC_E_ARG;
	return bgzf_compress_impl(in, n, device, level, out, cap, out_n);
}
