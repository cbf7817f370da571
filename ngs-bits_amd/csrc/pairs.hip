// BamFilter on the device (src/BamFilter/main.cpp:35-134): the mate join by read name, the record gather and the BGZF writer (ngsqc_filter_pairs).
//
// One pass over the tiles (stream_tiles), no second inflate. Per tile:
//   1. keys: per record a 64-bit hash of its read name (NGSQC_NAME_HASH_BITS truncates it: a test hook that makes collisions common), alignment_pass and the
//      size the record takes in the output. Secondary / supplementary records get the sentinel key and take no part.
//   2. sort: the open entries carried over from earlier tiles ("held", in (hash, ordinal) order) followed by the tile's records, radix-sorted by hash (rocPRIM,
//      stable: within a hash the order stays the file order).
//   3. resolve: one thread per run of equal hashes. When every name of the run is the same, the run pairs (0,1), (2,3), ... and an odd last entry stays open;
//      otherwise (a hash collision) the run is paired name by name in file order. A closed pair is kept when both records pass; the counts are atomic adds.
//   4. gather: the output size of every tile record (the pair it closes, opener then closer), an exclusive scan, and one wave per kept pair copying both
//      records into the uncompressed output stream - behind the partial BGZF piece the previous tile left.
//   5. held: the entries still open are compacted; their bytes are copied out of the tile buffer (the whole record if it passes, the name alone if not).
//   6. deflate: the whole 0xff00-byte pieces of the stream go through the encoder (deflate.hip); the compressed members are copied to pinned memory and
//      written by a host thread while the next tile is processed. The rest of the stream moves to the front for the next tile.
#include "handle.h"
#include "rec.h"
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

namespace ngsqc {

namespace {
constexpr uint64_t KEY_NONE = ~0ull;

struct PairParams { int32_t min_mq, max_mq, max_mm, max_gap, min_dup, max_is; uint64_t mask; };

__device__ __forceinline__ uint64_t name_hash(const uint8_t* p, int n)   // FNV-1a, then a 64-bit finaliser (splitmix64)
{
	uint64_t h = 0xcbf29ce484222325ull;
	for (int i = 0; i < n; ++i) h = (h ^ p[i]) * 0x100000001b3ull;
	h ^= h >> 30; h *= 0xbf58476d1ce4e5b9ull; h ^= h >> 27; h *= 0x94d049bb133111ebull; h ^= h >> 31;
	return h;
}

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
__device__ __forceinline__ uint32_t out_size(const RecView& r)
{
	CgInfo g;
	if (!cg_of(r, g)) return r.bs + 4;
	return g.n <= 65535 ? r.bs + 4 - 4 * r.n_cigar_raw - 8 : r.bs + 4 - 4 * r.n_cigar_raw + 8;
}

__device__ bool alignment_pass(RecView r, const PairParams& p)
{
	rec_apply_cg(r);
	int n_gaps = 0, indel = 0;
	for (uint32_t i = 0; i < r.n_cigar; ++i)
	{
		const uint32_t c = ld32(r.cigar + 4ull * i), op = c & 15u;
		if (op == 1 || op == 2) { indel += (int)(c >> 4); ++n_gaps; }
	}
	const int mm = aux_tagi(r, 'N', 'M') - indel, dup = aux_tagi(r, 'D', 'P');
	const int mq = (int)r.mapq;
	return !(r.flag & 4) && (r.flag & 1) && !(r.flag & 8) && mq >= p.min_mq && mq <= p.max_mq && (p.max_gap == -1 || n_gaps <= p.max_gap) &&
	       (p.max_mm == -1 || mm <= p.max_mm) && dup >= p.min_dup && (p.max_is == -1 || r.isize <= p.max_is);
}

// entries: [0, H) held, [H, H + n) the tile's records. info = output size | pass << 31
__global__ __launch_bounds__(256) void pair_keys_kernel(const uint8_t* __restrict__ infl, const int64_t* __restrict__ recoff, int64_t n, int64_t H, PairParams p,
                                                        uint64_t* __restrict__ key, uint32_t* __restrict__ val, uint64_t* __restrict__ src, uint32_t* __restrict__ info)
{
	const int64_t stride = (int64_t)gridDim.x * blockDim.x;
	for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < H + n; e += stride)
	{
		val[e] = (uint32_t)e;
		if (e < H) continue;
		const int64_t i = e - H;
		const uint8_t* q = infl + recoff[i];
		const RecView r = load_rec(infl, recoff[i]);
		src[e] = (uint64_t)(uintptr_t)q;
		if (r.flag & 0x900) { key[e] = KEY_NONE; info[e] = 0; continue; }
		key[e] = name_hash(r.core + 32, r.l_name ? (int)r.l_name - 1 : 0) & p.mask;
		info[e] = out_size(r) | (alignment_pass(r, p) ? 0x80000000u : 0u);
	}
}

__device__ __forceinline__ bool same_name(const uint8_t* a, const uint8_t* b)
{
	const uint32_t la = a[12], lb = b[12];
	if (la != lb) return false;
	for (uint32_t i = 0; i < la; ++i) if (a[36 + i] != b[36 + i]) return false;
	return true;
}

struct ResolveOut { int64_t* close_of; uint8_t* held; uint8_t* st; unsigned long long* counts; };   // close_of[tile record] = opener entry << 1 | kept; held / st: per sorted position

__device__ __forceinline__ void close_pair(const ResolveOut& o, const uint32_t* info, int64_t H, uint32_t oe, uint32_t ce)
{
	const bool kept = (info[oe] >> 31) && (info[ce] >> 31);
	o.close_of[ce - H] = (int64_t)oe << 1 | (kept ? 1 : 0);   // (a closer is always a tile record: every held entry lies before the tile)
	atomicAdd(&o.counts[kept ? 0 : 1], 1ull);
}

__global__ __launch_bounds__(256) void pair_resolve_kernel(const uint64_t* __restrict__ ks, const uint32_t* __restrict__ vs, int64_t N, int64_t H, const uint64_t* __restrict__ src,
                                                           const uint32_t* __restrict__ info, ResolveOut o)
{
	const int64_t stride = (int64_t)gridDim.x * blockDim.x;
	for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < N; j += stride)
	{
		const uint64_t k = ks[j];
		if (k == KEY_NONE || (j > 0 && ks[j - 1] == k)) continue;
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
}

__global__ __launch_bounds__(256) void pair_sizes_kernel(const int64_t* __restrict__ close_of, const uint32_t* __restrict__ info, int64_t n, int64_t H, uint64_t* __restrict__ sz)
{
	const int64_t stride = (int64_t)gridDim.x * blockDim.x;
	for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
	{
		const int64_t c = close_of[i];
		sz[i] = c >= 0 && (c & 1) ? (uint64_t)(info[c >> 1] & 0x7fffffffu) + (info[H + i] & 0x7fffffffu) : 0;
	}
}

// A window of the output stream: the bytes [lo, hi) of obuf are written, a record at position pos (relative to obuf[0]; negative: it began in an earlier window)
// writes only what falls inside - so a record that straddles two windows is written in two launches, the same bytes each time.
struct Win { uint8_t* base; int64_t lo, hi; };
__device__ __forceinline__ void put(const Win& w, int64_t& pos, uint8_t v) { if (pos >= w.lo && pos < w.hi) w.base[pos] = v; ++pos; }

// one record into the output window at pos (wave-wide)
__device__ void write_record(const uint8_t* __restrict__ s, const Win& w, int64_t pos, int lane)
{
	const RecView r = load_rec(s, 0);
	CgInfo g;
	if (!cg_of(r, g))
	{
		const int64_t n = (int64_t)r.bs + 4, a = max<int64_t>(0, w.lo - pos), b = min<int64_t>(n, w.hi - pos);
		for (int64_t i = a + lane; i < b; i += 64) w.base[pos + i] = s[i];
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

// off: absolute stream position of every kept pair; ws: the stream position of obuf[0]
__global__ __launch_bounds__(256) void pair_gather_kernel(const int64_t* __restrict__ close_of, const uint64_t* __restrict__ sz, const uint64_t* __restrict__ off, int64_t n, int64_t H,
                                                          const uint64_t* __restrict__ src, const uint32_t* __restrict__ info, int64_t ws, Win w)
{
	const int lane = threadIdx.x & 63;
	const int64_t nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
	for (int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; i < n; i += nw)
	{
		if (!sz[i]) continue;
		const int64_t pos = (int64_t)off[i] - ws;
		if (pos >= w.hi || pos + (int64_t)sz[i] <= w.lo) continue;
		const uint32_t oe = (uint32_t)(close_of[i] >> 1);
		write_record((const uint8_t*)(uintptr_t)src[oe], w, pos, lane);
		write_record((const uint8_t*)(uintptr_t)src[H + i], w, pos + (info[oe] & 0x7fffffffu), lane);
	}
}

// the bytes a held entry keeps: the whole record when it passes, else the fixed part and the name (all a later name comparison reads)
__global__ __launch_bounds__(256) void held_bytes_kernel(const uint8_t* __restrict__ held, const uint32_t* __restrict__ vs, int64_t N, const uint64_t* __restrict__ src, const uint32_t* __restrict__ info, uint64_t* __restrict__ nb)
{
	const int64_t stride = (int64_t)gridDim.x * blockDim.x;
	for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < N; j += stride)
	{
		if (!held[j]) { nb[j] = 0; continue; }
		const uint8_t* s = (const uint8_t*)(uintptr_t)src[vs[j]];
		nb[j] = (info[vs[j]] >> 31) ? (uint64_t)ld32(s) + 4 : 36ull + s[12];
	}
}

__global__ __launch_bounds__(256) void held_store_kernel(const uint8_t* __restrict__ held, const uint64_t* __restrict__ hpos, const uint64_t* __restrict__ nb, const uint64_t* __restrict__ boff,
                                                         const uint32_t* __restrict__ vs, const uint64_t* __restrict__ ks, int64_t N, const uint64_t* __restrict__ src, const uint32_t* __restrict__ info,
                                                         uint8_t* __restrict__ pool, uint64_t* __restrict__ hk, uint64_t* __restrict__ hs, uint32_t* __restrict__ hi)
{
	const int lane = threadIdx.x & 63;
	const int64_t nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
	for (int64_t j = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; j < N; j += nw)
	{
		if (!held[j]) continue;
		const uint8_t* s = (const uint8_t*)(uintptr_t)src[vs[j]];
		uint8_t* d = pool + boff[j];
		for (uint64_t i = lane; i < nb[j]; i += 64) d[i] = s[i];
		if (lane == 0) { const uint64_t h = hpos[j]; hk[h] = ks[j]; hs[h] = (uint64_t)(uintptr_t)d; hi[h] = info[vs[j]]; }
	}
}

unsigned grid_for(int64_t n, int per = 256) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + per - 1) / per, 65536)); }

// compressed members to the file: two pinned buffers, a host thread writes one while the next is filled
struct FileSink
{
	FILE* f = nullptr; std::thread th; std::mutex mu; std::condition_variable cv;
	PinBuf<uint8_t> pb[2]; size_t len[2] = {0, 0}; bool full[2] = {false, false}; bool stop = false; std::string err; int next = 0;
	double write_ms = 0;
	void open(const char* path)
	{
		f = fopen(path, "wb");
		if (!f) throw IoError(std::string("Could not open BAM/CRAM file for writing: ") + path);
		th = std::thread([this] { run(); });
	}
	void run()
	{
		int cur = 0;
		std::unique_lock<std::mutex> lk(mu);
		for (;;)
		{
			cv.wait(lk, [&] { return full[cur] || stop; });
			if (!full[cur]) return;
			lk.unlock();
			const double t0 = wall_ms();
			const bool ok = fwrite(pb[cur].p, 1, len[cur], f) == len[cur];
			lk.lock();
			write_ms += wall_ms() - t0;
			if (!ok && err.empty()) err = "write error";
			full[cur] = false; cur ^= 1; cv.notify_all();
		}
	}
	uint8_t* slot(size_t n)   // waits until the next buffer is free
	{
		std::unique_lock<std::mutex> lk(mu);
		cv.wait(lk, [&] { return !full[next]; });
		lk.unlock();
		pb[next].ensure(std::max<size_t>(n, 1));
		return pb[next].p;
	}
	void commit(size_t n) { { std::lock_guard<std::mutex> g(mu); len[next] = n; full[next] = true; } cv.notify_all(); next ^= 1; }
	void put_device(const uint8_t* d, size_t n, hipStream_t s)
	{
		if (!n) return;
		uint8_t* p = slot(n);
		HIPCHK(hipMemcpyAsync(p, d, n, hipMemcpyDeviceToHost, s)); HIPCHK(hipStreamSynchronize(s));
		commit(n);
	}
	void put_host(const uint8_t* h, size_t n) { if (!n) return; uint8_t* p = slot(n); memcpy(p, h, n); commit(n); }
	void finish()
	{
		{ std::lock_guard<std::mutex> g(mu); stop = true; } cv.notify_all();
		if (th.joinable()) th.join();
		if (f) { if (fclose(f) != 0 && err.empty()) err = "close error"; f = nullptr; }
	}
	~FileSink() { finish(); }
};

const uint8_t BGZF_EOF[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};

// device buffers of the join and the held set grow with the tile and with the names still open: planned against hipMemGetInfo before they are allocated
template <typename T> void grow(DevBuf<T>& b, size_t n, const char* what)
{
	if (b.n >= n) return;
	const size_t want = (n + n / 4 + 1024) * sizeof(T);
	size_t fr = 0, tot = 0;
	if (hipMemGetInfo(&fr, &tot) == hipSuccess && want > fr + b.n * sizeof(T))
	{
		reaper().drain();   // (memory on its way back to the driver)
		if (hipMemGetInfo(&fr, &tot) == hipSuccess && want > fr + b.n * sizeof(T))
			throw std::runtime_error(std::string("BamFilter: ") + what + " does not fit in device memory (" + std::to_string(want >> 20) + " MiB needed, " + std::to_string(fr >> 20) + " MiB free)");
	}
	try { b.alloc(n + n / 4 + 1024); }
	catch (std::exception& e) { throw std::runtime_error(std::string("BamFilter: ") + what + " does not fit in device memory (" + std::to_string((n * sizeof(T)) >> 20) + " MiB asked for; " + e.what() + ")"); }
}
} // namespace

namespace lib {
void filter_pairs(ngsqc_handle* h, const ngsqc_pair_filter* fp, const char* out_path, int64_t* passed, int64_t* dropped)
{
	if (!fp || !out_path || !passed || !dropped) throw ArgError("null argument");
	if (h->selection || h->n_shards != 1 || h->shard_own_members >= 0) throw ArgError("BamFilter needs a handle on the whole file (not a shard, a range or regions)");
	const char* hb = getenv("NGSQC_NAME_HASH_BITS");   // test hook: fewer hash bits, collisions everywhere
	const int bits = hb ? std::max(1, std::min(63, atoi(hb))) : 63;
	PairParams p{fp->min_mq, fp->max_mq, fp->max_mm, fp->max_gap, fp->min_dup, fp->max_is, bits >= 63 ? (~0ull >> 1) : ((1ull << bits) - 1)};
	const bool timing = getenv("NGSQC_TIMING") != nullptr;
	hipStream_t s = h->stream;
	// the header: the input's bytes (magic, l_text, text, n_ref, refs), in members of its own
	std::vector<uint8_t> hdr;
	auto put32 = [&](uint32_t v) { for (int i = 0; i < 4; ++i) hdr.push_back((uint8_t)(v >> (8 * i))); };
	hdr.insert(hdr.end(), {'B', 'A', 'M', 1}); put32((uint32_t)h->header_text.size()); hdr.insert(hdr.end(), h->header_text.begin(), h->header_text.end());
	put32((uint32_t)h->ref_names.size());
	for (size_t i = 0; i < h->ref_names.size(); ++i) { put32((uint32_t)h->ref_names[i].size() + 1); hdr.insert(hdr.end(), h->ref_names[i].begin(), h->ref_names[i].end()); hdr.push_back(0); put32((uint32_t)h->ref_lens[i]); }
	// the writer works on fixed windows of the output stream (NGSQC_WRITE_WINDOW_PIECES: pieces of 0xff00 bytes per window, a test hook; default about 1 GiB):
	// its device and pinned memory does not depend on the size of the file or of a tile
	const char* wp = getenv("NGSQC_WRITE_WINDOW_PIECES");
	const int64_t W = std::max<int64_t>(1, wp ? atoll(wp) : 16384) * BGZF_PIECE;
	FileSink sink; sink.open(out_path);
	BgzfDeflater z;   // (its slots grow with the largest window deflated, at most W)
	DevBuf<uint8_t> obuf, zbuf, pool[2]; int cur_pool = 0;
	DevBuf<uint64_t> key, skey, src, sz, off, hk, hs, nb, boff, hpos; DevBuf<uint32_t> val, sval, info, hi; DevBuf<int64_t> close_of; DevBuf<uint8_t> held, st, sort_tmp;
	DevBuf<unsigned long long> counts; counts.alloc(2); HIPCHK(hipMemsetAsync(counts.p, 0, 2 * sizeof(unsigned long long), s));
	int64_t H = 0, carry = 0, ws = 0;   // ws: stream position of obuf[0]; obuf[0, carry) holds the partial piece in front of what comes next
	double ms_pair = 0, ms_deflate = 0, ms_copy = 0, t_w = wall_ms();
	auto deflate_out = [&](int64_t bytes) {   // the first `bytes` of obuf (whole pieces, or the tail at the end) to the file
		if (bytes <= 0) return;
		const double t0 = wall_ms();
		grow(zbuf, bgzf_max_bytes(bytes), "the compressed output window");   // (bytes <= W: bounded)
		const size_t zn = z.run(obuf.p, bytes, zbuf.p, s, h->device);
		const double t1 = wall_ms(); ms_deflate += t1 - t0;
		sink.put_device(zbuf.p, zn, s);   // (waits while both pinned buffers are still being written)
		ms_copy += wall_ms() - t1;
	};
	// obuf grows with what a window needs, up to W, keeping the partial piece in front (a small file never allocates a whole window)
	auto ensure_obuf = [&](int64_t need) {
		if ((int64_t)obuf.n >= need) return;
		DevBuf<uint8_t> nbf; grow(nbf, (size_t)std::min<int64_t>(W, need + need / 4) , "the output window");
		if (nbf.n > (size_t)W) { nbf.release(); nbf.alloc((size_t)W); }
		if (carry) HIPCHK(hipMemcpyAsync(nbf.p, obuf.p, (size_t)carry, hipMemcpyDeviceToDevice, s));
		HIPCHK(hipStreamSynchronize(s));
		std::swap(obuf.p, nbf.p); std::swap(obuf.n, nbf.n);
	};
	for (size_t o = 0; o < hdr.size(); o += (size_t)W)   // (the header's pieces are cut from its own start: windows are whole pieces)
	{
		const size_t k = std::min(hdr.size() - o, (size_t)W);
		ensure_obuf((int64_t)k);
		HIPCHK(hipMemcpyAsync(obuf.p, hdr.data() + o, k, hipMemcpyHostToDevice, s));
		deflate_out((int64_t)k);
	}
	const bool lazy_keep = h->lazy_recoff; h->lazy_recoff = false;
	struct Restore { ngsqc_handle* h; bool v; ~Restore() { h->lazy_recoff = v; } } restore{h, lazy_keep};
	stream_tiles(h, [&](const TileCtx& c) {
		const double t0 = wall_ms();
		const int64_t n = c.n_rec, N = H + n;
		const int64_t* rec = n ? ensure_recoff(h) : nullptr;
		grow(key, (size_t)N + 1, "the pair join"); grow(skey, (size_t)N + 1, "the pair join"); grow(val, (size_t)N + 1, "the pair join"); grow(sval, (size_t)N + 1, "the pair join");
		grow(src, (size_t)N + 1, "the pair join"); grow(info, (size_t)N + 1, "the pair join"); grow(held, (size_t)N + 1, "the pair join"); grow(st, (size_t)N + 1, "the pair join");
		grow(close_of, (size_t)n + 1, "the pair join"); grow(sz, (size_t)N + 1, "the pair join"); grow(off, (size_t)N + 1, "the pair join");
		grow(nb, (size_t)N + 1, "the pair join"); grow(boff, (size_t)N + 1, "the pair join"); grow(hpos, (size_t)N + 1, "the pair join");
		if (H)
		{
			HIPCHK(hipMemcpyAsync(key.p, hk.p, (size_t)H * 8, hipMemcpyDeviceToDevice, s)); HIPCHK(hipMemcpyAsync(src.p, hs.p, (size_t)H * 8, hipMemcpyDeviceToDevice, s));
			HIPCHK(hipMemcpyAsync(info.p, hi.p, (size_t)H * 4, hipMemcpyDeviceToDevice, s));
		}
		if (N == 0) return true;
		hipLaunchKernelGGL(pair_keys_kernel, dim3(grid_for(N)), dim3(256), 0, s, c.infl, rec, n, H, p, key.p, val.p, src.p, info.p); KCHECK();
		// (every temporary size first: a buffer must not be replaced while a queued kernel still uses it)
		size_t tb = 0, sb1 = 0, sb2 = 0, sb3 = 0;
		(void)rocprim::radix_sort_pairs(nullptr, tb, key.p, skey.p, val.p, sval.p, (size_t)N, 0, 64, s);
		(void)rocprim::exclusive_scan(nullptr, sb1, sz.p, off.p, (uint64_t)0, (size_t)std::max<int64_t>(n, 1), rocprim::plus<uint64_t>(), s);
		(void)rocprim::exclusive_scan(nullptr, sb2, nb.p, boff.p, (uint64_t)0, (size_t)N, rocprim::plus<uint64_t>(), s);
		(void)rocprim::exclusive_scan(nullptr, sb3, held.p, hpos.p, (uint64_t)0, (size_t)N, rocprim::plus<uint64_t>(), s);
		grow(sort_tmp, std::max(std::max(tb, sb1), std::max(sb2, sb3)) + 16, "the pair join");
		tb = sort_tmp.n;
		if (rocprim::radix_sort_pairs(sort_tmp.p, tb, key.p, skey.p, val.p, sval.p, (size_t)N, 0, 64, s) != hipSuccess) throw std::runtime_error("rocprim::radix_sort_pairs failed");
		if (n) HIPCHK(hipMemsetAsync(close_of.p, 0xff, (size_t)n * sizeof(int64_t), s));
		HIPCHK(hipMemsetAsync(held.p, 0, (size_t)N, s));
		hipLaunchKernelGGL(pair_resolve_kernel, dim3(grid_for(N)), dim3(256), 0, s, skey.p, sval.p, N, H, src.p, info.p, ResolveOut{close_of.p, held.p, st.p, counts.p}); KCHECK();
		// the output of the tile's pairs, behind the carried partial piece
		uint64_t tot[2] = {0, 0};
		if (n)
		{
			hipLaunchKernelGGL(pair_sizes_kernel, dim3(grid_for(n)), dim3(256), 0, s, close_of.p, info.p, n, H, sz.p); KCHECK();
			size_t sb = sort_tmp.n;
			if (rocprim::exclusive_scan(sort_tmp.p, sb, sz.p, off.p, (uint64_t)(ws + carry), (size_t)n, rocprim::plus<uint64_t>(), s) != hipSuccess) throw std::runtime_error("rocprim::exclusive_scan failed");
			HIPCHK(hipMemcpyAsync(&tot[0], off.p + n - 1, 8, hipMemcpyDeviceToHost, s)); HIPCHK(hipMemcpyAsync(&tot[1], sz.p + n - 1, 8, hipMemcpyDeviceToHost, s));
		}
		// the open entries: their bytes leave the tile buffer now (K1 will overwrite it)
		hipLaunchKernelGGL(held_bytes_kernel, dim3(grid_for(N)), dim3(256), 0, s, held.p, sval.p, N, src.p, info.p, nb.p); KCHECK();
		uint64_t hcnt[4] = {0, 0, 0, 0};
		{
			size_t sb = sort_tmp.n;
			if (rocprim::exclusive_scan(sort_tmp.p, sb, nb.p, boff.p, (uint64_t)0, (size_t)N, rocprim::plus<uint64_t>(), s) != hipSuccess) throw std::runtime_error("rocprim::exclusive_scan failed");
			sb = sort_tmp.n;
			if (rocprim::exclusive_scan(sort_tmp.p, sb, held.p, hpos.p, (uint64_t)0, (size_t)N, rocprim::plus<uint64_t>(), s) != hipSuccess) throw std::runtime_error("rocprim::exclusive_scan failed");
			HIPCHK(hipMemcpyAsync(&hcnt[0], boff.p + N - 1, 8, hipMemcpyDeviceToHost, s)); HIPCHK(hipMemcpyAsync(&hcnt[1], nb.p + N - 1, 8, hipMemcpyDeviceToHost, s));
			HIPCHK(hipMemcpyAsync(&hcnt[2], hpos.p + N - 1, 8, hipMemcpyDeviceToHost, s));
			uint8_t last_held = 0; HIPCHK(hipMemcpyAsync(&last_held, held.p + N - 1, 1, hipMemcpyDeviceToHost, s));
			HIPCHK(hipStreamSynchronize(s));
			hcnt[3] = last_held;
		}
		const int64_t out_end = n ? (int64_t)(tot[0] + tot[1]) : ws + carry;   // (stream position)
		const uint64_t pool_bytes = hcnt[0] + hcnt[1], newH = hcnt[2] + hcnt[3];
		DevBuf<uint8_t>& np = pool[cur_pool ^ 1];
		grow(np, (size_t)pool_bytes + 64, "the open read names (held set)");
		// (the held arrays are rewritten: their old contents were copied into the entry arrays above)
		grow(hk, (size_t)newH + 1, "the open read names (held set)"); grow(hs, (size_t)newH + 1, "the open read names (held set)"); grow(hi, (size_t)newH + 1, "the open read names (held set)");
		hipLaunchKernelGGL(held_store_kernel, dim3(grid_for(N, 4)), dim3(256), 0, s, held.p, hpos.p, nb.p, boff.p, sval.p, skey.p, N, src.p, info.p, np.p, hk.p, hs.p, hi.p); KCHECK();
		// the tile's pairs in windows of the stream: gather, whole pieces to the encoder, the partial piece to the front
		const double dz0 = ms_deflate + ms_copy;
		for (;;)
		{
			const int64_t w_end = std::min<int64_t>(out_end, ws + W), have = ws + carry;
			if (n && w_end > have)
			{
				ensure_obuf(w_end - ws);
				hipLaunchKernelGGL(pair_gather_kernel, dim3(grid_for(n, 4)), dim3(256), 0, s, close_of.p, sz.p, off.p, n, H, src.p, info.p, ws, Win{obuf.p, have - ws, w_end - ws}); KCHECK();
			}
			const int64_t fill = w_end - ws, whole = fill / BGZF_PIECE * BGZF_PIECE;
			if (whole)
			{
				deflate_out(whole);
				carry = fill - whole;
				if (carry) HIPCHK(hipMemcpyAsync(obuf.p, obuf.p + whole, (size_t)carry, hipMemcpyDeviceToDevice, s));   // (carry < one piece <= whole: no overlap)
				ws += whole;
			}
			else carry = fill;
			if (w_end >= out_end) break;
		}
		HIPCHK(hipStreamSynchronize(s));   // (the old pool and the tile's bytes are no longer read)
		cur_pool ^= 1; H = (int64_t)newH;
		ms_pair += wall_ms() - t0 - (ms_deflate + ms_copy - dz0);
		return true;
	});
	deflate_out(carry);
	sink.put_host(BGZF_EOF, sizeof(BGZF_EOF));
	unsigned long long cnt[2] = {0, 0};
	HIPCHK(hipMemcpyAsync(cnt, counts.p, sizeof(cnt), hipMemcpyDeviceToHost, s)); HIPCHK(hipStreamSynchronize(s));
	sink.finish();
	if (!sink.err.empty()) throw IoError(std::string("Could not write BAM file ") + out_path + ": " + sink.err);
	*passed = (int64_t)cnt[0]; *dropped = (int64_t)cnt[1];
	if (timing)
		fprintf(stderr, "[ngsqc] filter_pairs: %.1f ms in all: pair join and gather %.1f ms, deflate %.1f ms, copy to pinned memory %.1f ms, file writes %.1f ms (host thread), %lld open names at the end, windows of %lld bytes\n",
		        wall_ms() - t_w, ms_pair, ms_deflate, ms_copy, sink.write_ms, (long long)H, (long long)W);
}
} // namespace lib
} // namespace ngsqc

int ngsqc_filter_pairs(ngsqc_handle* h, const ngsqc_pair_filter* p, const char* out_bam_path, int64_t* pairs_passed, int64_t* pairs_dropped)
{
	return guarded(h, [&] { ngsqc::lib::filter_pairs(h, p, out_bam_path, pairs_passed, pairs_dropped); });
}
