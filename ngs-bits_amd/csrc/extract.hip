// BamExtract on the device (src/BamExtract/main.cpp:27-83): a set of read names in device memory, the lookup of every record's name in it, and the split of the
// file over one or two BGZF writers (ngsqc_extract_reads); the lookup on its own (ngsqc_match_names).
//
// The set (NameSet), built once per call: an open-addressed table of 16-byte slots {hash, name offset << 8 | length}, a power of two of slots and at least
// twice the listed names, linear probing; the names stay where the caller's buffer put them (one upload, no arena copy: the length sits in the slot, so a probe
// that meets another length never reads name bytes). Insertion is one lane per listed name: a compare-and-swap on the slot's second word claims an empty slot,
// a slot that holds the same bytes ends the walk (a duplicate), any other slot moves on. Which of two equal names wins a slot depends on the atomics; which
// names are in the table does not, and nothing is ever removed: a lookup that walks from the name's home slot finds it before the first empty slot.
// A listed name that no record can carry (no bytes, more than 254 bytes, a NUL byte) stays out of the table; the host counts the distinct ones of those.
//
// One pass over the tiles (stream_tiles), no join, nothing held between tiles but each writer's partial piece (BgzfStream). Per tile:
//   1. match: one lane per record. The name is the bytes in front of the first NUL of the l_read_name bytes (BamReader.h:69-72: bam_get_qname as a C string),
//      hashed with join.h's name_hash (NGSQC_NAME_HASH_BITS truncates it) and probed. A match byte, and the record's output size (recwrite.h) in the size array
//      of its stream, 0 in the other; the two counts are one atomic add per wave.
//   2. two exclusive scans (rocPRIM), each from its stream's position behind the carried partial piece.
//   3. gather: one wave per record of the stream (recwrite.h's gather_kernel) into the stream's window, per stream; the whole pieces go through the encoder.
// Every record is a candidate: secondary, supplementary and unmapped records are looked up and written like any other (:64-76).
#include "recwrite.h"
#include <unordered_set>

namespace ngsqc {

namespace {
constexpr uint64_t SLOT_EMPTY = ~0ull;
struct NameTable { const ulonglong2* slots; uint64_t slot_mask; const uint8_t* bytes; uint64_t hash_mask; };

__device__ __forceinline__ bool same_bytes(const uint8_t* a, const uint8_t* b, uint32_t n)
{
	for (uint32_t i = 0; i < n; ++i) if (a[i] != b[i]) return false;
	return true;
}

// ref[i]: offset << 8 | length of the i-th listed name, SLOT_EMPTY for a name that takes no part. slots: all words SLOT_EMPTY. *n_in: names that took a slot
__global__ __launch_bounds__(256) void ex_insert_kernel(const uint64_t* __restrict__ ref, int64_t n, const uint8_t* __restrict__ bytes, uint64_t hash_mask, uint64_t slot_mask,
                                                        unsigned long long* slots /* [slot][2] */, unsigned long long* __restrict__ n_in)
{
	const int64_t stride = (int64_t)gridDim.x * blockDim.x;
	const int64_t rounds = (n + stride - 1) / stride;   // (every lane of a wave makes the same number of rounds: the wave sum below sees whole waves)
	int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	uint32_t won = 0;
	for (int64_t r = 0; r < rounds; ++r, i += stride)
	{
		const uint64_t mine = i < n ? ref[i] : SLOT_EMPTY;
		if (mine == SLOT_EMPTY) continue;
		const uint8_t* p = bytes + (mine >> 8);
		const uint32_t len = (uint32_t)(mine & 0xff);
		const uint64_t h = name_hash(p, (int)len) & hash_mask;
		for (uint64_t s = h & slot_mask;; s = (s + 1) & slot_mask)
		{
			const uint64_t cur = atomicCAS(&slots[2 * s + 1], (unsigned long long)SLOT_EMPTY, (unsigned long long)mine);
			if (cur == SLOT_EMPTY) { slots[2 * s] = h; ++won; break; }   // (the hash word is read by the lookup only, behind this kernel; an inserter compares bytes)
			if ((cur & 0xff) == len && same_bytes(bytes + (cur >> 8), p, len)) break;
		}
	}
	const unsigned long long w = (unsigned long long)wave_sum((long long)won);
	if ((threadIdx.x & 63) == 0 && w) atomicAdd(n_in, w);
}

__device__ __forceinline__ bool table_has(const NameTable& t, const uint8_t* name, uint32_t len)
{
	const uint64_t h = name_hash(name, (int)len) & t.hash_mask;
	for (uint64_t s = h & t.slot_mask;; s = (s + 1) & t.slot_mask)
	{
		const ulonglong2 e = t.slots[s];   // (one 16-byte load per probe)
		if (e.y == SLOT_EMPTY) return false;
		if (e.x == h && (e.y & 0xff) == len && same_bytes(t.bytes + (e.y >> 8), name, len)) return true;
	}
}

// match[i] = 1 when the record's name is in the table; sz1 / sz2 (null: not wanted): the record's output size in the array of its stream, 0 in the other.
// counts[0] / [1]: records of stream 1 / 2 (stream 2 only with sz2). Compiled for 8 waves per SIMD (without the attribute the scalar registers allow 7): 35 VGPRs, no scratch
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8))) void ex_match_kernel(const uint8_t* __restrict__ infl, const int64_t* __restrict__ recoff, int64_t n, NameTable t,
                                                       uint8_t* __restrict__ match, uint64_t* __restrict__ sz1, uint64_t* __restrict__ sz2, unsigned long long* __restrict__ counts)
{
	const int64_t stride = (int64_t)gridDim.x * blockDim.x;
	const int64_t rounds = (n + stride - 1) / stride;
	int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	uint32_t c1 = 0, c2 = 0;
	for (int64_t r = 0; r < rounds; ++r, i += stride)
	{
		if (i >= n) continue;
		const RecView rec = load_rec(infl, recoff[i]);
		const uint8_t* name = rec.core + 32;
		uint32_t len = 0;
		while (len < rec.l_name && name[len]) ++len;
		const bool m = len && table_has(t, name, len);   // (the empty name is never listed)
		match[i] = m ? 1 : 0;
		if (sz1)
		{
			const uint64_t osz = m || sz2 ? out_size(rec) : 0;
			sz1[i] = m ? osz : 0;
			if (sz2) sz2[i] = m ? 0 : osz;
			c1 += m ? 1 : 0; c2 += !m && sz2 ? 1 : 0;
		}
	}
	if (!sz1) return;
	const unsigned long long w1 = (unsigned long long)wave_sum((long long)c1), w2 = (unsigned long long)wave_sum((long long)c2);
	if ((threadIdx.x & 63) == 0) { if (w1) atomicAdd(&counts[0], w1); if (w2) atomicAdd(&counts[1], w2); }
}

// the set of the listed names on the device
struct NameSet
{
	DevBuf<uint8_t> bytes; DevBuf<ulonglong2> slots; uint64_t slot_mask = 0; int64_t distinct = 0; double ms_build = 0;
	NameTable table(uint64_t hash_mask) const { return NameTable{slots.p, slot_mask, bytes.p, hash_mask}; }
	void build(const char* tool, const uint8_t* names, const int32_t* name_len, int64_t n, uint64_t hash_mask, hipStream_t s)
	{
		const double t0 = wall_ms();
		const char* what = "the set of read names";
		// offsets and lengths; the names no record can carry are counted here (QSet::count counts them too) and stay out of the table
		std::vector<uint64_t> ref((size_t)n);
		std::unordered_set<std::string> odd;
		uint64_t o = 0; int64_t usable = 0;
		for (int64_t i = 0; i < n; ++i)
		{
			const int64_t l = name_len[i];
			if (l < 0) throw ArgError("negative read name length");
			if (l >= 1 && l <= 254 && !memchr(names + o, 0, (size_t)l)) { ref[(size_t)i] = o << 8 | (uint64_t)l; ++usable; }
			else { ref[(size_t)i] = SLOT_EMPTY; odd.emplace((const char*)names + o, (size_t)l); }
			o += (uint64_t)l;
		}
		uint64_t cap = 64;
		while (cap < 2 * (uint64_t)usable) cap <<= 1;
		slot_mask = cap - 1;
		// the whole plan against the free memory first: the name bytes and the table stay for the call, the offsets go after the insertion
		const size_t need = (size_t)o + (size_t)cap * 16 + (size_t)n * 8 + (64u << 10);
		size_t fr = 0, tot = 0;
		if (hipMemGetInfo(&fr, &tot) == hipSuccess && need > fr)
		{
			reaper().drain();
			if (hipMemGetInfo(&fr, &tot) == hipSuccess && need > fr)
				throw std::runtime_error(std::string(tool) + ": " + what + " does not fit in device memory (" + std::to_string(need >> 20) + " MiB needed, " + std::to_string(fr >> 20) + " MiB free)");
		}
		DevBuf<uint64_t> dref; DevBuf<unsigned long long> cnt;
		grow(bytes, (size_t)o + 1, what, tool); grow(slots, (size_t)cap, what, tool); grow(dref, (size_t)n + 1, what, tool); cnt.alloc(1);
		if (o) HIPCHK(hipMemcpyAsync(bytes.p, names, (size_t)o, hipMemcpyHostToDevice, s));
		if (n) HIPCHK(hipMemcpyAsync(dref.p, ref.data(), (size_t)n * 8, hipMemcpyHostToDevice, s));
		HIPCHK(hipMemsetAsync(slots.p, 0xff, (size_t)cap * 16, s)); HIPCHK(hipMemsetAsync(cnt.p, 0, 8, s));
		if (usable) { hipLaunchKernelGGL(ex_insert_kernel, dim3(grid_for(n)), dim3(256), 0, s, dref.p, n, bytes.p, hash_mask, slot_mask, (unsigned long long*)slots.p, cnt.p); KCHECK(); }
		unsigned long long in = 0;
		HIPCHK(hipMemcpyAsync(&in, cnt.p, 8, hipMemcpyDeviceToHost, s)); HIPCHK(hipStreamSynchronize(s));
		distinct = (int64_t)in + (int64_t)odd.size();
		ms_build = wall_ms() - t0;
	}
};

void check_names(const void* names, const int32_t* name_len, int64_t n_names)
{
	if (n_names < 0) throw ArgError("negative number of read names");
	if (n_names && (!names || !name_len)) throw ArgError("null argument");
}
} // namespace

namespace lib {
void extract_reads(ngsqc_handle* h, const void* names, const int32_t* name_len, int64_t n_names, const char* out_path, const char* out2_path, ngsqc_extract_counts* cnt)
{
	if (!out_path || !cnt) throw ArgError("null argument");
	check_names(names, name_len, n_names);
	require_whole_file(h, "BamExtract");
	const char* T = "BamExtract";
	const bool two = out2_path && *out2_path;
	const uint64_t mask = name_hash_mask(h->sw.name_hash_bits);
	const bool timing = h->sw.timing;
	hipStream_t s = h->stream;
	const double t_w = wall_ms();
	NameSet set;
	set.build(T, (const uint8_t*)names, name_len, n_names, mask, s);
	const NameTable table = set.table(mask);
	const int64_t W = write_window_bytes(h->sw.write_window_pieces);
	BgzfStream o1(T, W, -1), o2(T, W, -1);
	BgzfStream* outs[2] = {&o1, &o2};
	const int n_out = two ? 2 : 1;
	open_bam(o1, out_path, h, s);
	if (two) open_bam(o2, out2_path, h, s);
	DevBuf<uint8_t> match, tmp; DevBuf<uint64_t> sz[2], off[2];
	DevBuf<unsigned long long> counts; counts.alloc(2); HIPCHK(hipMemsetAsync(counts.p, 0, 2 * sizeof(unsigned long long), s));
	StageClock ck_match(timing, s), ck_scan(timing, s), ck_gather(timing, s);
	double ms_tiles = 0; int64_t n_tiles = 0, n_records = 0;
	EagerRecoff eager(h);
	stream_tiles(h, [&](const TileCtx& c) {
		const double t0 = wall_ms();
		const int64_t n = c.n_rec;
		if (n == 0) return true;
		const int64_t* rec = ensure_recoff(h);
		const char* w = "the record sizes";
		grow(match, (size_t)n + 1, w, T);
		for (int k = 0; k < n_out; ++k) { grow(sz[k], (size_t)n + 1, w, T); grow(off[k], (size_t)n + 1, w, T); }
		grow(tmp, scan_tmp_bytes((size_t)n, s) + 16, w, T);
		ck_match.mark();
		hipLaunchKernelGGL(ex_match_kernel, dim3(grid_for(n)), dim3(256), 0, s, c.infl, rec, n, table, match.p, sz[0].p, two ? sz[1].p : nullptr, counts.p); KCHECK();
		ck_match.mark();
		// the position of every record in its stream, behind that stream's carried partial piece
		ck_scan.mark();
		for (int k = 0; k < n_out; ++k) outs[k]->place(tmp, sz[k].p, off[k].p, n, s);
		ck_scan.mark();
		HIPCHK(hipStreamSynchronize(s));
		double dz = 0;
		for (int k = 0; k < n_out; ++k)
		{
			BgzfStream& o = *outs[k];
			const double dz0 = o.ms_deflate + o.ms_copy;
			o.emit(o.placed_end(n), s, h->device, [&](const Win& win, int64_t ws) {
				ck_gather.mark();
				launch_gather<true>(FromTile{c.infl, rec}, NoMask{}, sz[k].p, off[k].p, n, ws, win, s);
				ck_gather.mark();
			});
			dz += o.ms_deflate + o.ms_copy - dz0;
		}
		HIPCHK(hipStreamSynchronize(s));   // (the tile's bytes are no longer read)
		ms_tiles += wall_ms() - t0 - dz; ++n_tiles; n_records += n;
		return true;
	});
	unsigned long long dc[2] = {0, 0};
	HIPCHK(hipMemcpyAsync(dc, counts.p, sizeof(dc), hipMemcpyDeviceToHost, s)); HIPCHK(hipStreamSynchronize(s));
	o1.close(s, h->device, out_path);
	if (two) o2.close(s, h->device, out2_path);
	cnt->out = (int64_t)dc[0]; cnt->out2 = (int64_t)dc[1]; cnt->names = set.distinct;
	if (timing)
		fprintf(stderr, "[ngsqc] extract_reads: %.1f ms in all: name set %.1f ms (%lld names, %lld distinct, %llu slots), match and scans %.1f ms on the host's clock (by HIP events: match kernel %.1f ms, scans %.1f ms, and "
		                "gather kernel %.1f ms, which the host's clock books with the deflate stage that waits for it; %lld records in %lld tiles; K1 %.1f ms and K2 %.1f ms of the input), deflate %.1f ms, copy to pinned memory %.1f ms, file writes %.1f ms (host thread), "
		                "windows of %lld bytes\n",
		        wall_ms() - t_w, set.ms_build, (long long)n_names, (long long)set.distinct, (unsigned long long)(set.slot_mask + 1), ms_tiles, ck_match.total(), ck_scan.total(), ck_gather.total(),
		        (long long)n_records, (long long)n_tiles, h->tm.inflate_ms, h->tm.index_ms, o1.ms_deflate + o2.ms_deflate, o1.ms_copy + o2.ms_copy, o1.sink.write_ms + o2.sink.write_ms, (long long)W);
}

void match_names(ngsqc_handle* h, const void* names, const int32_t* name_len, int64_t n_names, uint8_t* match_out, int64_t cap)
{
	if (cap < 0 || (cap && !match_out)) throw ArgError("null argument");
	check_names(names, name_len, n_names);
	require_whole_file(h, "BamExtract");
	const char* T = "BamExtract";
	const uint64_t mask = name_hash_mask(h->sw.name_hash_bits);
	hipStream_t s = h->stream;
	NameSet set;
	set.build(T, (const uint8_t*)names, name_len, n_names, mask, s);
	const NameTable table = set.table(mask);
	DevBuf<uint8_t> match;
	for_each_tile_bytes(h, match_out, cap, "the match buffer is smaller than the number of records", [&](const TileCtx& c, const int64_t* rec, int64_t n) {
		grow(match, (size_t)n + 1, "the match bytes", T);
		hipLaunchKernelGGL(ex_match_kernel, dim3(grid_for(n)), dim3(256), 0, s, c.infl, rec, n, table, match.p, (uint64_t*)nullptr, (uint64_t*)nullptr, (unsigned long long*)nullptr); KCHECK();
		return match.p;
	});
}
} // namespace lib
} // namespace ngsqc

int ngsqc_extract_reads(ngsqc_handle* h, const void* names, const int32_t* name_len, int64_t n_names, const char* out_bam_path, const char* out2_bam_path, ngsqc_extract_counts* c)
{
	if (!h || !out_bam_path || !c || n_names < 0 || (n_names && (!names || !name_len))) return NGSQC_E_ARG;   // (before a device is touched)
	return guarded(h, [&] { ngsqc::lib::extract_reads(h, names, name_len, n_names, out_bam_path, out2_bam_path, c); });
}

int ngsqc_match_names(ngsqc_handle* h, const void* names, const int32_t* name_len, int64_t n_names, uint8_t* match_out, int64_t cap)
{
	if (!h || n_names < 0 || (n_names && (!names || !name_len)) || cap < 0 || (cap && !match_out)) return NGSQC_E_ARG;
	return guarded(h, [&] { ngsqc::lib::match_names(h, names, name_len, n_names, match_out, cap); });
}
