// BamToFastq on the device (src/BamToFastq/main.cpp:77-214): the records to FASTQ, joined by read name, formatted and deflated into two BGZF streams
// (ngsqc_bam_to_fastq).
//
// One pass over the tiles (stream_tiles). Per tile:
//   1. keys: per record the steps of main() before the mate cache - the region (htslib's iterator rule), 0x900, duplicates -, the name hash, the size of its
//      FASTQ entry (extend and the NUL cut-off of gzputs included) and a "would throw" bit (a reverse-strand record with a base the complement does not know).
//   2. -fix: the tile's candidates are sorted by (name hash, read 1) (stable: file order within a key). In a run of equal keys a record is dropped when an
//      earlier record of the run or an entry of the persistent set has the same name; the others are merged into the set (keys sorted, names in an arena).
//   3. paired-end: unpaired records are counted; the others go through join.h's NameJoin (every closed pair is kept). Per closing record: the out1 and out2
//      entries, their sizes, the first throwing entry in output order (atomicMin), and +1 / -1 for an opening / closing record, whose prefix maximum is the
//      largest cache size (max_cached). Single-end: every record to out1.
//   4. format: an exclusive scan over the entry sizes per stream, then a wave per entry writing it at its offset - whole dwords inside, bytes at the ragged
//      ends - into that stream's window (an entry that straddles two windows is written in two launches). Whole pieces go through the encoder at the level.
#include "join.h"
#include "tofastq_visit.h"
#include <rocprim/device/device_merge.hpp>
#include <rocprim/device/device_reduce.hpp>

namespace ngsqc {

namespace {
struct FqParams { int32_t remove_dup, fix, extend, paired; int32_t reg_tid, reg_start, reg_end; uint64_t mask; };

enum { C_UNPAIRED, C_SINGLE, C_DUP, C_FIXED, N_FQ_COUNTS };
// (the region rule, the entry's info word, fq_entry / fq_byte and a lane's share of an entry: tofastq_visit.h)

// entries: [0, H) held, [H, H + n) the tile's records. key: KEY_NONE here (set by fq_join_keys_kernel); info = entry size | kept | throws.
// fkey: (name hash << 1 | read 1) of a candidate, KEY_NONE for a record that steps 1-2 skip; cand: the record reaches the -fix / mate-cache steps
__global__ __launch_bounds__(256) void fq_keys_kernel(const uint8_t* __restrict__ infl, const int64_t* __restrict__ recoff, int64_t n, int64_t H, FqParams p,
                                                      uint64_t* __restrict__ key, uint32_t* __restrict__ val, uint64_t* __restrict__ src, uint32_t* __restrict__ info,
                                                      uint64_t* __restrict__ fkey, uint32_t* __restrict__ fidx, uint8_t* __restrict__ cand, unsigned long long* __restrict__ counts)
{
	const int64_t stride = (int64_t)gridDim.x * blockDim.x;
	for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < H + n; e += stride)
	{
		val[e] = (uint32_t)e;
		if (e < H) continue;
		const int64_t i = e - H;
		const uint8_t* q = infl + recoff[i];
		const RecView r = load_rec(infl, recoff[i]);
		src[e] = (uint64_t)(uintptr_t)q; key[e] = KEY_NONE; info[e] = 0; fkey[i] = KEY_NONE; fidx[i] = (uint32_t)i; cand[i] = 0;
		if (p.reg_tid >= 0 && !fq_in_region(r, p.reg_tid, p.reg_start, p.reg_end)) continue;
		if (r.flag & 0x900) continue;
		if (p.remove_dup && (r.flag & 0x400)) { atomicAdd(&counts[C_DUP], 1ull); continue; }
		int nl;
		const uint64_t hash = name_hash_z(r.core + 32, r.l_name, nl);
		info[e] = fq_entry_info(r, p.extend, nl);
		fkey[i] = (hash & p.mask) << 1 | ((r.flag & 0x40) ? 1u : 0u);
		cand[i] = 1;
	}
}

// -fix: the persistent set (keys sorted, values = arena offsets of [name length][name bytes]; the name as join_visit.h's name_len gives it, at most 255 bytes)
__device__ __forceinline__ bool arena_same_name(const uint8_t* a, const uint8_t* rec)
{
	const uint32_t la = a[0];
	if (la != (uint32_t)rec_name_len(rec)) return false;
	for (uint32_t i = 0; i < la; ++i) if (a[1 + i] != rec[36 + i]) return false;
	return true;
}
// one thread per run of equal keys among the sorted candidates: a record is a winner unless the set or an earlier winner of the run has its name.
// wn[q] = winner ? 1 << 40 | name bytes : 0 (one scan gives both the winner's slot and its arena offset)
__global__ __launch_bounds__(256) void fq_fix_kernel(const uint64_t* __restrict__ ks, const uint32_t* __restrict__ is, int64_t n, int64_t H, const uint64_t* __restrict__ src,
                                                     const uint64_t* __restrict__ set_k, const uint64_t* __restrict__ set_v, int64_t S, const uint8_t* __restrict__ arena,
                                                     uint8_t* __restrict__ cand, uint64_t* __restrict__ wn, unsigned long long* __restrict__ counts)
{
	const int64_t stride = (int64_t)gridDim.x * blockDim.x;
	for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += stride)
	{
		const uint64_t k = ks[j];
		if (k == KEY_NONE) { wn[j] = 0; continue; }
		if (j > 0 && ks[j - 1] == k) continue;
		int64_t e = j + 1;
		while (e < n && ks[e] == k) ++e;
		int64_t lo = 0, hi = S;   // lower bound of k in the set
		while (lo < hi) { const int64_t m = (lo + hi) >> 1; if (set_k[m] < k) lo = m + 1; else hi = m; }
		for (int64_t q = j; q < e; ++q)
		{
			const uint8_t* a = (const uint8_t*)(uintptr_t)src[H + is[q]];
			bool seen = false;
			for (int64_t m = lo; m < S && set_k[m] == k && !seen; ++m) seen = arena_same_name(arena + set_v[m], a);
			for (int64_t r = j; r < q && !seen; ++r) seen = wn[r] && same_name((const uint8_t*)(uintptr_t)src[H + is[r]], a);
			if (seen) { wn[q] = 0; cand[is[q]] = 0; atomicAdd(&counts[C_FIXED], 1ull); }
			else wn[q] = 1ull << 40 | (1ull + (uint64_t)rec_name_len(a));
		}
	}
}

__global__ __launch_bounds__(256) void fq_fix_store_kernel(const uint64_t* __restrict__ ks, const uint32_t* __restrict__ is, const uint64_t* __restrict__ wn, const uint64_t* __restrict__ wo,
                                                           int64_t n, int64_t H, const uint64_t* __restrict__ src, uint64_t arena_used, uint8_t* __restrict__ arena,
                                                           uint64_t* __restrict__ wk, uint64_t* __restrict__ wv)
{
	const int64_t stride = (int64_t)gridDim.x * blockDim.x;
	for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += stride)
	{
		if (!wn[q]) continue;
		const uint64_t slot = wo[q] >> 40, off = arena_used + (wo[q] & ((1ull << 40) - 1));
		const uint8_t* a = (const uint8_t*)(uintptr_t)src[H + is[q]];
		const uint32_t la = (uint32_t)rec_name_len(a);
		arena[off] = (uint8_t)la;
		for (uint32_t i = 0; i < la; ++i) arena[off + 1 + i] = a[36 + i];
		wk[slot] = ks[q]; wv[slot] = off;
	}
}

// after -fix: the mate-cache keys (paired-end) or the single-end entries
__global__ __launch_bounds__(256) void fq_join_keys_kernel(const uint8_t* __restrict__ cand, const uint64_t* __restrict__ fkey, int64_t n, int64_t H, int paired,
                                                           const uint64_t* __restrict__ src, const uint32_t* __restrict__ info, uint64_t* __restrict__ key,
                                                           uint64_t* __restrict__ rp1, uint64_t* __restrict__ sz1, unsigned long long* __restrict__ err, unsigned long long* __restrict__ counts)
{
	const int64_t stride = (int64_t)gridDim.x * blockDim.x;
	for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
	{
		if (!paired) { rp1[i] = 0; sz1[i] = 0; }
		if (!cand[i]) continue;
		if (paired)
		{
			const uint16_t flag = ld16((const uint8_t*)(uintptr_t)src[H + i] + 18);
			if (!(flag & 1)) { atomicAdd(&counts[C_UNPAIRED], 1ull); continue; }
			key[H + i] = fkey[i] >> 1;
		}
		else
		{
			atomicAdd(&counts[C_SINGLE], 1ull);
			rp1[i] = src[H + i]; sz1[i] = info[H + i] & INFO_SIZE;
			if (info[H + i] & INFO_THROWS) atomicMin(err, (unsigned long long)i);
		}
	}
}

// per tile record after the join: the pair it closes (out1: the read-1 record, out2: the other), the +1 / -1 of the cache and the first throwing entry
// (ordinal 2 i for the out1 entry, 2 i + 1 for the out2 entry)
__global__ __launch_bounds__(256) void fq_pair_sizes_kernel(const int64_t* __restrict__ close_of, const uint64_t* __restrict__ key, int64_t n, int64_t H, const uint64_t* __restrict__ src,
                                                            const uint32_t* __restrict__ info, uint64_t* __restrict__ rp1, uint64_t* __restrict__ sz1, uint64_t* __restrict__ rp2,
                                                            uint64_t* __restrict__ sz2, int64_t* __restrict__ dc, unsigned long long* __restrict__ err)
{
	const int64_t stride = (int64_t)gridDim.x * blockDim.x;
	for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
	{
		const int64_t c = close_of[i];
		dc[i] = key[H + i] == KEY_NONE ? 0 : c >= 0 ? -1 : 1;
		if (c < 0) { rp1[i] = rp2[i] = 0; sz1[i] = sz2[i] = 0; continue; }
		const uint32_t oe = (uint32_t)(c >> 1), ce = (uint32_t)(H + i);
		const bool closer_r1 = (ld16((const uint8_t*)(uintptr_t)src[ce] + 18) & 0x40) != 0;
		const uint32_t e1 = closer_r1 ? ce : oe, e2 = closer_r1 ? oe : ce;
		rp1[i] = src[e1]; sz1[i] = info[e1] & INFO_SIZE; rp2[i] = src[e2]; sz2[i] = info[e2] & INFO_SIZE;
		if (info[e1] & INFO_THROWS) atomicMin(err, (unsigned long long)(2 * i));
		else if (info[e2] & INFO_THROWS) atomicMin(err, (unsigned long long)(2 * i + 1));
	}
}

// the first base of the reversed sequence without a complement, of the entry that throws first
__global__ void fq_bad_base_kernel(const uint64_t* __restrict__ rp, unsigned long long idx, unsigned long long* __restrict__ out)
{
	const uint8_t* rec = (const uint8_t*)(uintptr_t)rp[idx];
	const RecView r = load_rec(rec, 0);
	const uint8_t* sq = r.cigar + 4ull * r.n_cigar_raw;
	for (int j = r.l_seq - 1; j >= 0; --j) { const int c = base_code(sq, j); if (!has_complement(c)) { *out = (unsigned long long)(uint8_t)c_nt16[c]; return; } }
	*out = 'N';
}

// one wave per entry: the bytes of the entry that fall inside the window, whole dwords where they can, single bytes at the ends
__global__ __launch_bounds__(256) void fq_format_kernel(const uint64_t* __restrict__ rp, const uint64_t* __restrict__ sz, const uint64_t* __restrict__ off, int64_t n, int extend,
                                                        int64_t ws, Win w)
{
	const int lane = threadIdx.x & 63;
	const int64_t nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
	for (int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; i < n; i += nw)
	{
		const int64_t size = (int64_t)sz[i];
		if (!size) continue;
		const int64_t pos = (int64_t)off[i] - ws;
		const FqSplit sp = fq_split(pos, size, w.lo, w.hi);
		if (sp.a >= sp.b) continue;
		fq_format_lane(fq_entry((const uint8_t*)(uintptr_t)rp[i], (uint32_t)size, extend), pos, sp, lane, w.base);
	}
}

// a buffer that keeps its first `used` elements when it grows
template <typename T> void grow_keep(DevBuf<T>& b, size_t used, size_t n, const char* what, hipStream_t s)
{
	if (b.n >= n) return;
	DevBuf<T> nb; grow(nb, n, what, "BamToFastq");
	if (used) HIPCHK(hipMemcpyAsync(nb.p, b.p, used * sizeof(T), hipMemcpyDeviceToDevice, s));
	HIPCHK(hipStreamSynchronize(s));
	std::swap(b.p, nb.p); std::swap(b.n, nb.n);
}

template <typename F> size_t temp_bytes(F f) { size_t b = 0; (void)f(b); return b; }
} // namespace

namespace lib {
void bam_to_fastq(ngsqc_handle* h, const ngsqc_fastq_params* fp, const char* out1, const char* out2, ngsqc_fastq_counts* cnt)
{
	if (!fp || !out1 || !cnt) throw ArgError("null argument");
	// (a handle on regions is laid out like a range: what it holds beyond the region is filtered by the keys kernel)
	if (h->selection ? fp->reg_tid < 0 : (h->n_shards != 1 || h->shard_own_members >= 0))
		throw ArgError("BamToFastq needs a handle on the whole file or on a region (not a shard or a range without a region)");
	if (fp->compression_level < 0 || fp->compression_level > 9) throw ArgError("compression level " + std::to_string(fp->compression_level) + " is not in 0..9");
	if (fp->reg_tid >= (int32_t)h->ref_names.size()) throw ArgError("region reference id out of range");
	const bool paired = out2 && *out2;
	FqParams p{fp->remove_duplicates ? 1 : 0, fp->fix ? 1 : 0, std::max(0, fp->extend), paired ? 1 : 0, fp->reg_tid, fp->reg_start, fp->reg_end, name_hash_mask(h->sw.name_hash_bits) >> 1};   // (a 62-bit hash: (hash << 1 | read 1) never equals KEY_NONE)
	const bool timing = h->sw.timing;
	hipStream_t s = h->stream;
	const char* T = "BamToFastq";
	const int64_t W = write_window_bytes(h->sw.write_window_pieces);
	BgzfStream o1(T, W, fp->compression_level), o2(T, W, fp->compression_level);
	o1.sink.open(out1, std::string("Could not open file '") + out1 + "' for writing!");
	if (paired) o2.sink.open(out2, std::string("Could not open file '") + out2 + "' for writing!");
	NameJoin j(T, s);
	DevBuf<unsigned long long> counts; counts.alloc(N_FQ_COUNTS + 2); HIPCHK(hipMemsetAsync(counts.p, 0, (N_FQ_COUNTS + 2) * sizeof(unsigned long long), s));
	DevBuf<uint64_t> fkey, sfkey, rp1, rp2, sz1, sz2, off1, off2, wn, wo, set_k[2], set_v[2]; DevBuf<uint32_t> fidx, sfidx; DevBuf<uint8_t> cand, arena, tmp; DevBuf<int64_t> dc, dsum, dmax;
	DevBuf<unsigned long long> err; err.alloc(1);
	int set_cur = 0; int64_t S = 0; uint64_t arena_used = 0;
	int64_t max_cached = 0;
	double ms_join = 0, t_w = wall_ms();
	EagerRecoff eager(h);
	stream_tiles(h, [&](const TileCtx& c) {
		const double t0 = wall_ms();
		const int64_t n = c.n_rec, H = j.H, N = H + n;
		if (n == 0) return true;
		const int64_t* rec = ensure_recoff(h);
		j.begin_tile(paired ? n : 0, s);
		if (!paired) { grow(j.key, (size_t)N + 1, "the records", T); grow(j.val, (size_t)N + 1, "the records", T); grow(j.src, (size_t)N + 1, "the records", T); grow(j.info, (size_t)N + 1, "the records", T); }
		const char* w = "the FASTQ entries";
		grow(fkey, (size_t)n + 1, w, T); grow(sfkey, (size_t)n + 1, w, T); grow(fidx, (size_t)n + 1, w, T); grow(sfidx, (size_t)n + 1, w, T); grow(cand, (size_t)n + 1, w, T);
		grow(rp1, (size_t)n + 1, w, T); grow(rp2, (size_t)n + 1, w, T); grow(sz1, (size_t)n + 1, w, T); grow(sz2, (size_t)n + 1, w, T); grow(off1, (size_t)n + 1, w, T); grow(off2, (size_t)n + 1, w, T);
		grow(wn, (size_t)n + 1, w, T); grow(wo, (size_t)n + 1, w, T); grow(dc, (size_t)n + 1, w, T); grow(dsum, (size_t)n + 1, w, T); grow(dmax, 2, w, T);
		// (every temporary size first: a buffer must not be replaced while a queued kernel still uses it)
		size_t tb = 0;
		tb = std::max(tb, temp_bytes([&](size_t& b) { return rocprim::radix_sort_pairs(nullptr, b, fkey.p, sfkey.p, fidx.p, sfidx.p, (size_t)n, 0, 64, s); }));
		tb = std::max(tb, scan_tmp_bytes((size_t)n, s));
		tb = std::max(tb, temp_bytes([&](size_t& b) { return rocprim::inclusive_scan(nullptr, b, dc.p, dsum.p, (size_t)n, rocprim::plus<int64_t>(), s); }));
		tb = std::max(tb, temp_bytes([&](size_t& b) { return rocprim::reduce(nullptr, b, dsum.p, dmax.p, (int64_t)0, (size_t)n, rocprim::maximum<int64_t>(), s); }));
		grow(tmp, tb + 16, w, T);
		HIPCHK(hipMemsetAsync(err.p, 0xff, sizeof(unsigned long long), s));
		hipLaunchKernelGGL(fq_keys_kernel, dim3(grid_for(N)), dim3(256), 0, s, c.infl, rec, n, H, p, j.key.p, j.val.p, j.src.p, j.info.p, fkey.p, fidx.p, cand.p, counts.p); KCHECK();
		if (p.fix)
		{
			size_t b = tmp.n;
			if (rocprim::radix_sort_pairs(tmp.p, b, fkey.p, sfkey.p, fidx.p, sfidx.p, (size_t)n, 0, 64, s) != hipSuccess) throw std::runtime_error("rocprim::radix_sort_pairs failed");
			hipLaunchKernelGGL(fq_fix_kernel, dim3(grid_for(n)), dim3(256), 0, s, sfkey.p, sfidx.p, n, H, j.src.p, set_k[set_cur].p, set_v[set_cur].p, S, arena.p, cand.p, wn.p, counts.p); KCHECK();
			scan_u64(tmp, wn.p, wo.p, 0, (size_t)n, s);
			uint64_t last[2] = {0, 0};
			HIPCHK(hipMemcpyAsync(&last[0], wo.p + n - 1, 8, hipMemcpyDeviceToHost, s)); HIPCHK(hipMemcpyAsync(&last[1], wn.p + n - 1, 8, hipMemcpyDeviceToHost, s));
			HIPCHK(hipStreamSynchronize(s));
			const uint64_t tot = last[0] + last[1], nwin = tot >> 40, nbytes = tot & ((1ull << 40) - 1);
			if (nwin)
			{
				// the set grows with the file ("needs much memory"): planned against free memory, a clear error when it does not fit
				const char* fw = "the -fix set of read names";
				grow_keep(arena, arena_used, arena_used + nbytes + 64, fw, s);
				DevBuf<uint64_t>& nk = set_k[set_cur ^ 1]; DevBuf<uint64_t>& nv = set_v[set_cur ^ 1];
				grow(nk, (size_t)(S + nwin) + 1, fw, T); grow(nv, (size_t)(S + nwin) + 1, fw, T);
				// the winners, in key order, into buffers that are free until the pair sizes (sz2, off2)
				uint64_t* wk = sz2.p; uint64_t* wv = off2.p;
				hipLaunchKernelGGL(fq_fix_store_kernel, dim3(grid_for(n)), dim3(256), 0, s, sfkey.p, sfidx.p, wn.p, wo.p, n, H, j.src.p, arena_used, arena.p, wk, wv); KCHECK();
				if (S == 0)
				{
					HIPCHK(hipMemcpyAsync(nk.p, wk, (size_t)nwin * 8, hipMemcpyDeviceToDevice, s)); HIPCHK(hipMemcpyAsync(nv.p, wv, (size_t)nwin * 8, hipMemcpyDeviceToDevice, s));
				}
				else
				{
					size_t mb = 0;
					(void)rocprim::merge(nullptr, mb, set_k[set_cur].p, wk, nk.p, set_v[set_cur].p, wv, nv.p, (size_t)S, (size_t)nwin, rocprim::less<uint64_t>(), s);
					DevBuf<uint8_t> mtmp; grow(mtmp, mb + 16, fw, T); mb = mtmp.n;
					if (rocprim::merge(mtmp.p, mb, set_k[set_cur].p, wk, nk.p, set_v[set_cur].p, wv, nv.p, (size_t)S, (size_t)nwin, rocprim::less<uint64_t>(), s) != hipSuccess) throw std::runtime_error("rocprim::merge failed");
				}
				HIPCHK(hipStreamSynchronize(s));
				set_cur ^= 1; S += (int64_t)nwin; arena_used += nbytes;
			}
		}
		hipLaunchKernelGGL(fq_join_keys_kernel, dim3(grid_for(n)), dim3(256), 0, s, cand.p, fkey.p, n, H, paired ? 1 : 0, j.src.p, j.info.p, j.key.p, rp1.p, sz1.p, err.p, counts.p); KCHECK();
		int64_t mx = 0; unsigned long long e_ord = ~0ull;
		if (paired)
		{
			j.sort_resolve(n, s);
			hipLaunchKernelGGL(fq_pair_sizes_kernel, dim3(grid_for(n)), dim3(256), 0, s, j.close_of.p, j.key.p, n, H, j.src.p, j.info.p, rp1.p, sz1.p, rp2.p, sz2.p, dc.p, err.p); KCHECK();
			size_t b = tmp.n;
			if (rocprim::inclusive_scan(tmp.p, b, dc.p, dsum.p, (size_t)n, rocprim::plus<int64_t>(), s) != hipSuccess) throw std::runtime_error("rocprim::inclusive_scan failed");
			b = tmp.n;
			if (rocprim::reduce(tmp.p, b, dsum.p, dmax.p, (int64_t)0, (size_t)n, rocprim::maximum<int64_t>(), s) != hipSuccess) throw std::runtime_error("rocprim::reduce failed");
			HIPCHK(hipMemcpyAsync(&mx, dmax.p, 8, hipMemcpyDeviceToHost, s));
			o2.place(tmp, sz2.p, off2.p, n, s);
		}
		o1.place(tmp, sz1.p, off1.p, n, s);
		HIPCHK(hipMemcpyAsync(&e_ord, err.p, 8, hipMemcpyDeviceToHost, s));
		if (paired) j.keep_open(n, s);   // (waits for the stream)
		HIPCHK(hipStreamSynchronize(s));
		if (e_ord != ~0ull)
		{
			// the first entry in output order that throws: what it leaves the files is not written (the tool stops there)
			const uint64_t* rp = paired ? ((e_ord & 1) ? rp2.p : rp1.p) : rp1.p;
			const unsigned long long idx = paired ? e_ord >> 1 : e_ord;
			hipLaunchKernelGGL(fq_bad_base_kernel, dim3(1), dim3(1), 0, s, rp, idx, err.p); KCHECK();
			unsigned long long ch = 'N';
			HIPCHK(hipMemcpyAsync(&ch, err.p, 8, hipMemcpyDeviceToHost, s)); HIPCHK(hipStreamSynchronize(s));
			throw FormatError(std::string("Could not convert base '") + (char)ch + "' to complement!");
		}
		if (paired) max_cached = std::max<int64_t>(max_cached, H + mx);
		// the tile's entries in windows of each stream
		const double dz0 = o1.ms_deflate + o1.ms_copy + o2.ms_deflate + o2.ms_copy;
		o1.emit(o1.placed_end(n), s, h->device, [&](const Win& win, int64_t ws) {
			hipLaunchKernelGGL(fq_format_kernel, dim3(grid_for(n, 4)), dim3(256), 0, s, rp1.p, sz1.p, off1.p, n, p.extend, ws, win); KCHECK();
		});
		if (paired)
			o2.emit(o2.placed_end(n), s, h->device, [&](const Win& win, int64_t ws) {
				hipLaunchKernelGGL(fq_format_kernel, dim3(grid_for(n, 4)), dim3(256), 0, s, rp2.p, sz2.p, off2.p, n, p.extend, ws, win); KCHECK();
			});
		HIPCHK(hipStreamSynchronize(s));   // (the old pool and the tile's bytes are no longer read)
		if (paired) j.end_tile();
		ms_join += wall_ms() - t0 - (o1.ms_deflate + o1.ms_copy + o2.ms_deflate + o2.ms_copy - dz0);
		return true;
	});
	unsigned long long jc[4] = {0, 0, 0, 0}, fc[N_FQ_COUNTS] = {0, 0, 0, 0};
	j.read_counts(jc, s);
	HIPCHK(hipMemcpyAsync(fc, counts.p, sizeof(fc), hipMemcpyDeviceToHost, s)); HIPCHK(hipStreamSynchronize(s));
	o1.finish(s, h->device);
	if (paired) o2.finish(s, h->device);
	if (!o1.sink.err.empty()) throw IoError(std::string("Could not write to file '") + out1 + "'!");
	if (paired && !o2.sink.err.empty()) throw IoError(std::string("Could not write to file '") + out2 + "'!");
	cnt->paired = paired ? (int64_t)jc[0] : 0; cnt->unpaired = (int64_t)fc[C_UNPAIRED]; cnt->unmatched = paired ? j.H : 0; cnt->single_end = (int64_t)fc[C_SINGLE];
	cnt->duplicates = (int64_t)fc[C_DUP]; cnt->fixed = (int64_t)fc[C_FIXED]; cnt->max_cached = max_cached;
	if (timing)
		fprintf(stderr, "[ngsqc] bam_to_fastq: %.1f ms in all: join and format %.1f ms, deflate %.1f ms, copy to pinned memory %.1f ms, file writes %.1f ms (host threads), "
		                "%lld open names at the end, %lld names in the -fix set (%llu bytes), level %d, windows of %lld bytes\n",
		        wall_ms() - t_w, ms_join, o1.ms_deflate + o2.ms_deflate, o1.ms_copy + o2.ms_copy, o1.sink.write_ms + o2.sink.write_ms, (long long)j.H, (long long)S,
		        (unsigned long long)arena_used, fp->compression_level, (long long)W);
}
} // namespace lib
} // namespace ngsqc

int ngsqc_bam_to_fastq(ngsqc_handle* h, const ngsqc_fastq_params* p, const char* out1, const char* out2, ngsqc_fastq_counts* c)
{
	return guarded(h, [&] { ngsqc::lib::bam_to_fastq(h, p, out1, out2, c); });
}
