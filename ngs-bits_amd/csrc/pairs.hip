// BamFilter on the device (src/BamFilter/main.cpp:35-134): the mate join by read name, the record gather and the BGZF writer (ngsqc_filter_pairs).
//
// One pass over the tiles (stream_tiles), no second inflate; the join and the writer are join.h's (NameJoin, BgzfStream). Per tile:
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
#include "recwrite.h"

namespace ngsqc {

namespace {
struct PairParams { int32_t min_mq, max_mq, max_mm, max_gap, min_dup, max_is; uint64_t mask; };

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
		key[e] = rec_name_hash(r) & p.mask;
		info[e] = out_size(r) | (alignment_pass(r, p) ? 0x80000000u : 0u);
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
} // namespace

namespace lib {
void filter_pairs(ngsqc_handle* h, const ngsqc_pair_filter* fp, const char* out_path, int64_t* passed, int64_t* dropped)
{
	if (!fp || !out_path || !passed || !dropped) throw ArgError("null argument");
	require_whole_file(h, "BamFilter");
	PairParams p{fp->min_mq, fp->max_mq, fp->max_mm, fp->max_gap, fp->min_dup, fp->max_is, name_hash_mask(h->sw.name_hash_bits)};
	const bool timing = h->sw.timing;
	hipStream_t s = h->stream;
	const int64_t W = write_window_bytes(h->sw.write_window_pieces);
	BgzfStream out("BamFilter", W, -1);
	NameJoin j("BamFilter", s);
	DevBuf<uint64_t> sz, off;
	double ms_pair = 0, t_w = wall_ms();
	open_bam(out, out_path, h, s);
	EagerRecoff eager(h);
	stream_tiles(h, [&](const TileCtx& c) {
		const double t0 = wall_ms();
		const int64_t n = c.n_rec, H = j.H, N = H + n;
		const int64_t* rec = n ? ensure_recoff(h) : nullptr;
		j.begin_tile(n, s);
		grow(sz, (size_t)N + 1, "the pair join", "BamFilter"); grow(off, (size_t)N + 1, "the pair join", "BamFilter");
		if (N == 0) return true;
		hipLaunchKernelGGL(pair_keys_kernel, dim3(grid_for(N)), dim3(256), 0, s, c.infl, rec, n, H, p, j.key.p, j.val.p, j.src.p, j.info.p); KCHECK();
		j.sort_resolve(n, s);
		// the output of the tile's pairs, behind the carried partial piece
		if (n)
		{
			hipLaunchKernelGGL(pair_sizes_kernel, dim3(grid_for(n)), dim3(256), 0, s, j.close_of.p, j.info.p, n, H, sz.p); KCHECK();
			out.place(j.tmp, sz.p, off.p, n, s);
		}
		j.keep_open(n, s);   // (waits for the stream: the placed end is on the host)
		// the tile's pairs in windows of the stream
		const double dz0 = out.ms_deflate + out.ms_copy;
		out.emit(out.placed_end(n), s, h->device, [&](const Win& w, int64_t ws) {
			if (n) { hipLaunchKernelGGL(pair_gather_kernel, dim3(grid_for(n, 4)), dim3(256), 0, s, j.close_of.p, sz.p, off.p, n, H, j.src.p, j.info.p, ws, w); KCHECK(); }
		});
		HIPCHK(hipStreamSynchronize(s));   // (the old pool and the tile's bytes are no longer read)
		j.end_tile();
		ms_pair += wall_ms() - t0 - (out.ms_deflate + out.ms_copy - dz0);
		return true;
	});
	unsigned long long cnt[4] = {0, 0, 0, 0};
	j.read_counts(cnt, s);
	out.close(s, h->device, out_path);
	*passed = (int64_t)cnt[0]; *dropped = (int64_t)cnt[1];
	if (timing)
		fprintf(stderr, "[ngsqc] filter_pairs: %.1f ms in all: pair join and gather %.1f ms, deflate %.1f ms, copy to pinned memory %.1f ms, file writes %.1f ms (host thread), %lld open names at the end, windows of %lld bytes\n",
		        wall_ms() - t_w, ms_pair, out.ms_deflate, out.ms_copy, out.sink.write_ms, (long long)j.H, (long long)W);
}
} // namespace lib
} // namespace ngsqc

int ngsqc_filter_pairs(ngsqc_handle* h, const ngsqc_pair_filter* p, const char* out_bam_path, int64_t* pairs_passed, int64_t* pairs_dropped)
{
	return guarded(h, [&] { ngsqc::lib::filter_pairs(h, p, out_bam_path, pairs_passed, pairs_dropped); });
}
