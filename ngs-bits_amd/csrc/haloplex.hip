// BamCleanHaloplex on the device (src/BamCleanHaloplex/main.cpp:27-69): a verdict per record from the sum of its CIGAR's M lengths, and the copy of every record
// into one BGZF writer with the flag word of the failed ones patched (ngsqc_clean_haloplex); the verdicts on their own (ngsqc_haloplex_verdicts).
//
// One pass over the tiles (stream_tiles), no join, nothing held between tiles but the writer's partial piece (BgzfStream). Per tile:
//   1. verdict: one lane per record. The candidate test on the flag word, rec_apply_cg (a record whose CIGAR sits in its CG tag is judged on the tag's
//      operations, as htslib hands them out), and for a CIGAR of at most HX_LANE_OPS operations the sum in the lane (haloplex_visit.h). A candidate with a longer
//      CIGAR goes on the tile's list: one atomic add per wave reserves the wave's slots, the lanes fill them by their rank in the ballot. The record's output size
//      (recwrite.h) and the three counts, one atomic add per wave and count.
//   2. long CIGARs: one wave per listed record, the lanes stride the operations, wave_sum adds up; lane 0 stores the verdict and counts a failed record. The
//      number of listed records comes to the host with the scan's totals (one wait for both); with an empty list the kernel is not launched.
//   3. an exclusive scan of the sizes (rocPRIM) from the stream position behind the carried partial piece.
//   4. gather: one wave per record (recwrite.h's gather_kernel and write_record), with 0x104 as its flag mask for a failed record. The gather runs once per output window,
//      so it counts nothing. Nothing else of a record changes: bin, the mate fields and the tags are the input's.
// The reference counts reads in `int`; the counts here are 64-bit, and so is the sum of a CIGAR (2^29 operations of up to 2^28 - 1 fit).
//
// Compiled for gfx950 (-Rpass-analysis=kernel-resource-usage): hx_verdict_kernel 32 VGPRs, 92 SGPRs, 8 waves per SIMD; hx_long_kernel 30 VGPRs,
// 85 SGPRs, 8 waves per SIMD. No scratch and no LDS in either; the gather's numbers are in recwrite.h.
#include "recwrite.h"
#include "haloplex_visit.h"

namespace ngsqc {

namespace {
enum { C_READS, C_CANDIDATES, C_FAILED, C_N };

// vd[i]: the verdict byte (a listed record: HX_KEPT until the long kernel has judged it). sz (null: not wanted): the record's output size. counts (null: not wanted)
__global__ __launch_bounds__(256) void hx_verdict_kernel(const uint8_t* __restrict__ infl, const int64_t* __restrict__ recoff, int64_t n, int32_t min_match, uint8_t* __restrict__ vd,
                                                         uint64_t* __restrict__ sz, int64_t* __restrict__ long_list, unsigned long long* __restrict__ long_count,
                                                         unsigned long long* __restrict__ counts)
{
	const int lane = threadIdx.x & 63;
	const int64_t stride = (int64_t)gridDim.x * blockDim.x;
	const int64_t rounds = (n + stride - 1) / stride;   // (every lane of a wave makes the same number of rounds: the ballot and the wave sums below see whole waves)
	int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	uint32_t c_reads = 0, c_cand = 0, c_failed = 0;
	for (int64_t r = 0; r < rounds; ++r, i += stride)
	{
		bool listed = false;
		if (i < n)
		{
			const RecView rec = load_rec(infl, recoff[i]);
			const bool cand = hx_candidate(rec.flag);
			RecView e = rec; rec_apply_cg(e);
			if (sz) sz[i] = out_size(rec, e);
			uint8_t v = HX_NOT_CANDIDATE;
			if (cand)
			{
				listed = e.n_cigar > HX_LANE_OPS;
				v = listed ? HX_KEPT : hx_verdict(true, hx_match_sum(e.cigar, e.n_cigar, 0, 1), min_match);
			}
			vd[i] = v;
			++c_reads; c_cand += cand ? 1 : 0; c_failed += v == HX_FAILED ? 1 : 0;
		}
		const unsigned long long lb = __ballot(listed);
		if (lb)
		{
			unsigned long long base = 0;
			if (lane == 0) base = atomicAdd(long_count, (unsigned long long)__popcll(lb));
			base = (unsigned long long)__shfl((long long)base, 0);
			if (listed) long_list[base + (unsigned long long)__popcll(lb & ((1ull << lane) - 1ull))] = i;   // (at most n entries: every record is listed once)
		}
	}
	if (!counts) return;
	const unsigned long long w0 = (unsigned long long)wave_sum((long long)c_reads), w1 = (unsigned long long)wave_sum((long long)c_cand), w2 = (unsigned long long)wave_sum((long long)c_failed);
	if (lane == 0) { if (w0) atomicAdd(&counts[C_READS], w0); if (w1) atomicAdd(&counts[C_CANDIDATES], w1); if (w2) atomicAdd(&counts[C_FAILED], w2); }
}

// the listed records (all candidates), a wave each
__global__ __launch_bounds__(256) void hx_long_kernel(const uint8_t* __restrict__ infl, const int64_t* __restrict__ recoff, const int64_t* __restrict__ long_list, int64_t n_long,
                                                      int32_t min_match, uint8_t* __restrict__ vd, unsigned long long* __restrict__ counts)
{
	const int lane = threadIdx.x & 63;
	const int64_t nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
	for (int64_t wv = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; wv < n_long; wv += nw)
	{
		const int64_t i = long_list[wv];
		RecView e = load_rec(infl, recoff[i]); rec_apply_cg(e);
		const long long sum = wave_sum(hx_match_sum(e.cigar, e.n_cigar, (uint32_t)lane, 64));
		if (lane) continue;
		const uint8_t v = hx_verdict(true, sum, min_match);
		vd[i] = v;
		if (v == HX_FAILED && counts) atomicAdd(&counts[C_FAILED], 1ull);
	}
}

// the gather's flag mask (recwrite.h's gather_kernel): 0x104 for a failed record
struct HxMask { const uint8_t* vd; __device__ uint32_t operator()(int64_t i) const { return hx_flag_mask(vd[i]); } };

const char* const TOOL = "BamCleanHaloplex";

// the verdicts of a tile: the lane-per-record kernel; then, once the host knows how many records were listed, the wave-per-record kernel
struct Verdicts
{
	DevBuf<uint8_t> vd; DevBuf<int64_t> long_list; DevBuf<unsigned long long> long_count; unsigned long long n_long = 0;
	void begin(const uint8_t* infl, const int64_t* rec, int64_t n, int32_t min_match, uint64_t* sz, unsigned long long* counts, hipStream_t s)
	{
		const char* w = "the verdicts";
		grow(vd, (size_t)n + 1, w, TOOL); grow(long_list, (size_t)n + 1, w, TOOL);
		if (!long_count.p) long_count.alloc(1);
		HIPCHK(hipMemsetAsync(long_count.p, 0, sizeof(unsigned long long), s));
		hipLaunchKernelGGL(hx_verdict_kernel, dim3(grid_for(n)), dim3(256), 0, s, infl, rec, n, min_match, vd.p, sz, long_list.p, long_count.p, counts); KCHECK();
	}
	// the number of listed records to the host: queued by the caller next to its other copies (a copy to pageable memory holds the host until the stream has
	// come that far, so it goes behind everything that can be queued first); valid behind the caller's next wait for the stream
	void fetch(hipStream_t s) { HIPCHK(hipMemcpyAsync(&n_long, long_count.p, sizeof(unsigned long long), hipMemcpyDeviceToHost, s)); }
	void finish(const uint8_t* infl, const int64_t* rec, int64_t n, int32_t min_match, unsigned long long* counts, hipStream_t s)
	{
		if (!n_long) return;
		if ((int64_t)n_long > n) throw std::runtime_error("BamCleanHaloplex: more long CIGARs listed than the tile has records");
		hipLaunchKernelGGL(hx_long_kernel, dim3(grid_for((int64_t)n_long, 4)), dim3(256), 0, s, infl, rec, long_list.p, (int64_t)n_long, min_match, vd.p, counts); KCHECK();
	}
};
} // namespace

namespace lib {
void clean_haloplex(ngsqc_handle* h, int32_t min_match, const char* out_path, ngsqc_haloplex_counts* cnt)
{
	if (!out_path || !cnt) throw ArgError("null argument");
	require_whole_file(h, TOOL);
	const bool timing = h->sw.timing;
	hipStream_t s = h->stream;
	const double t_w = wall_ms();
	const int64_t W = write_window_bytes(h->sw.write_window_pieces);
	BgzfStream out(TOOL, W, -1);
	open_bam(out, out_path, h, s);
	Verdicts vb; DevBuf<uint8_t> tmp; DevBuf<uint64_t> sz, off;
	DevBuf<unsigned long long> counts; counts.alloc(C_N); HIPCHK(hipMemsetAsync(counts.p, 0, C_N * sizeof(unsigned long long), s));
	StageClock ck_verdict(timing, s), ck_long(timing, s), ck_scan(timing, s), ck_gather(timing, s);
	double ms_tiles = 0; int64_t n_tiles = 0, n_records = 0, n_listed = 0;
	EagerRecoff eager(h);
	stream_tiles(h, [&](const TileCtx& c) {
		const double t0 = wall_ms();
		const int64_t n = c.n_rec;
		if (n == 0) return true;
		const int64_t* rec = ensure_recoff(h);
		const char* w = "the record sizes";
		grow(sz, (size_t)n + 1, w, TOOL); grow(off, (size_t)n + 1, w, TOOL);
		grow(tmp, scan_tmp_bytes((size_t)n, s) + 16, w, TOOL);
		ck_verdict.mark();
		vb.begin(c.infl, rec, n, min_match, sz.p, counts.p, s);
		ck_verdict.mark();
		// the position of every record in the stream, behind the carried partial piece
		ck_scan.mark();
		out.place(tmp, sz.p, off.p, n, s);
		ck_scan.mark();
		vb.fetch(s);
		HIPCHK(hipStreamSynchronize(s));   // (the totals and the number of listed records are on the host)
		ck_long.mark();
		vb.finish(c.infl, rec, n, min_match, counts.p, s);
		ck_long.mark();
		n_listed += (int64_t)vb.n_long;
		const double dz0 = out.ms_deflate + out.ms_copy;
		out.emit(out.placed_end(n), s, h->device, [&](const Win& win, int64_t ws) {
			ck_gather.mark();
			launch_gather<false>(FromTile{c.infl, rec}, HxMask{vb.vd.p}, sz.p, off.p, n, ws, win, s);
			ck_gather.mark();
		});
		HIPCHK(hipStreamSynchronize(s));   // (the tile's bytes are no longer read)
		ms_tiles += wall_ms() - t0 - (out.ms_deflate + out.ms_copy - dz0); ++n_tiles; n_records += n;
		return true;
	});
	unsigned long long dc[C_N] = {0, 0, 0};
	HIPCHK(hipMemcpyAsync(dc, counts.p, sizeof(dc), hipMemcpyDeviceToHost, s)); HIPCHK(hipStreamSynchronize(s));
	out.close(s, h->device, out_path);
	cnt->reads = (int64_t)dc[C_READS]; cnt->candidates = (int64_t)dc[C_CANDIDATES]; cnt->failed = (int64_t)dc[C_FAILED];
	if (timing)
		fprintf(stderr, "[ngsqc] clean_haloplex: %.1f ms in all: verdicts and scan %.1f ms on the host's clock (by HIP events: verdict kernel %.1f ms, long-CIGAR kernel %.1f ms for %lld listed records, scan %.1f ms, and "
		                "gather kernel %.1f ms, which the host's clock books with the deflate stage that waits for it; %lld records in %lld tiles; K1 %.1f ms and K2 %.1f ms of the input), deflate %.1f ms, copy to pinned memory %.1f ms, "
		                "file writes %.1f ms (host thread), windows of %lld bytes\n",
		        wall_ms() - t_w, ms_tiles, ck_verdict.total(), ck_long.total(), (long long)n_listed, ck_scan.total(), ck_gather.total(), (long long)n_records, (long long)n_tiles, h->tm.inflate_ms, h->tm.index_ms,
		        out.ms_deflate, out.ms_copy, out.sink.write_ms, (long long)W);
}

void haloplex_verdicts(ngsqc_handle* h, int32_t min_match, uint8_t* out, int64_t cap)
{
	if (cap < 0 || (cap && !out)) throw ArgError("null argument");
	require_whole_file(h, TOOL);
	hipStream_t s = h->stream;
	Verdicts vb;
	for_each_tile_bytes(h, out, cap, "the verdict buffer is smaller than the number of records", [&](const TileCtx& c, const int64_t* rec, int64_t n) {
		vb.begin(c.infl, rec, n, min_match, nullptr, nullptr, s);
		vb.fetch(s); HIPCHK(hipStreamSynchronize(s));
		vb.finish(c.infl, rec, n, min_match, nullptr, s);
		return vb.vd.p;
	});
}
} // namespace lib
} // namespace ngsqc

int ngsqc_clean_haloplex(ngsqc_handle* h, int32_t min_match, const char* out_bam_path, ngsqc_haloplex_counts* counts)
{
	if (!h || !out_bam_path || !counts) return NGSQC_E_ARG;   // (before a device is touched)
	return guarded(h, [&] { ngsqc::lib::clean_haloplex(h, min_match, out_bam_path, counts); });
}

int ngsqc_haloplex_verdicts(ngsqc_handle* h, int32_t min_match, uint8_t* out, int64_t cap)
{
	if (!h || cap < 0 || (cap && !out)) return NGSQC_E_ARG;
	return guarded(h, [&] { ngsqc::lib::haloplex_verdicts(h, min_match, out, cap); });
}
