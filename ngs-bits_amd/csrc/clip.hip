// BamClipOverlap on the device (src/BamClipOverlap/main.cpp:43-554, NGSHelper::softClipAlignment): the preconditions, the mate join by read name, the visit of every
// closed pair, the records with their rewritten CIGAR, and the BGZF writer (ngsqc_clip_overlap); the plan of every record on its own (ngsqc_clip_overlap_plan).
//
// One pass over the tiles (stream_tiles); the join and the writer are join.h's (NameJoin, BgzfStream), the bytes of an unchanged record recwrite.h's, the visit
// of a pair and the bytes of its two records clip_visit.h's (free of HIP: tests/emul/clip_emul.cpp holds the same text against the literal restatement). Per tile:
//   1. keys: a record that fails a precondition (:69-92, on the CIGAR a CG tag gives it) gets KEY_NONE and is written at its own place, every other record its
//      name hash. info = pass bit | the record's ordinal in the file (a held opener keeps its whole record; the ordinal puts the names still open at the end
//      back into file order and addresses the plan). The join closes the 1st and 2nd record of a name, a 3rd opens again (QHash::take).
//   2. flags: per closed pair the geometric test alone (soft_clip, :113-126). Their exclusive scan in closer order, started at the count of the tiles before,
//      is reads_clipped / 2 at every pair: its parity decides which mate an indel near the clip position sends the whole clip to (:479-491). It counts pairs
//      that -overlap_mismatch_remove drops as well, and nothing else of a pair's visit reaches a later pair.
//   3. plan: a thread per pair runs the visit (clip_visit.h visit_pair): the sizes of the two records as written (0 for a removed pair), the counters, the
//      error. A thread, not a wave, also for long CIGARs: the visit is sequential in the CIGAR's operations and both mates may be long; a pair of long reads
//      costs its thread their length, and the other lanes of its wave wait for it.
//   4. sizes -> stream positions (exclusive scan behind the carried partial piece): a record adds itself (written through), nothing (an opener, an open
//      name, the closer of a removed pair) or the pair it closes, forward read first - which may be the closer.
//   5. gather: a wave per record that adds something. A pair that is not soft-clipped leaves as it came (write_record); for a soft-clipped one the wave runs
//      the visit again (write_pair): the copies are strided over the lanes, lane 0 lays the new CIGAR, the patched bases or qualities and the BS tag over them.
//      The tile and the held copies of openers stay the input's bytes.
//   6. behind the last tile the names still open are written in file order (the reference writes them in QHash order, which it leaves open).
// The earliest error in file order (by the closer's ordinal) stops the run.
#include "recwrite.h"
#include "clip_visit.h"

namespace ngsqc {

namespace {
using namespace clip;
enum { C_PASS, C_BASES, C_MISMATCH_PAIRS, C_BASES_CLIPPED, C_ERR_ORD, C_N };
constexpr uint32_t INFO_PASS = 0x80000000u, INFO_ORD = 0x7fffffffu;

struct WinSink
{
	Win w;
	__device__ void operator()(long long at, uint8_t v) const { if (at >= w.lo && at < w.hi) w.base[at] = v; }
	__device__ void fence() const { __threadfence_block(); }
};

__device__ __forceinline__ void plan_row(int32_t* plan, int64_t cap, int64_t ord, int role, const MateOut& m)
{
	if (!plan || ord >= cap) return;
	int32_t* p = plan + 6 * ord;
	p[0] = role; p[1] = m.clip; p[2] = m.pos; p[3] = m.n_cigar; p[4] = m.tlen; p[5] = m.bits;
}

// entries: [0, H) held, [H, H + n) the tile's records. joins[i]: the record enters the name map
__global__ __launch_bounds__(256) void clip_keys_kernel(const uint8_t* __restrict__ infl, const int64_t* __restrict__ recoff, int64_t n, int64_t H, int64_t ord_base, uint64_t mask,
                                                        uint64_t* __restrict__ key, uint32_t* __restrict__ val, uint64_t* __restrict__ src, uint32_t* __restrict__ info, uint8_t* __restrict__ jn,
                                                        unsigned long long* __restrict__ counts, int32_t* __restrict__ plan, int64_t plan_cap)
{
	const int64_t stride = (int64_t)gridDim.x * blockDim.x, N = H + n;
	const int lane = threadIdx.x & 63;
	for (int64_t e0 = (int64_t)blockIdx.x * blockDim.x; e0 < N; e0 += stride)   // (the whole wave takes every turn: wave_sum)
	{
		const int64_t e = e0 + threadIdx.x;
		long long bases = 0, pass = 0;
		if (e < N)
		{
			val[e] = (uint32_t)e;
			if (e >= H)
			{
				const int64_t i = e - H;
				RecView r = load_rec(infl, recoff[i]); rec_apply_cg(r);
				src[e] = (uint64_t)(uintptr_t)(infl + recoff[i]);
				const bool j = joins(r);
				key[e] = j ? rec_name_hash(r) & mask : KEY_NONE;
				info[e] = INFO_PASS | ((uint32_t)(ord_base + i) & INFO_ORD);
				jn[i] = j ? 1 : 0;
				bases = r.l_seq; pass = j ? 0 : 1;
				plan_row(plan, plan_cap, ord_base + i, j ? ROLE_LEFTOVER : ROLE_PASS, MateOut{0, r.pos, (int)r.n_cigar, r.isize, 0, 0});
			}
		}
		bases = wave_sum(bases); pass = wave_sum(pass);
		if (lane == 0) { if (bases) atomicAdd(&counts[C_BASES], (unsigned long long)bases); if (pass) atomicAdd(&counts[C_PASS], (unsigned long long)pass); }
	}
}

__device__ __forceinline__ void pair_views(const uint8_t* a, const uint8_t* b, RecView& ra, RecView& rb, RecView& ea, RecView& eb, bool& cg)
{
	ra = load_rec(a, 0); rb = load_rec(b, 0); ea = ra; eb = rb; rec_apply_cg(ea); rec_apply_cg(eb);
	cg = ea.cigar != ra.cigar || eb.cigar != rb.cigar;
}

__global__ __launch_bounds__(256) void clip_flags_kernel(const int64_t* __restrict__ close_of, const uint64_t* __restrict__ src, int64_t n, int64_t H, uint64_t* __restrict__ flag)
{
	const int64_t stride = (int64_t)gridDim.x * blockDim.x;
	for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
	{
		const int64_t c = close_of[i];
		uint64_t f = 0;
		if (c >= 0)
		{
			RecView ra, rb, ea, eb; bool cg;
			pair_views((const uint8_t*)(uintptr_t)src[c >> 1], (const uint8_t*)(uintptr_t)src[H + i], ra, rb, ea, eb, cg);
			f = geometry(ea, eb).soft_clip ? 1 : 0;
		}
		flag[i] = f;
	}
}

// par[i]: the soft-clipped pairs in front of record i in the whole file. sz[i]: the bytes record i adds to the output; err[3 i ..]: the code and its two integers
__global__ __launch_bounds__(256) void clip_plan_kernel(const int64_t* __restrict__ close_of, const uint8_t* __restrict__ jn, const uint64_t* __restrict__ par, const uint64_t* __restrict__ src,
                                                        const uint32_t* __restrict__ info, int64_t n, int64_t H, int64_t ord_base, int mode, int ignore_indels, uint64_t* __restrict__ sz,
                                                        int32_t* __restrict__ err, unsigned long long* __restrict__ counts, int32_t* __restrict__ plan, int64_t plan_cap)
{
	const int64_t stride = (int64_t)gridDim.x * blockDim.x;
	const int lane = threadIdx.x & 63;
	for (int64_t i0 = (int64_t)blockIdx.x * blockDim.x; i0 < n; i0 += stride)
	{
		const int64_t i = i0 + threadIdx.x;
		long long mm = 0, clipped = 0;
		if (i < n)
		{
			const int64_t c = close_of[i];
			uint64_t size = 0;
			err[3 * i] = E_NONE;
			if (!jn[i]) size = out_size(load_rec((const uint8_t*)(uintptr_t)src[H + i], 0));
			else if (c >= 0)
			{
				RecView ra, rb, ea, eb; bool cg;
				pair_views((const uint8_t*)(uintptr_t)src[c >> 1], (const uint8_t*)(uintptr_t)src[H + i], ra, rb, ea, eb, cg);
				PairOut o;
				visit_pair(ea, eb, cg, mode, ignore_indels != 0, (int)(par[i] & 1), o, NoEmit{}, NoEmit{}, NoMM{});
				if (o.err)
				{
					err[3 * i] = o.err; err[3 * i + 1] = o.ea; err[3 * i + 2] = o.eb;
					atomicMin(&counts[C_ERR_ORD], (unsigned long long)(ord_base + i));
				}
				else
				{
					const RecView& f = o.fwd_is_opener ? ra : rb; const RecView& r = o.fwd_is_opener ? rb : ra;
					if (!o.soft_clip) size = (uint64_t)out_size(ra) + out_size(rb);
					else if (!(o.f.bits & V_REMOVED)) size = (uint64_t)written_size(f, o.f, cigar_text_len(f)) + written_size(r, o.r, cigar_text_len(r));
					if (o.soft_clip) { clipped = o.overlap; mm = o.mismatch ? 1 : 0; }
					const int64_t ord_o = info[c >> 1] & INFO_ORD, ord_c = ord_base + i;
					plan_row(plan, plan_cap, o.fwd_is_opener ? ord_o : ord_c, ROLE_FORWARD, o.f);
					plan_row(plan, plan_cap, o.fwd_is_opener ? ord_c : ord_o, ROLE_REVERSE, o.r);
				}
			}
			sz[i] = size;
		}
		mm = wave_sum(mm); clipped = wave_sum(clipped);
		if (lane == 0) { if (mm) atomicAdd(&counts[C_MISMATCH_PAIRS], (unsigned long long)mm); if (clipped) atomicAdd(&counts[C_BASES_CLIPPED], (unsigned long long)clipped); }
	}
}

// off: the absolute stream position of what record i adds; ws: the stream position of obuf[0]
__global__ __launch_bounds__(256) void clip_gather_kernel(const int64_t* __restrict__ close_of, const uint8_t* __restrict__ jn, const uint64_t* __restrict__ par, const uint64_t* __restrict__ sz,
                                                          const uint64_t* __restrict__ off, int64_t n, int64_t H, const uint64_t* __restrict__ src, int mode, int ignore_indels, int64_t ws, Win w)
{
	const int lane = threadIdx.x & 63;
	const int64_t nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
	for (int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; i < n; i += nw)
	{
		if (!sz[i]) continue;
		const int64_t pos = (int64_t)off[i] - ws;
		if (pos >= w.hi || pos + (int64_t)sz[i] <= w.lo) continue;
		const uint8_t* closer = (const uint8_t*)(uintptr_t)src[H + i];
		if (!jn[i]) { write_record(closer, w, pos, lane); continue; }
		const uint8_t* opener = (const uint8_t*)(uintptr_t)src[close_of[i] >> 1];
		PairOut o; uint32_t sf, sr;
		if (write_pair(opener, closer, mode, ignore_indels != 0, (int)(par[i] & 1), pos, WinSink{w}, lane, 64, o, sf, sr)) continue;
		const uint8_t* first = o.fwd_is_opener ? opener : closer; const uint8_t* second = o.fwd_is_opener ? closer : opener;
		write_record(first, w, pos, lane);
		write_record(second, w, pos + out_size(load_rec(first, 0)), lane);
	}
}

// the names still open at the end, in file order
__global__ __launch_bounds__(256) void clip_left_sizes_kernel(const uint64_t* __restrict__ src, int64_t n, uint64_t* __restrict__ sz)
{
	const int64_t stride = (int64_t)gridDim.x * blockDim.x;
	for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) sz[i] = out_size(load_rec((const uint8_t*)(uintptr_t)src[i], 0));
}

// the reference's message for the pair that the record with ordinal `ord` of the resident tile closes
[[noreturn]] void throw_pair_error(const TileCtx& c, const int64_t* rec, int64_t ord, const int32_t* err_dev, ngsqc_clip_error* out, hipStream_t s)
{
	const int64_t i = ord - c.ord_base;
	if (i < 0 || i >= c.n_rec) throw std::runtime_error("BamClipOverlap: the failing record is not in the resident tile");
	int32_t e[3] = {0, 0, 0};
	HIPCHK(hipMemcpyAsync(e, err_dev + 3 * i, sizeof(e), hipMemcpyDeviceToHost, s));
	const std::string name = fetch_rec_head(c, rec, i, s).name;   // (waits for the stream)
	if (out) *out = ngsqc_clip_error{ord, e[0], e[1], e[2]};
	const std::string ch(1, (char)e[1]);
	switch (e[0])
	{
		case E_CIGAR_CHAR: throw FormatError("Unknown CIGAR character '" + ch + "'");
		case E_LENGTH: throw FormatError("Length mismatch between forward/reverse overlap - forward:" + std::to_string(e[1]) + " reverse:" + std::to_string(e[2]) + " in read with name '" + name + "'");
		case E_SC_ORDER: throw FormatError("End position is smaller than start position.");
		case E_SC_START: throw FormatError("Start position " + std::to_string(e[1]) + " not within alignment of read " + name + ".");
		case E_SC_END: throw FormatError("End position " + std::to_string(e[1]) + " not within alignment of read " + name + ".");
		case E_SC_INDEX: throw FormatError("Index out of boundary!");
		case E_SC_OP: throw FormatError("Unsupported CIGAR type '" + ch + "'");
		case E_BAD_BASE: throw FormatError("Cannot store character '" + ch + "' in BAM/CRAM file. Only A,C,G,T,N are allowed!");
		case E_UNSUPPORTED: throw std::domain_error("BamClipOverlap: clipping a read whose CIGAR is stored in a CG tag, or whose clipped CIGAR has more than 65535 operations, is not supported (read '" + name + "')");
		default: throw FormatError("Read orientation of the pair with name '" + name + "' was not identified.");
	}
}

// out_path == null: the plan alone
void clip_run(ngsqc_handle* h, const char* out_path, int mode, int ignore_indels, int level, int64_t* counts_out, ngsqc_clip_error* err_out, int32_t* plan_out, int64_t plan_cap)
{
	const char* T = "BamClipOverlap";
	require_whole_file(h, T);
	if (mode & ~(MODE_MAPQ | MODE_REMOVE | MODE_BASEQ | MODE_BASEN)) throw ArgError("unknown mode bits");
	if (level < -1 || level > 9) throw ArgError("the compression level is -1 (the default) or 0 .. 9");
	if (err_out) *err_out = ngsqc_clip_error{-1, 0, 0, 0};
	const bool write = out_path != nullptr, timing = h->sw.timing;
	const uint64_t mask = name_hash_mask(h->sw.name_hash_bits);
	hipStream_t s = h->stream;
	const double t_w = wall_ms();
	const int64_t W = write_window_bytes(h->sw.write_window_pieces);
	BgzfStream out(T, W, level);
	NameJoin j(T, s);
	DevBuf<uint64_t> flag, par, sz, off; DevBuf<uint8_t> jn; DevBuf<int32_t> err, plan;
	DevBuf<unsigned long long> counts; counts.alloc(C_N);
	HIPCHK(hipMemsetAsync(counts.p, 0, C_N * sizeof(unsigned long long), s)); HIPCHK(hipMemsetAsync(counts.p + C_ERR_ORD, 0xff, sizeof(unsigned long long), s));
	if (plan_out) { grow(plan, (size_t)(6 * plan_cap) + 6, "the plan", T); if (plan_cap) HIPCHK(hipMemsetAsync(plan.p, 0, (size_t)(6 * plan_cap) * sizeof(int32_t), s)); }
	if (write) open_bam(out, out_path, h, s);
	StageClock ck_join(timing, s), ck_plan(timing, s), ck_gather(timing, s);
	int64_t n_reads = 0; uint64_t clipped_pairs = 0;
	EagerRecoff eager(h);
	stream_tiles(h, [&](const TileCtx& c) {
		const int64_t n = c.n_rec, H = j.H, N = H + n;
		const int64_t* rec = n ? ensure_recoff(h) : nullptr;
		if (c.ord_base + n > (int64_t)INFO_ORD) throw ArgError("BamClipOverlap: more than 2^31 - 1 records");
		if (plan_out && c.ord_base + n > plan_cap) throw ArgError("the plan buffer is smaller than the number of records");
		n_reads += n;
		j.begin_tile(n, s);
		const char* w = "the pair plan";
		grow(flag, (size_t)n + 1, w, T); grow(par, (size_t)n + 1, w, T); grow(sz, (size_t)n + 1, w, T); grow(off, (size_t)n + 1, w, T); grow(jn, (size_t)n + 1, w, T); grow(err, 3 * (size_t)n + 3, w, T);
		if (N == 0) return true;
		ck_join.mark();
		hipLaunchKernelGGL(clip_keys_kernel, dim3(grid_for(N)), dim3(256), 0, s, c.infl, rec, n, H, c.ord_base, mask, j.key.p, j.val.p, j.src.p, j.info.p, jn.p, counts.p, plan.p, plan_out ? plan_cap : 0); KCHECK();
		j.sort_resolve(n, s);
		ck_join.mark();
		uint64_t ptot[2] = {0, 0}; unsigned long long err_ord = ~0ull;
		if (n)
		{
			ck_plan.mark();
			hipLaunchKernelGGL(clip_flags_kernel, dim3(grid_for(n)), dim3(256), 0, s, j.close_of.p, j.src.p, n, H, flag.p); KCHECK();
			scan_u64(j.tmp, flag.p, par.p, clipped_pairs, (size_t)n, s);
			hipLaunchKernelGGL(clip_plan_kernel, dim3(grid_for(n)), dim3(256), 0, s, j.close_of.p, jn.p, par.p, j.src.p, j.info.p, n, H, c.ord_base, mode, ignore_indels, sz.p, err.p, counts.p,
			                   plan.p, plan_out ? plan_cap : 0); KCHECK();
			ck_plan.mark();
			out.place(j.tmp, sz.p, off.p, n, s);
			HIPCHK(hipMemcpyAsync(&ptot[0], par.p + n - 1, 8, hipMemcpyDeviceToHost, s)); HIPCHK(hipMemcpyAsync(&ptot[1], flag.p + n - 1, 8, hipMemcpyDeviceToHost, s));
			HIPCHK(hipMemcpyAsync(&err_ord, counts.p + C_ERR_ORD, 8, hipMemcpyDeviceToHost, s));
		}
		j.keep_open(n, s);   // (waits for the stream: the placed end, ptot and err_ord are on the host)
		if (err_ord != ~0ull) throw_pair_error(c, rec, (int64_t)err_ord, err.p, err_out, s);
		if (n) clipped_pairs = ptot[0] + ptot[1];
		if (write)
			out.emit(out.placed_end(n), s, h->device, [&](const Win& win, int64_t ws) {
				if (!n) return;
				ck_gather.mark();
				hipLaunchKernelGGL(clip_gather_kernel, dim3(grid_for(n, 4)), dim3(256), 0, s, j.close_of.p, jn.p, par.p, sz.p, off.p, n, H, j.src.p, mode, ignore_indels, ws, win); KCHECK();
				ck_gather.mark();
			});
		HIPCHK(hipStreamSynchronize(s));   // (the old pool and the tile's bytes are no longer read)
		j.end_tile();
		return true;
	});
	// the names still open, in file order
	const int64_t L = j.H;
	if (write && L)
	{
		// (their ordinals ride in the low 31 bits of the held info words, which all carry the pass bit: a radix sort of the words is a sort by ordinal)
		DevBuf<uint32_t> okey; DevBuf<uint64_t> lsrc;
		grow(okey, (size_t)L + 1, "the open names", T); grow(lsrc, (size_t)L + 1, "the open names", T);
		size_t tb = 0;
		(void)rocprim::radix_sort_pairs(nullptr, tb, j.hi.p, okey.p, j.hs.p, lsrc.p, (size_t)L, 0, 32, s);
		grow(j.tmp, tb + 16, "the open names", T);
		tb = j.tmp.n;
		if (rocprim::radix_sort_pairs(j.tmp.p, tb, j.hi.p, okey.p, j.hs.p, lsrc.p, (size_t)L, 0, 32, s) != hipSuccess) throw std::runtime_error("rocprim::radix_sort_pairs failed");
		grow(sz, (size_t)L + 1, "the open names", T); grow(off, (size_t)L + 1, "the open names", T);
		grow(j.tmp, scan_tmp_bytes((size_t)L, s) + 16, "the open names", T);
		hipLaunchKernelGGL(clip_left_sizes_kernel, dim3(grid_for(L)), dim3(256), 0, s, lsrc.p, L, sz.p); KCHECK();
		out.place(j.tmp, sz.p, off.p, L, s);
		HIPCHK(hipStreamSynchronize(s));
		out.emit(out.placed_end(L), s, h->device, [&](const Win& win, int64_t ws) { launch_gather<false>(FromPtrs{lsrc.p}, NoMask{}, sz.p, off.p, L, ws, win, s); });
		HIPCHK(hipStreamSynchronize(s));
	}
	unsigned long long jc[4] = {0, 0, 0, 0}, dc[C_N];
	j.read_counts(jc, s);
	HIPCHK(hipMemcpyAsync(dc, counts.p, sizeof(dc), hipMemcpyDeviceToHost, s)); HIPCHK(hipStreamSynchronize(s));
	if (write) out.close(s, h->device, out_path);
	if (plan_out && n_reads) { HIPCHK(hipMemcpyAsync(plan_out, plan.p, (size_t)(6 * n_reads) * sizeof(int32_t), hipMemcpyDeviceToHost, s)); HIPCHK(hipStreamSynchronize(s)); }
	if (counts_out)
	{
		counts_out[0] = n_reads; counts_out[1] = (int64_t)dc[C_PASS] + 2 * (int64_t)(jc[0] + jc[1]) + L; counts_out[2] = 2 * (int64_t)clipped_pairs;
		counts_out[3] = 2 * (int64_t)dc[C_MISMATCH_PAIRS]; counts_out[4] = (int64_t)dc[C_BASES]; counts_out[5] = (int64_t)dc[C_BASES_CLIPPED];
	}
	if (timing)
		fprintf(stderr, "[ngsqc] clip_overlap%s: %.1f ms in all; by HIP events: keys and join %.1f ms, flags, parity scan and plan %.1f ms, gather %.1f ms; deflate %.1f ms, copy to pinned memory "
		                "%.1f ms, file writes %.1f ms (host thread); K1 %.1f ms and K2 %.1f ms of the input; %lld open names at the end, windows of %lld bytes\n",
		        write ? "" : "_plan", wall_ms() - t_w, ck_join.total(), ck_plan.total(), ck_gather.total(), out.ms_deflate, out.ms_copy, out.sink.write_ms, h->tm.inflate_ms, h->tm.index_ms,
		        (long long)L, (long long)W);
}
} // namespace
} // namespace ngsqc

int ngsqc_clip_overlap(ngsqc_handle* h, const char* out_bam_path, int32_t mode_bits, int32_t ignore_indels, int32_t level, int64_t* counts, ngsqc_clip_error* err)
{
	if (!h || !out_bam_path || !counts) return NGSQC_E_ARG;   // (before a device is touched)
	return guarded(h, [&] { ngsqc::clip_run(h, out_bam_path, mode_bits, ignore_indels, level, counts, err, nullptr, 0); });
}

int ngsqc_clip_overlap_plan(ngsqc_handle* h, int32_t mode_bits, int32_t ignore_indels, int32_t* plan, int64_t cap_records, ngsqc_clip_error* err)
{
	if (!h || cap_records < 0 || (cap_records && !plan)) return NGSQC_E_ARG;
	return guarded(h, [&] { ngsqc::clip_run(h, nullptr, mode_bits, ignore_indels, -1, nullptr, err, plan ? plan : (int32_t*)nullptr, cap_records); });
}
