// BamRemoveVariants on the device (src/BamRemoveVariants/main.cpp:34-278): a verdict per record against a table of VCF lines, the pair decision, the gather and,
// with -mask, the sequence patch in the gathered copy (ngsqc_remove_variants, ngsqc_variant_verdicts).
//
// One pass over the tiles (stream_tiles); the join and the writer are join.h's (NameJoin, BgzfStream), the record layout recwrite.h's. Per tile:
//   1. verdict: one thread per record walks the table lines its span overlaps, in table order (alignment_pass :34-66, mask_alignment :68-110), and writes the
//      join's key, source pointer and info word (bit 31: passes, bit 30: modified, below: the size in the output) and a verdict byte. The first candidate line is
//      found by binary search on the running maximum of `end` (end is not monotone: a long REF lies in front of the lines it covers); the visit stops at
//      beg > record end. Records with more than LONG_CIGAR operations go on a list to a wave-per-record kernel that gives every lane a line.
//   2. the join (paired mode), then one thread per record: the size of the pair a record closes, the `modified` of closers whose opener failed (the reference
//      never visits them, :218), the earliest record whose error counts.
//   3. gather: a wave per kept pair (or record) copies the records into the output window; for a modified record the same wave runs the visit again on the
//      source bytes and stores the bytes of the sequence that differ. The tile and the held copies of openers stay the input's bytes: other jobs read the tile, and
//      a held opener is patched in whichever later tile closes it. A stored byte is computed from the source alone (both nibbles after every line of the visit),
//      so a record that straddles two windows gets the same bytes in both launches, and lanes that store the same byte store the same value.
// With -mask a later line sees what an earlier line wrote (:92-95). No state is kept for that: the base at read index p in front of line k is the source's
// nibble folded over the SNV lines j < k of the visit whose index is p (nib_at) - quadratic in the lines of one read, which a VCF of one sample keeps small.
// A record with tid < 0 indexes chrs_[-1] in the reference (undefined there); here it overlaps nothing and passes as it is.
#include "recwrite.h"
#include "rmvar_visit.h"

namespace ngsqc {

namespace {
enum { C_SKIPPED, C_MODIFIED, C_MOD_MINUS, C_SE_PASSED, C_SE_DROPPED, C_ERR_ORD, C_N };
constexpr uint32_t INFO_PASS = 0x80000000u, INFO_MOD = 0x40000000u, INFO_SIZE = 0x3fffffffu;

// the same visit by a wave: a lane per line, 64 lines at a time; the first line in table order that ends the visit decides
__device__ Verdict visit_wave(const RecView& r, const RmTable& T, const RmMode& m, int lane, Span& sp)
{
	Verdict out{V_PASS, -1, 0};
	if (!rec_span(r, T, sp)) { sp.a = sp.last = 0; return out; }
	bool pass = true; int eff = 0, bad = -2; int32_t E = sp.last;
	for (int32_t k0 = sp.a; k0 < sp.last; k0 += 64)
	{
		const int32_t k = k0 + lane;
		const bool valid = k < sp.last && T.v[k].beg <= sp.re;   // (beg does not decrease: the valid lanes are the first ones)
		const int n_valid = __popcll(__ballot(valid));
		LineOut o{L_NONE, 0, -1, 0, 0};
		if (valid) o = eval_line(r, T, sp, k, m, bad);
		const bool term = o.code == L_ERR || o.code == L_OTHER || (o.code == L_SNV && !m.mask);
		const unsigned long long tb = __ballot(term);
		const int first = tb ? __ffsll((long long)tb) - 1 : 64;
		eff += __popcll(__ballot(lane < first && o.code == L_SNV && o.old_nib != o.ref_nib));
		if (tb)
		{
			const int code = __shfl(o.code, first), err = __shfl(o.err, first), ap = __shfl(o.ap, first);
			E = k0 + first;
			if (code == L_ERR) { out.bits = V_ERR | (uint32_t)err << 4; out.ev = ap; out.E = E; return out; }
			pass = code == L_OTHER && m.mask && m.keep_indels;
			break;
		}
		if (n_valid < 64) { E = k0 + n_valid; break; }
	}
	out.E = E;
	bool mod = eff == 1;
	if (eff > 1)
	{
		bool mine = false;
		for (int32_t q = sp.a + lane; q < E; q += 64)
		{
			const LineOut o = eval_line(r, T, sp, q, m, bad);
			mine |= o.code == L_SNV && nib_at(r, T, sp, E, o.ap) != seq_nib(r, o.ap);
		}
		mod = __any(mine);
	}
	out.bits = (pass ? V_PASS : 0) | (mod ? V_MOD : 0);
	return out;
}

struct VerdictOut { uint64_t* key; uint32_t* val; uint64_t* src; uint32_t* info; uint8_t* vd; int32_t* ev; unsigned long long* counts; };   // key == null: the verdict bytes alone

__device__ __forceinline__ void store_verdict(const VerdictOut& o, int64_t H, int64_t i, const RecView& r, const Verdict& v, const RmMode& m)
{
	o.vd[i] = (uint8_t)v.bits; o.ev[i] = v.ev;
	if (!o.key) return;
	o.info[H + i] = out_size(r) | ((v.bits & V_PASS) ? INFO_PASS : 0u) | ((v.bits & V_MOD) ? INFO_MOD : 0u);
	// paired: every participant's (the closers whose opener failed are taken off behind the join); single-end: the written records' (:155-160)
	if ((v.bits & V_MOD) && (!m.single_end || (v.bits & V_PASS))) atomicAdd(&o.counts[C_MODIFIED], 1ull);
}

// entries: [0, H) held, [H, H + n) the tile's records
__global__ __launch_bounds__(256) void rm_verdict_kernel(const uint8_t* __restrict__ infl, const int64_t* __restrict__ recoff, int64_t n, int64_t H, RmTable T, RmMode m, uint64_t hash_mask,
                                                         VerdictOut o, int64_t* __restrict__ long_list, unsigned long long* __restrict__ long_count)
{
	const int64_t stride = (int64_t)gridDim.x * blockDim.x;
	for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < H + n; e += stride)
	{
		if (o.key) o.val[e] = (uint32_t)e;
		if (e < H) continue;
		const int64_t i = e - H;
		RecView r = load_rec(infl, recoff[i]);
		if (o.key) { o.src[e] = (uint64_t)(uintptr_t)(infl + recoff[i]); o.key[e] = KEY_NONE; }
		if (r.flag & 0x900)
		{
			o.vd[i] = V_SKIP; o.ev[i] = -1;
			if (o.key) { o.info[e] = 0; atomicAdd(&o.counts[C_SKIPPED], 1ull); }
			continue;
		}
		if (o.key && !m.single_end) o.key[e] = rec_name_hash(r) & hash_mask;
		const RecView raw = r;
		rec_apply_cg(r);
		if (r.n_cigar > (uint32_t)LONG_CIGAR) { long_list[atomicAdd(long_count, 1ull)] = i; continue; }   // wave-per-record path (rm_long_kernel)
		store_verdict(o, H, i, raw, visit_seq(r, T, m), m);
	}
}

__global__ __launch_bounds__(256) void rm_long_kernel(const uint8_t* __restrict__ infl, const int64_t* __restrict__ recoff, const int64_t* __restrict__ long_list,
                                                      const unsigned long long* __restrict__ n_long_dev, int64_t H, RmTable T, RmMode m, VerdictOut o)
{
	const int lane = threadIdx.x & 63;
	const int64_t nw = ((int64_t)gridDim.x * blockDim.x) >> 6, n_long = (int64_t)*n_long_dev;
	for (int64_t wv = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; wv < n_long; wv += nw)
	{
		const int64_t i = long_list[wv];
		const RecView raw = load_rec(infl, recoff[i]);
		RecView r = raw; rec_apply_cg(r);
		Span sp;
		const Verdict v = visit_wave(r, T, m, lane, sp);
		if (lane == 0) store_verdict(o, H, i, raw, v, m);
	}
}

// behind the join: the size of the pair record i closes; the modified closers the reference never visits; the earliest error that counts
__global__ __launch_bounds__(256) void rm_pair_post_kernel(const int64_t* __restrict__ close_of, const uint32_t* __restrict__ info, const uint8_t* __restrict__ vd, int64_t n, int64_t H,
                                                           int64_t ord_base, uint64_t* __restrict__ sz, unsigned long long* __restrict__ counts)
{
	const int64_t stride = (int64_t)gridDim.x * blockDim.x;
	for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
	{
		const int64_t c = close_of[i];
		const bool opener_failed = c >= 0 && !(info[c >> 1] & INFO_PASS);
		if (opener_failed && (info[H + i] & INFO_MOD)) atomicAdd(&counts[C_MOD_MINUS], 1ull);
		if ((vd[i] & V_ERR) && !opener_failed) atomicMin(&counts[C_ERR_ORD], (unsigned long long)(ord_base + i));
		sz[i] = c >= 0 && (c & 1) ? (uint64_t)(info[c >> 1] & INFO_SIZE) + (info[H + i] & INFO_SIZE) : 0;
	}
}

__global__ __launch_bounds__(256) void rm_single_post_kernel(const uint32_t* __restrict__ info, const uint8_t* __restrict__ vd, int64_t n, int64_t ord_base, uint64_t* __restrict__ sz,
                                                             unsigned long long* __restrict__ counts)
{
	const int64_t stride = (int64_t)gridDim.x * blockDim.x;
	for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
	{
		sz[i] = 0;
		if (vd[i] & V_SKIP) continue;
		if (vd[i] & V_ERR) atomicMin(&counts[C_ERR_ORD], (unsigned long long)(ord_base + i));
		const bool pass = info[i] & INFO_PASS;
		if (pass) sz[i] = info[i] & INFO_SIZE;
		atomicAdd(&counts[pass ? C_SE_PASSED : C_SE_DROPPED], 1ull);
	}
}

// the sequence of a modified record in its copy at pos (recwrite.h's layout): the visit again on the source bytes, then every byte that holds a stored base
__device__ void patch_record(const uint8_t* __restrict__ s, const Win& w, int64_t pos, int lane, const RmTable& T, const RmMode& m)
{
	const RecView raw = load_rec(s, 0);
	RecView r = raw; rec_apply_cg(r);
	// where seq lands: behind the CIGAR as it is written (a CG-tag CIGAR inline up to 65535 operations, else the two-operation placeholder)
	const uint32_t n_out = r.cigar == raw.cigar ? raw.n_cigar_raw : (r.n_cigar <= 65535u ? r.n_cigar : 2u);
	const int64_t seq_out = pos + 36 + raw.l_name + 4ll * n_out;
	Span sp;
	const Verdict v = visit_wave(r, T, m, lane, sp);
	int bad = -1;   // (a kept record has no error)
	for (int32_t q = sp.a + lane; q < v.E; q += 64)
	{
		const LineOut o = eval_line(r, T, sp, q, m, bad);
		if (o.code != L_SNV) continue;
		const int64_t at = seq_out + (o.ap >> 1);
		if (at >= w.lo && at < w.hi) w.base[at] = patched_byte(r, T, sp, v.E, o.ap);
	}
}

__device__ __forceinline__ void write_patched(const uint8_t* s, uint32_t info, const Win& w, int64_t pos, int lane, const RmTable& T, const RmMode& m)
{
	write_record(s, w, pos, lane);
	if (!(info & INFO_MOD)) return;
	__threadfence_block();   // (the copy's bytes first, then the stored bases over them)
	patch_record(s, w, pos, lane, T, m);
}

// off: absolute stream position of every kept pair; ws: the stream position of obuf[0]
__global__ __launch_bounds__(256) void rm_pair_gather_kernel(const int64_t* __restrict__ close_of, const uint64_t* __restrict__ sz, const uint64_t* __restrict__ off, int64_t n, int64_t H,
                                                             const uint64_t* __restrict__ src, const uint32_t* __restrict__ info, int64_t ws, Win w, RmTable T, RmMode m)
{
	const int lane = threadIdx.x & 63;
	const int64_t nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
	for (int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; i < n; i += nw)
	{
		if (!sz[i]) continue;
		const int64_t pos = (int64_t)off[i] - ws;
		if (pos >= w.hi || pos + (int64_t)sz[i] <= w.lo) continue;
		const uint32_t oe = (uint32_t)(close_of[i] >> 1);
		write_patched((const uint8_t*)(uintptr_t)src[oe], info[oe], w, pos, lane, T, m);
		write_patched((const uint8_t*)(uintptr_t)src[H + i], info[H + i], w, pos + (info[oe] & INFO_SIZE), lane, T, m);
	}
}

__global__ __launch_bounds__(256) void rm_single_gather_kernel(const uint64_t* __restrict__ sz, const uint64_t* __restrict__ off, int64_t n, const uint64_t* __restrict__ src,
                                                               const uint32_t* __restrict__ info, int64_t ws, Win w, RmTable T, RmMode m)
{
	const int lane = threadIdx.x & 63;
	const int64_t nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
	for (int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; i < n; i += nw)
	{
		if (!sz[i]) continue;
		const int64_t pos = (int64_t)off[i] - ws;
		if (pos >= w.hi || pos + (int64_t)sz[i] <= w.lo) continue;
		write_patched((const uint8_t*)(uintptr_t)src[i], info[i], w, pos, lane, T, m);
	}
}

// the table in device memory: the lines of every reference of the BAM in file order, the running maximum of end, the range of every tid
struct RmDevTable
{
	DevBuf<ngsqc_rm_variant> v; DevBuf<int32_t> maxend, tid_first; std::vector<int64_t> orig; std::vector<ngsqc_rm_variant> lines; int32_t n_ref = 0;
	void build(const ngsqc_handle* h, const ngsqc_rm_variant* in, int64_t n, hipStream_t s)
	{
		n_ref = (int32_t)h->ref_names.size();
		std::vector<int64_t> first((size_t)n_ref, -1), count((size_t)n_ref, 0);
		int32_t cur = -1; int32_t prev_beg = 0;
		for (int64_t i = 0; i < n; ++i)
		{
			const ngsqc_rm_variant& x = in[i];
			if (x.kind > NGSQC_RMVAR_INVALID) throw ArgError("unknown kind of variant line " + std::to_string(i));
			if (x.tid < 0 || x.tid >= n_ref) continue;
			if (x.tid != cur)
			{
				if (first[(size_t)x.tid] >= 0) throw ArgError("the variant lines of a chromosome are not contiguous (line " + std::to_string(i) + "): the VCF is not sorted");
				first[(size_t)x.tid] = i; cur = x.tid;
			}
			else if (x.beg < prev_beg) throw ArgError("the variant lines are not sorted by position (line " + std::to_string(i) + "): the VCF is not sorted");
			prev_beg = x.beg; ++count[(size_t)x.tid];
		}
		std::vector<int32_t> tf((size_t)n_ref + 1, 0), me;
		for (int32_t t = 0; t < n_ref; ++t)
		{
			tf[(size_t)t] = (int32_t)lines.size();
			if (first[(size_t)t] < 0) continue;
			int32_t run = INT32_MIN; int64_t got = 0;
			for (int64_t i = first[(size_t)t]; got < count[(size_t)t]; ++i)
			{
				if (in[i].tid != t) continue;   // (lines of no reference of the BAM lie between)
				run = std::max(run, in[i].end); lines.push_back(in[i]); me.push_back(run); orig.push_back(i); ++got;
			}
		}
		tf[(size_t)n_ref] = (int32_t)lines.size();
		if (lines.size() > (size_t)INT32_MAX - 64) throw ArgError("too many variant lines");
		lines.push_back(ngsqc_rm_variant{-1, 0, 0, 0, 0, 0, 0, 0}); me.push_back(0);   // (never empty)
		v.upload(lines, s); maxend.upload(me, s); tid_first.upload(tf, s);
		HIPCHK(hipStreamSynchronize(s));
	}
	RmTable table() const { return RmTable{v.p, maxend.p, tid_first.p, n_ref}; }
};

// the verdicts of a tile: the thread-per-record kernel, then the listed long records
struct VerdictBufs
{
	DevBuf<uint8_t> vd; DevBuf<int32_t> ev; DevBuf<int64_t> long_list; DevBuf<unsigned long long> long_count;
	void run(const uint8_t* infl, const int64_t* rec, int64_t n, int64_t H, const RmTable& T, const RmMode& m, uint64_t hash_mask, VerdictOut o, hipStream_t s)
	{
		const char* T_ = "BamRemoveVariants"; const char* w = "the verdicts";
		grow(vd, (size_t)n + 1, w, T_); grow(ev, (size_t)n + 1, w, T_); grow(long_list, (size_t)n + 1, w, T_);
		if (!long_count.p) long_count.alloc(1);
		HIPCHK(hipMemsetAsync(long_count.p, 0, sizeof(unsigned long long), s));
		o.vd = vd.p; o.ev = ev.p;
		hipLaunchKernelGGL(rm_verdict_kernel, dim3(grid_for(H + n)), dim3(256), 0, s, infl, rec, n, H, T, m, hash_mask, o, long_list.p, long_count.p); KCHECK();
		if (n) { hipLaunchKernelGGL(rm_long_kernel, dim3(grid_for(n, 4)), dim3(256), 0, s, infl, rec, long_list.p, long_count.p, H, T, m, o); KCHECK(); }   // (sized for the most there can be)
	}
};

// the reference's message for the record with ordinal `ord` of the resident tile
[[noreturn]] void throw_record_error(const TileCtx& c, const int64_t* rec, int64_t ord, const VerdictBufs& vb, const RmDevTable& tab, ngsqc_rm_counts* cnt, hipStream_t s)
{
	const int64_t i = ord - c.ord_base;
	if (i < 0 || i >= c.n_rec) throw std::runtime_error("BamRemoveVariants: the failing record is not in the resident tile");
	uint8_t vd = 0; int32_t ev = -1;
	HIPCHK(hipMemcpyAsync(&vd, vb.vd.p + i, 1, hipMemcpyDeviceToHost, s)); HIPCHK(hipMemcpyAsync(&ev, vb.ev.p + i, 4, hipMemcpyDeviceToHost, s));
	const RecHead rh = fetch_rec_head(c, rec, i, s);   // (waits for the stream)
	const uint8_t* head = rh.head; const std::string& name = rh.name;
	const int code = vd >> 4 & 3;
	cnt->err_record = ord; cnt->err_code = code; cnt->err_variant = code == NGSQC_RMERR_BAD_BASE ? ev : (int32_t)tab.orig[(size_t)ev];
	int32_t pos; memcpy(&pos, head + 8, 4);
	if (code == NGSQC_RMERR_POS_NOT_FOUND)
		throw FormatError("Could not find position " + std::to_string(tab.lines[(size_t)ev].start) + " in read " + name + " with start position " + std::to_string((long long)pos + 1) + "!");
	if (code == NGSQC_RMERR_BAD_BASE)
	{
		// (the base itself: one more byte of the record)
		uint32_t w2 = 0; memcpy(&w2, head + 16, 4);
		uint8_t b = 0; HIPCHK(hipMemcpy(&b, c.infl + rh.off + 36 + head[12] + 4ll * (w2 & 0xffff) + (ev >> 1), 1, hipMemcpyDeviceToHost));
		throw FormatError(std::string("Cannot store character '") + "=ACMGRSVTWYHKDBN"[(b >> ((~ev & 1) << 2)) & 15] + "' in BAM/CRAM file. Only A,C,G,T,N are allowed!");
	}
	throw FormatError("BamRemoveVariants: read " + name + " visits variant line " + std::to_string(cnt->err_variant) + ", which is no valid variant");
}
} // namespace

namespace lib {
void remove_variants(ngsqc_handle* h, const ngsqc_rm_variant* variants, int64_t n_var, const ngsqc_rm_params* p, const char* out_path, ngsqc_rm_counts* cnt)
{
	if (!p || !out_path || !cnt || n_var < 0 || (n_var && !variants)) throw ArgError("null argument");
	const char* TOOL = "BamRemoveVariants";
	require_whole_file(h, TOOL);
	const RmMode m{p->mask ? 1 : 0, p->single_end ? 1 : 0, p->keep_indels ? 1 : 0};
	const uint64_t hash_mask = name_hash_mask(h->sw.name_hash_bits);
	const bool timing = h->sw.timing;
	hipStream_t s = h->stream;
	*cnt = ngsqc_rm_counts{0, 0, 0, 0, -1, 0, -1};
	const double t_w = wall_ms();
	RmDevTable tab; tab.build(h, variants, n_var, s);
	const RmTable T = tab.table();
	const double ms_table = wall_ms() - t_w;
	const int64_t W = write_window_bytes(h->sw.write_window_pieces);
	BgzfStream out(TOOL, W, -1);
	NameJoin j(TOOL, s);
	VerdictBufs vb;
	DevBuf<uint64_t> sz, off; DevBuf<unsigned long long> counts; counts.alloc(C_N);
	HIPCHK(hipMemsetAsync(counts.p, 0, C_N * sizeof(unsigned long long), s)); HIPCHK(hipMemsetAsync(counts.p + C_ERR_ORD, 0xff, sizeof(unsigned long long), s));
	StageClock ck_verdict(timing, s), ck_gather(timing, s);
	double ms_tiles = 0;
	open_bam(out, out_path, h, s);
	EagerRecoff eager(h);
	stream_tiles(h, [&](const TileCtx& c) {
		const double t0 = wall_ms();
		const int64_t n = c.n_rec, H = j.H, N = H + n;   // (single-end: nothing is ever held, H stays 0)
		const int64_t* rec = n ? ensure_recoff(h) : nullptr;
		j.begin_tile(n, s);
		grow(sz, (size_t)N + 1, "the record sizes", TOOL); grow(off, (size_t)N + 1, "the record sizes", TOOL);
		if (N == 0) return true;
		ck_verdict.mark();
		vb.run(c.infl, rec, n, H, T, m, hash_mask, VerdictOut{j.key.p, j.val.p, j.src.p, j.info.p, nullptr, nullptr, counts.p}, s);
		ck_verdict.mark();
		if (!m.single_end) j.sort_resolve(n, s);
		unsigned long long err_ord = ~0ull;
		if (n)
		{
			if (m.single_end) { hipLaunchKernelGGL(rm_single_post_kernel, dim3(grid_for(n)), dim3(256), 0, s, j.info.p, vb.vd.p, n, c.ord_base, sz.p, counts.p); KCHECK(); }
			else { hipLaunchKernelGGL(rm_pair_post_kernel, dim3(grid_for(n)), dim3(256), 0, s, j.close_of.p, j.info.p, vb.vd.p, n, H, c.ord_base, sz.p, counts.p); KCHECK(); }
			out.place(j.tmp, sz.p, off.p, n, s);
			HIPCHK(hipMemcpyAsync(&err_ord, counts.p + C_ERR_ORD, 8, hipMemcpyDeviceToHost, s));
		}
		if (m.single_end) HIPCHK(hipStreamSynchronize(s));
		else j.keep_open(n, s);   // (waits for the stream: the placed end and err_ord are on the host)
		if (err_ord != ~0ull) throw_record_error(c, rec, (int64_t)err_ord, vb, tab, cnt, s);
		const double dz0 = out.ms_deflate + out.ms_copy;
		out.emit(out.placed_end(n), s, h->device, [&](const Win& w, int64_t ws) {
			if (!n) return;
			ck_gather.mark();
			if (m.single_end) hipLaunchKernelGGL(rm_single_gather_kernel, dim3(grid_for(n, 4)), dim3(256), 0, s, sz.p, off.p, n, j.src.p, j.info.p, ws, w, T, m);
			else hipLaunchKernelGGL(rm_pair_gather_kernel, dim3(grid_for(n, 4)), dim3(256), 0, s, j.close_of.p, sz.p, off.p, n, H, j.src.p, j.info.p, ws, w, T, m);
			KCHECK();
			ck_gather.mark();
		});
		HIPCHK(hipStreamSynchronize(s));   // (the old pool and the tile's bytes are no longer read)
		if (!m.single_end) j.end_tile();
		ms_tiles += wall_ms() - t0 - (out.ms_deflate + out.ms_copy - dz0);
		return true;
	});
	unsigned long long jc[4] = {0, 0, 0, 0}, dc[C_N];
	j.read_counts(jc, s);
	HIPCHK(hipMemcpyAsync(dc, counts.p, sizeof(dc), hipMemcpyDeviceToHost, s)); HIPCHK(hipStreamSynchronize(s));
	out.close(s, h->device, out_path);
	cnt->passed = (int64_t)(m.single_end ? dc[C_SE_PASSED] : jc[0]); cnt->dropped = (int64_t)(m.single_end ? dc[C_SE_DROPPED] : jc[1]);
	cnt->modified = (int64_t)dc[C_MODIFIED] - (int64_t)dc[C_MOD_MINUS]; cnt->skipped = (int64_t)dc[C_SKIPPED];
	if (timing)
		fprintf(stderr, "[ngsqc] remove_variants: %.1f ms in all: variant table %.1f ms (%lld lines), verdicts, join and gather %.1f ms on the host's clock (by HIP events: verdict kernels %.1f ms, gather and patch "
		                "kernel %.1f ms, which the host's clock books with the deflate stage that waits for it; K1 %.1f ms and K2 %.1f ms of the input), deflate %.1f ms, copy to pinned memory %.1f ms, "
		                "file writes %.1f ms (host thread), %lld open names at the end, windows of %lld bytes\n",
		        wall_ms() - t_w, ms_table, (long long)n_var, ms_tiles, ck_verdict.total(), ck_gather.total(), h->tm.inflate_ms, h->tm.index_ms, out.ms_deflate, out.ms_copy, out.sink.write_ms,
		        (long long)j.H, (long long)W);
}

void variant_verdicts(ngsqc_handle* h, const ngsqc_rm_variant* variants, int64_t n_var, const ngsqc_rm_params* p, uint8_t* out, int64_t cap)
{
	if (!p || n_var < 0 || (n_var && !variants) || cap < 0 || (cap && !out)) throw ArgError("null argument");
	require_whole_file(h, "BamRemoveVariants");
	const RmMode m{p->mask ? 1 : 0, p->single_end ? 1 : 0, p->keep_indels ? 1 : 0};
	hipStream_t s = h->stream;
	RmDevTable tab; tab.build(h, variants, n_var, s);
	const RmTable T = tab.table();
	VerdictBufs vb;
	const int64_t done = for_each_tile_bytes(h, out, cap, "the verdict buffer is smaller than the number of records", [&](const TileCtx& c, const int64_t* rec, int64_t n) {
		vb.run(c.infl, rec, n, 0, T, m, 0, VerdictOut{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}, s);
		return vb.vd.p;
	});
	for (int64_t i = 0; i < done; ++i) out[i] &= 15;   // (the device's byte also holds the error code)
}
} // namespace lib
} // namespace ngsqc

int ngsqc_remove_variants(ngsqc_handle* h, const ngsqc_rm_variant* variants, int64_t n, const ngsqc_rm_params* p, const char* out_bam_path, ngsqc_rm_counts* counts)
{
	if (!h || !p || !out_bam_path || !counts || n < 0 || (n && !variants)) return NGSQC_E_ARG;   // (before a device is touched)
	return guarded(h, [&] { ngsqc::lib::remove_variants(h, variants, n, p, out_bam_path, counts); });
}

int ngsqc_variant_verdicts(ngsqc_handle* h, const ngsqc_rm_variant* variants, int64_t n, const ngsqc_rm_params* p, uint8_t* out, int64_t cap)
{
	if (!h || !p || n < 0 || (n && !variants) || cap < 0 || (cap && !out)) return NGSQC_E_ARG;
	return guarded(h, [&] { ngsqc::lib::variant_verdicts(h, variants, n, p, out, cap); });
}
