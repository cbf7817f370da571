// BamClipOverlap's visit of a closed read pair (src/BamClipOverlap/main.cpp:94-535, NGSHelper::softClipAlignment NGSHelper.cpp:670-810), free of HIP: the text
// the plan and gather kernels of clip.hip compile, and tests/emul/clip_emul.cpp compiles for the CPU against the literal restatement
// (tests/bamclipoverlap_oracle.py). Nothing here is sized by the read length:
//   - the overlap comparison (the reference's two lists with '+' placeholders, :270-408) is a merge of two cursors over the expanded CIGARs (merge_overlaps):
//     where the operations differ and exactly one side is I, that side alone advances and is a mismatch against '+';
//   - the soft-clip rewrite (the per-base matrix, the dropped clipped D, the D / I clean-up around S and the start shift, NGSHelper.cpp:691-807) is one pass
//     over the operations: every operation gives at most three segments (first type, marked type, length) that go through the run-length stage, the clean-up
//     stage (which only ever looks at the previous operation, so one pending operation is the whole state) and the start-shift counter;
//   - the positions of the mismatches are not stored: the gather runs the visit again with a functor that patches its copy.
// A record is seen with the CIGAR of its CG tag in place (rec_apply_cg), as htslib hands it to the reference. A pair that is clipped and holds such a record, or
// whose new CIGAR would need more than 65535 operations (bam_write1 would move it into a CG tag), is E_UNSUPPORTED.
// A CIGAR that walks behind the end of the sequence reads behind the arrays in the reference; here such an index gives a base of its own (no nibble), equal only
// to itself, and is never patched.
#pragma once
#include "rec.h"

namespace ngsqc {
namespace clip {

enum { MODE_MAPQ = 1, MODE_REMOVE = 2, MODE_BASEQ = 4, MODE_BASEN = 8 };   // precedence among them: mapq > remove > baseq > basen (:421-471)
enum { ROLE_PASS = 0, ROLE_FORWARD = 1, ROLE_REVERSE = 2, ROLE_LEFTOVER = 3 };
enum { V_CLIP_PAIR = 1, V_MISMATCH = 2, V_REMOVED = 4, V_MAPQ0 = 8, V_QUAL = 16, V_BASES = 32, V_REWRITTEN = 64 };
enum { E_NONE = 0, E_ORIENT, E_CIGAR_CHAR, E_LENGTH, E_SC_ORDER, E_SC_START, E_SC_END, E_SC_INDEX, E_SC_OP, E_BAD_BASE, E_UNSUPPORTED };
enum { OP_M = 0, OP_I = 1, OP_D = 2, OP_S = 4, OP_H = 5 };
enum { BASE_DEL = 16, BASE_NONE = 18 };   // what an overlap entry holds besides a nibble: '-' and "behind the sequence"

__device__ __forceinline__ int op_char(uint32_t op) { return "MIDNSHP=XB??????"[op & 15]; }
__device__ __forceinline__ bool op_known(uint32_t op) { return op == OP_M || op == OP_I || op == OP_D || op == OP_S || op == OP_H; }
__device__ __forceinline__ int32_t mate_tid(const RecView& r) { return (int32_t)ld32(r.core + 20); }
__device__ __forceinline__ int seq_nib(const RecView& r, int i) { const uint8_t b = r.core[32 + r.l_name + 4ull * r.n_cigar_raw + ((uint32_t)i >> 1)]; return (i & 1) ? (b & 15) : (b >> 4); }

// bam_endpos: pos + the reference length of the CIGAR (M, D, N, =, X), at least 1
__device__ inline int ref_len(const RecView& r)
{
	int n = 0;
	for (uint32_t k = 0; k < r.n_cigar; ++k) { const uint32_t c = ld32(r.cigar + 4ull * k); if ((0x3C1A7u >> ((c & 15u) << 1)) & 2u) n += (int)(c >> 4); }
	return n;
}
__device__ inline int end_of(const RecView& r) { const int n = (r.flag & 4) ? 0 : ref_len(r); return r.pos + (n ? n : 1); }

// the preconditions (:69-92) on the record with its effective CIGAR: false = the record is written through as it is
__device__ inline bool joins(const RecView& r)
{
	if (!(r.flag & 1) || (r.flag & 0x900) || (r.flag & 4) || (r.flag & 8) || r.tid != mate_tid(r)) return false;
	for (uint32_t k = 0; k < r.n_cigar; ++k) { const uint32_t op = ld32(r.cigar + 4ull * k) & 15u; if (op != OP_I && op != OP_S) return true; }
	return false;   // cigarIsOnlyInsertion (an empty CIGAR included)
}

// cigarDataAsString(): the length of the text and its characters, one by one
__device__ inline int cigar_text_len(const RecView& r)
{
	int n = 0;
	for (uint32_t k = 0; k < r.n_cigar; ++k) { uint32_t len = ld32(r.cigar + 4ull * k) >> 4; do { ++n; len /= 10; } while (len); ++n; }
	return n;
}
template <typename Put> __device__ inline void cigar_text_put(const RecView& r, Put put)
{
	for (uint32_t k = 0; k < r.n_cigar; ++k)
	{
		const uint32_t c = ld32(r.cigar + 4ull * k); uint32_t len = c >> 4, div = 1;
		while (len / div >= 10) div *= 10;
		for (; div; div /= 10) put((uint8_t)('0' + len / div % 10));
		put((uint8_t)op_char(c));
	}
}

// ---- the geometry (:98-203) ----
struct Geo { bool soft_clip, fwd_is_opener, both; int s1, e1, s2, e2, clip_f, clip_r, overlap, ov_start, ov_end, err; };

__device__ inline Geo geometry(const RecView& opener, const RecView& closer)
{
	Geo g{};
	const bool rev_o = opener.flag & 16, rev_c = closer.flag & 16;
	g.fwd_is_opener = true; g.both = rev_o != rev_c;
	if (g.both && !rev_c) g.fwd_is_opener = false;
	const RecView& f = g.fwd_is_opener ? opener : closer; const RecView& r = g.fwd_is_opener ? closer : opener;
	const int s1 = g.s1 = f.pos + 1, e1 = g.e1 = end_of(f), s2 = g.s2 = r.pos + 1, e2 = g.e2 = end_of(r);
	if (f.tid == r.tid) g.soft_clip = (s1 >= s2 && s1 <= e2) || (e1 >= s2 && e1 <= e2) || (s1 <= s2 && e1 >= e2);
	if (!g.soft_clip) return g;
	const bool read1 = f.flag & 64;
	int ov, half;
	if (s1 <= s2 && e1 <= e2) { ov = e1 - s2 + 1; half = ov / 2; g.ov_start = s2 - 1; g.ov_end = e1; g.clip_f = half; g.clip_r = half; (read1 ? g.clip_f : g.clip_r) += ov % 2; }
	else if (s1 > s2 && e1 > e2) { ov = e2 - s1 + 1; half = ov / 2; g.ov_start = s1 - 1; g.ov_end = e2; g.clip_f = half + (e1 - e2); g.clip_r = half + (s1 - s2); (read1 ? g.clip_f : g.clip_r) += ov % 2; }
	else if (g.both && s1 >= s2 && e1 <= e2) { ov = e1 - s1 + 1; half = ov / 2; g.ov_start = s1 - 1; g.ov_end = e1; g.clip_f = half; g.clip_r = half + (s1 - s2); (read1 ? g.clip_f : g.clip_r) += ov % 2; }
	else if (g.both && s1 <= s2 && e1 >= e2) { ov = e2 - s2 + 1; half = ov / 2; g.ov_start = s2 - 1; g.ov_end = e2; g.clip_f = half + (e1 - e2); g.clip_r = half; (read1 ? g.clip_f : g.clip_r) += ov % 2; }
	else if (!g.both && s1 >= s2 && e1 <= e2) { ov = e1 - s1 + 1; g.ov_start = s1 - 1; g.ov_end = e1; g.clip_f = ov; g.clip_r = 0; }
	else if (!g.both && s1 <= s2 && e1 >= e2) { ov = e2 - s2 + 1; g.ov_start = s2 - 1; g.ov_end = e2; g.clip_f = 0; g.clip_r = ov; }
	else { ov = 0; g.err = E_ORIENT; }   // (cannot be reached: end >= start on both reads)
	g.overlap = ov;
	return g;
}

// ---- the walk of one read (:278-322): unknown characters and an indel near the clip position, operation by operation ----
__device__ inline int walk_check(const RecView& r, int clip_position, bool ignore_indels, bool& has_indel, int& bad_char)
{
	int g = r.pos;
	for (uint32_t k = 0; k < r.n_cigar; ++k)
	{
		const uint32_t c = ld32(r.cigar + 4ull * k), op = c & 15u; const int len = (int)(c >> 4);
		if (!len) continue;
		if (!op_known(op)) { bad_char = op_char(op); return E_CIGAR_CHAR; }
		if (!ignore_indels)
		{
			if (op == OP_I && g > clip_position - 5 && g < clip_position + 5) has_indel = true;
			if (op == OP_D && g < clip_position + 5 && g + len - 1 > clip_position - 5) has_indel = true;
		}
		if (op == OP_M || op == OP_D) g += len;
	}
	return E_NONE;
}

// ---- the overlap entries of one read, in order: a cursor over the expanded CIGAR ----
struct OvEntry { int op, rp, base; };
struct OvCursor
{
	const RecView* r; uint32_t k; int left, op, g, rp, lo, hi;
	__device__ OvCursor(const RecView& rec, int lo_, int hi_) : r(&rec), k(0), left(0), op(0), g(rec.pos), rp(0), lo(lo_), hi(hi_) {}
	__device__ bool next(OvEntry& e)
	{
		for (;;)
		{
			if (g >= hi) return false;   // (genome_pos never falls)
			if (!left)
			{
				if (k == r->n_cigar) return false;
				const uint32_t c = ld32(r->cigar + 4ull * k); ++k;
				op = (int)(c & 15u); left = (int)(c >> 4);
				continue;
			}
			if (op == OP_H) { left = 0; continue; }
			if (op == OP_S) { rp += left; left = 0; continue; }
			if (g < lo)   // in front of the overlap: whole stretches at once
			{
				if (op == OP_I) { rp += left; left = 0; continue; }
				const int skip = left < lo - g ? left : lo - g;
				g += skip; if (op == OP_M) rp += skip; left -= skip;
				continue;
			}
			e.op = op; e.rp = rp;
			e.base = op == OP_D ? (int)BASE_DEL : (rp >= 0 && rp < r->l_seq ? seq_nib(*r, rp) : (int)BASE_NONE);
			if (op == OP_M) { ++g; ++rp; } else if (op == OP_D) ++g; else ++rp;
			--left;
			return true;
		}
	}
	__device__ int rest() { OvEntry e; int n = 0; while (next(e)) ++n; return n; }
};

// The insertion correction and the mismatch detection (:374-408) as a merge. on_mm(first, second): the read positions of a mismatch, -1 where that side holds
// '-' or '+'. E_LENGTH with the two lengths as the reference would print them; the reverse list ending first is undefined there and reported the same way.
template <typename MM> __device__ inline int merge_overlaps(const RecView& f, const RecView& r, int lo, int hi, MM on_mm, int& len_f, int& len_r)
{
	OvCursor a(f, lo, hi), b(r, lo, hi);
	OvEntry x, y;
	bool ha = a.next(x), hb = b.next(y);
	int i = 0;
	while (ha)
	{
		if (!hb) { len_f = i + 1 + a.rest(); len_r = i; return E_LENGTH; }
		if (x.op != y.op && x.op == OP_I) { on_mm(x.rp, -1); ha = a.next(x); }
		else if (x.op != y.op && y.op == OP_I) { on_mm(-1, y.rp); hb = b.next(y); }
		else
		{
			if (x.base != y.base) on_mm(x.base == BASE_DEL ? -1 : x.rp, y.base == BASE_DEL ? -1 : y.rp);
			ha = a.next(x); hb = b.next(y);
		}
		++i;
	}
	len_f = i; len_r = i;
	if (hb) { len_r = i + 1 + b.rest(); return E_LENGTH; }
	return E_NONE;
}

// ---- softClipAlignment as one pass over the operations ----
// emit(k, word): the k-th operation of the new CIGAR as bam_cigar_gen makes it (a read whose every base was a clipped D gives the one word 0xffffffff)
template <typename Emit> struct SoftClipper
{
	Emit emit; int n_out = 0, rlen = 0, offset = 0;
	int tmp_char = -1, tmp_count = 0;      // the run-length stage
	bool have_prev = false; int pt = 0, pn = 0;   // the clean-up stage: the operation at i - 1
	int phase = 0;                          // the start shift: 0 leading H, 1 the clipped run, 2 done
	__device__ explicit SoftClipper(Emit e) : emit(e) {}
	__device__ void out(int t, int n) { emit(n_out, ((uint32_t)n << 4) | (uint32_t)t); ++n_out; if (t == OP_M || t == OP_D) rlen += n; }
	__device__ void clean(int t, int n)
	{
		if (!have_prev) { have_prev = true; pt = t; pn = n; return; }
		if (pt == OP_S && t == OP_D) return;
		if (pt == OP_D && t == OP_S) { pt = t; pn = n; return; }
		if (pt == OP_S && t == OP_I) { pn += n; return; }
		if (pt == OP_I && t == OP_S) { pt = t; pn += n; return; }
		out(pt, pn); pt = t; pn = n;
	}
	__device__ void seg(int first, int second, int len)
	{
		if (len <= 0) return;
		if (phase == 0 && second != OP_H) phase = second == OP_S ? 1 : 2;
		if (phase == 1) { if (second == OP_S) { if (first == OP_M || first == OP_D) offset += len; } else phase = 2; }
		if (first == OP_D && second == OP_S) return;
		if (second != tmp_char) { if (tmp_char != -1) clean(tmp_char, tmp_count); tmp_char = second; tmp_count = 0; }
		tmp_count += len;
	}
	__device__ void finish() { clean(tmp_char, tmp_count); out(pt, pn); }
};

template <typename Emit> __device__ inline int soft_clip(const RecView& r, int start_ref, int end_ref, Emit emit, int& new_pos, int& n_out, int& new_rlen, int& ea)
{
	const int al_start = r.pos + 1, al_end = end_of(r);
	if (start_ref > end_ref) return E_SC_ORDER;
	if (start_ref < al_start || start_ref > al_end) { ea = start_ref; return E_SC_START; }
	if (end_ref < al_start || end_ref > al_end) { ea = end_ref; return E_SC_END; }
	int total = 0;
	for (uint32_t k = 0; k < r.n_cigar; ++k)
	{
		const uint32_t c = ld32(r.cigar + 4ull * k), op = c & 15u;
		if (!op_known(op)) { ea = op_char(op); return E_SC_OP; }
		if (op == OP_M || op == OP_D) total += (int)(c >> 4);
	}
	if (!total) return E_SC_INDEX;   // (the matrix walk waits for a reference base that never comes)
	SoftClipper<Emit> sc(emit);
	int cur = al_start;
	for (uint32_t k = 0; k < r.n_cigar; ++k)
	{
		const uint32_t c = ld32(r.cigar + 4ull * k); const int op = (int)(c & 15u), len = (int)(c >> 4);
		if (op == OP_H || cur > al_end) sc.seg(op, op, len);   // (behind the last reference base the walk has ended)
		else if (op == OP_I || op == OP_S) sc.seg(op, cur >= start_ref && cur <= end_ref ? (int)OP_S : op, len);
		else
		{
			int a = start_ref - cur; a = a < 0 ? 0 : (a > len ? len : a);
			int e = end_ref - cur + 1; e = e < a ? a : (e > len ? len : e);
			sc.seg(op, op, a); sc.seg(op, OP_S, e - a); sc.seg(op, op, len - e);
			cur += len;
		}
	}
	sc.finish();
	new_pos = r.pos + sc.offset; n_out = sc.n_out; new_rlen = sc.rlen;
	return sc.n_out > 65535 ? (int)E_UNSUPPORTED : (int)E_NONE;
}

// ---- the pair ----
struct MateOut { int clip, pos, n_cigar, tlen, mpos, bits; };
struct PairOut { bool soft_clip, fwd_is_opener, mismatch; int overlap, err, ea, eb; MateOut f, r; };
struct NoEmit { __device__ void operator()(int, uint32_t) const {} };
struct NoMM { __device__ void operator()(int, int) const {} };

__device__ inline bool storable(int nib) { return nib == 1 || nib == 2 || nib == 4 || nib == 8 || nib == 15; }

// setBases (BamReader.cpp:133-181) stores A, C, G, T, N alone: the first base of the read that is neither storable nor replaced by N
__device__ inline int first_unstorable(const RecView& f, const RecView& r, const Geo& g, bool forward_side)
{
	const RecView& x = forward_side ? f : r;
	for (int p = 0; p < x.l_seq; ++p)
	{
		const int nib = seq_nib(x, p);
		if (storable(nib)) continue;
		bool patched = false; int lf, lr;
		merge_overlaps(f, r, g.ov_start, g.ov_end, [&](int a, int b) { if ((forward_side ? a : b) == p) patched = true; }, lf, lr);
		if (!patched) return "=ACMGRSVTWYHKDBN"[nib];
	}
	return 0;
}

// opener / closer: the two records of a name in file order, CG applied; either_cg: one of them takes its CIGAR from a CG tag. parity: the number of earlier
// pairs with soft_clip, mod 2 (reads_clipped % 4 == 0 exactly when it is even). emit_f / emit_r: the new CIGAR of a clipped mate; on_mm: the mismatches, when
// the pair has no error (called before the clip).
template <typename EF, typename ER, typename MM>
__device__ inline void visit_pair(const RecView& opener, const RecView& closer, bool either_cg, int mode, bool ignore_indels, int parity, PairOut& o, EF emit_f, ER emit_r, MM on_mm)
{
	const Geo g = geometry(opener, closer);
	const RecView& f = g.fwd_is_opener ? opener : closer; const RecView& r = g.fwd_is_opener ? closer : opener;
	o.soft_clip = g.soft_clip; o.fwd_is_opener = g.fwd_is_opener; o.mismatch = false; o.overlap = g.overlap; o.err = E_NONE; o.ea = o.eb = 0;
	o.f = MateOut{0, f.pos, (int)f.n_cigar, f.isize, (int)ld32(f.core + 24), 0};
	o.r = MateOut{0, r.pos, (int)r.n_cigar, r.isize, (int)ld32(r.core + 24), 0};
	if (!g.soft_clip) return;
	if (either_cg) { o.err = E_UNSUPPORTED; return; }
	if (g.err) { o.err = g.err; return; }
	bool has_indel = false;
	if ((o.err = walk_check(f, g.e1 - g.clip_f, ignore_indels, has_indel, o.ea)) != E_NONE) return;
	if ((o.err = walk_check(r, g.s2 - 1 + g.clip_r, ignore_indels, has_indel, o.ea)) != E_NONE) return;
	bool mm = false;
	if ((o.err = merge_overlaps(f, r, g.ov_start, g.ov_end, [&](int, int) { mm = true; }, o.ea, o.eb)) != E_NONE) return;
	o.ea = o.eb = 0;
	int bits = V_CLIP_PAIR;
	if (mm && (mode & (MODE_MAPQ | MODE_REMOVE | MODE_BASEQ | MODE_BASEN)))
	{
		o.mismatch = true;
		bits |= V_MISMATCH | ((mode & MODE_MAPQ) ? V_MAPQ0 : (mode & MODE_REMOVE) ? V_REMOVED : (mode & MODE_BASEQ) ? V_QUAL : V_BASES);
		if (bits & V_BASES)
		{
			int ch = first_unstorable(f, r, g, true);
			if (!ch) ch = first_unstorable(f, r, g, false);
			if (ch) { o.err = E_BAD_BASE; o.ea = ch; return; }
		}
		if (bits & (V_QUAL | V_BASES)) { int lf, lr; merge_overlaps(f, r, g.ov_start, g.ov_end, on_mm, lf, lr); }
	}
	int clip_f = g.clip_f, clip_r = g.clip_r;
	if (has_indel) { if (parity == 0) { clip_f = 0; clip_r = g.overlap; } else { clip_f = g.overlap; clip_r = 0; } }
	int f_pos = f.pos, f_n = (int)f.n_cigar, f_rlen = ref_len(f), r_pos = r.pos, r_n = (int)r.n_cigar, r_rlen = ref_len(r);
	if (clip_f > 0 && (o.err = soft_clip(f, g.e1 - clip_f + 1, g.e1, emit_f, f_pos, f_n, f_rlen, o.ea)) != E_NONE) return;
	if (clip_r > 0 && (o.err = soft_clip(r, g.s2, g.s2 - 1 + clip_r, emit_r, r_pos, r_n, r_rlen, o.ea)) != E_NONE) return;
	// the insert size and the mate start of the clipped reads (:497-518)
	const int f_start = f_pos + 1, r_start = r_pos + 1;
	int r_end = r_pos + (r_rlen ? r_rlen : 1);   // (the forward read's end only shows in the reference's log)
	if (r_start == r_end) r_end -= 1;
	o.f = MateOut{clip_f, f_pos, f_n, r_end - f_start + 1, r_start - 1, bits | (clip_f > 0 ? (int)V_REWRITTEN : 0)};
	o.r = MateOut{clip_r, r_pos, r_n, f_start - r_end - 1, f_start - 1, bits | (clip_r > 0 ? (int)V_REWRITTEN : 0)};
}

// ---- the bytes of the two records of a soft-clipped pair ----
// A record of such a pair is the input's bytes with pos, mapq, next_pos and tlen patched and, under -overlap_mismatch_baseq / _basen, the mismatching
// qualities set to 0 / bases to N. A mate that was clipped (V_REWRITTEN) also has block_size and n_cigar_op patched, the new CIGAR in place of the old one
// (everything behind it moves by 4 * (new - old operations)) and "BS" 'Z' <old CIGAR text> NUL behind its last tag. The bin field keeps the input's bytes.
// Sink: sink(at, byte) stores one byte at a position of the output stream (and drops what lies outside its window); sink.fence() orders the copy before the
// patches laid over it. lane / n_lanes: the copies are strided over the lanes of a wave, everything serial is lane 0's.
__device__ inline uint32_t written_size(const RecView& raw, const MateOut& m, int text_len)
{
	return (m.bits & V_REWRITTEN) ? raw.bs + 4u + 4u * (uint32_t)(m.n_cigar - (int)raw.n_cigar_raw) + 4u + (uint32_t)text_len : raw.bs + 4u;
}

template <typename Sink> struct CigarSink
{
	Sink sink; long long at; bool on;
	__device__ void operator()(int k, uint32_t w) { if (on) for (int i = 0; i < 4; ++i) sink(at + 4ll * k + i, (uint8_t)(w >> (8 * i))); }
};

struct PatchSide { const RecView* rec; long long seq_out, qual_out; int pend_idx, pend_val; };
template <typename Sink> struct PatchState
{
	Sink sink; bool bases, on; PatchSide s[2];
	__device__ void flush(PatchSide& x) { if (x.pend_idx >= 0 && on) sink(x.seq_out + x.pend_idx, (uint8_t)x.pend_val); x.pend_idx = -1; }
	// (the positions of one side never fall: a byte that takes two N is finished before the next one begins, and is built from the source alone)
	__device__ void one(PatchSide& x, int p)
	{
		if (p < 0 || p >= x.rec->l_seq) return;
		if (!bases) { if (on) sink(x.qual_out + p, 0); return; }
		if ((p >> 1) != x.pend_idx) { flush(x); x.pend_idx = p >> 1; x.pend_val = x.rec->core[32 + x.rec->l_name + 4ull * x.rec->n_cigar_raw + (uint32_t)(p >> 1)]; }
		x.pend_val = (p & 1) ? (x.pend_val | 0x0f) : (x.pend_val | 0xf0);
	}
};
template <typename Sink> struct PatchMM
{
	PatchState<Sink>* st;
	__device__ void operator()(int a, int b) const { st->one(st->s[0], a); st->one(st->s[1], b); }
};

template <typename Sink> __device__ inline void write_mate(const uint8_t* s, const RecView& raw, const MateOut& m, int text_len, long long pos, Sink sink, int lane, int n_lanes)
{
	const bool rew = m.bits & V_REWRITTEN;
	const uint32_t n_old = raw.n_cigar_raw, nc = rew ? (uint32_t)m.n_cigar : n_old, size = written_size(raw, m, text_len);
	if (lane == 0)
	{
		uint8_t fixed[36];
		for (int i = 0; i < 36; ++i) fixed[i] = s[i];
		auto put32 = [&](int at, uint32_t v) { for (int i = 0; i < 4; ++i) fixed[at + i] = (uint8_t)(v >> (8 * i)); };
		put32(0, size - 4); put32(8, (uint32_t)m.pos); put32(28, (uint32_t)m.mpos); put32(32, (uint32_t)m.tlen);
		if (m.bits & V_MAPQ0) fixed[13] = 0;
		fixed[16] = (uint8_t)nc; fixed[17] = (uint8_t)(nc >> 8);
		for (int i = 0; i < 36; ++i) sink(pos + i, fixed[i]);
	}
	const long long head = 36ll + raw.l_name + (rew ? 0 : 4ll * n_old);   // the name, and the CIGAR of a mate that keeps it
	for (long long i = 36 + lane; i < head; i += n_lanes) sink(pos + i, s[i]);
	const long long src = 36ll + raw.l_name + 4ll * n_old, dst = 36ll + raw.l_name + 4ll * nc, rest = (long long)raw.bs + 4 - src;
	for (long long i = lane; i < rest; i += n_lanes) sink(pos + dst + i, s[src + i]);
	if (rew && lane == 0)
	{
		long long at = pos + dst + rest;
		sink(at++, 'B'); sink(at++, 'S'); sink(at++, 'Z');
		cigar_text_put(raw, [&](uint8_t c) { sink(at++, c); });
		sink(at, 0);
	}
}

// The pair that `closer` closes, at stream position pos: forward read, then reverse read. False (and nothing written) when the pair is not soft-clipped: its
// two records leave as they are, in the same order, by the caller's own copy. The pair has no error and is not removed (the plan has settled both).
template <typename Sink> __device__ inline bool write_pair(const uint8_t* opener, const uint8_t* closer, int mode, bool ignore_indels, int parity, long long pos, Sink sink, int lane, int n_lanes,
                                                           PairOut& o, uint32_t& size_f, uint32_t& size_r)
{
	const RecView ro = load_rec(opener, 0), rc = load_rec(closer, 0);
	RecView eo = ro, ec = rc; rec_apply_cg(eo); rec_apply_cg(ec);
	const bool cg = eo.cigar != ro.cigar || ec.cigar != rc.cigar;
	visit_pair(eo, ec, cg, mode, ignore_indels, parity, o, NoEmit{}, NoEmit{}, NoMM{});
	size_f = size_r = 0;
	if (!o.soft_clip || o.err) return false;
	const uint8_t* sf = o.fwd_is_opener ? opener : closer; const uint8_t* sr = o.fwd_is_opener ? closer : opener;
	const RecView& f = o.fwd_is_opener ? ro : rc; const RecView& r = o.fwd_is_opener ? rc : ro;
	const int tf = cigar_text_len(f), tr = cigar_text_len(r);
	size_f = written_size(f, o.f, tf); size_r = written_size(r, o.r, tr);
	if (o.f.bits & V_REMOVED) { size_f = size_r = 0; return true; }
	const long long pos_r = pos + size_f;
	write_mate(sf, f, o.f, tf, pos, sink, lane, n_lanes);
	write_mate(sr, r, o.r, tr, pos_r, sink, lane, n_lanes);
	const bool rew_f = o.f.bits & V_REWRITTEN, rew_r = o.r.bits & V_REWRITTEN, patch = o.f.bits & (V_QUAL | V_BASES);
	if (!rew_f && !rew_r && !patch) return true;
	sink.fence();
	const bool l0 = lane == 0;
	const long long seq_f = pos + 36 + f.l_name + 4ll * (rew_f ? (uint32_t)o.f.n_cigar : f.n_cigar_raw), seq_r = pos_r + 36 + r.l_name + 4ll * (rew_r ? (uint32_t)o.r.n_cigar : r.n_cigar_raw);
	PatchState<Sink> st{sink, (o.f.bits & V_BASES) != 0, l0, {{&f, seq_f, seq_f + ((uint32_t)f.l_seq + 1) / 2, -1, 0}, {&r, seq_r, seq_r + ((uint32_t)r.l_seq + 1) / 2, -1, 0}}};
	PairOut again;
	visit_pair(eo, ec, false, mode, ignore_indels, parity, again,   // (the second time: the new CIGARs and the patches go into the copies)
	           CigarSink<Sink>{sink, pos + 36 + f.l_name, l0 && rew_f}, CigarSink<Sink>{sink, pos_r + 36 + r.l_name, l0 && rew_r}, PatchMM<Sink>{&st});
	st.flush(st.s[0]); st.flush(st.s[1]);
	return true;
}

} // namespace clip
} // namespace ngsqc
