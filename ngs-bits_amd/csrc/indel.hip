// Indel windows: BamReader::getIndels (src/cppNGS/BamReader.cpp:948-1125) for a table of windows, the indel half of BamReader::getVariantDetails (:888-946).
//
// The reference runs one indexed query per variant over the window [start, end] that Variant::indelRegion widens by one base on each side. Here every record
// looks up the windows its reference span overlaps (per-reference 64 kb buckets, then a binary search: a window table of a whole VCF is dense where the site
// table of the pileup is sparse) and walks its CIGAR once for all of them. Per window, counts[8 * i + k]:
//   0 reads_mapped   records that overlap the window (htslib region semantics: pos < end && bam_endpos > start - 1) and pass the filters of :970-981
//   1 reads_mapq0    ... of which MAPQ 0 (not counted further)
//   2 depth          records with start <= window.start and end >= window.end, minus one for each N operation that spans the window (:1068-1075); kept
//                    modulo 2^32 (a decrement is + 0xFFFFFFFF): the host reads it as int32
//   3 n_ins, 4 n_del I / D operations of spanning records whose genome position lies in [start, end] (:1046-1066), one per operation
//   5 n_match        ... equal to the window's query allele: "+SEQ" (the read's bases, mid() semantics) / "-REF" (the reference slice at the operation, cut at
//                    the contig's end - the length the BAM header gives - as FastaFileIndex::seq cuts it)
//   6 unknown        spanning records with an I / D / N operation that also hold an operation the reference throws on ("Unknown CIGAR operation")
// Records with more than LONG_CIGAR operations go to a wave-per-record kernel, as in the site pileup.
#include "common.h"
#include "rec.h"

namespace ngsqc {

// first window of reference tid [first, last) whose start is >= x
__device__ __forceinline__ int win_lower(const IndelTables& w, int tid, int first, int last, long long x)
{
	return postable_lower_bsearch(w.tab, tid, first, last, x);
}

__device__ __forceinline__ char seq_char(const RecView& r, int i)
{
	const uint8_t* seq = r.core + 32 + r.l_name + 4ull * r.n_cigar_raw;
	return "=ACMGRSVTWYHKDBN"[(seq[i >> 1] >> ((~i & 1) << 2)) & 15];
}

// an I (op 1) or D (op 2) operation of length len at 1-based genome position gp, read position rp, against window i
__device__ __forceinline__ void indel_event(const IndelTables& w, const RecView& r, int i, uint32_t op, int len, long long gp, int rp, uint32_t* counts)
{
	const IndelWin& q = w.win[i];
	bool match = false;
	if (op == 1u)
	{
		// al.bases().mid(read_pos, len): what SEQ holds of the inserted bases
		const int avail = max(0, min(len, r.l_seq - rp));
		if (q.kind == NGSQC_ALLELE_INS && avail == q.len)
		{
			match = true;
			for (int j = 0; j < avail && match; ++j) match = seq_char(r, rp + j) == (char)w.pool[q.qoff + j];
		}
	}
	else if (q.kind == NGSQC_ALLELE_DEL)
	{
		// "-" + reference.seq(chr, genome_pos, len): FastaFileIndex::seq ends at the contig's end (FastaFileIndex.cpp:89-94), so a deletion running past it is
		// compared by the bases that are left. The slice holds [start, end + q.len) of the window, 0 behind the contig end: gp <= end keeps s + q.len inside it
		const long long left = (long long)q.ref_len - gp + 1;
		const int have = (int)max(0ll, min((long long)len, left));
		if (have == q.len)
		{
			const int64_t s = q.soff + (gp - w.tab.pos[i]);
			match = true;
			for (int j = 0; j < have && match; ++j) match = w.pool[s + j] == w.pool[q.qoff + j];
		}
	}
	atomicAdd(&counts[8ull * i + (op == 1u ? 3 : 4)], 1u);
	if (match) atomicAdd(&counts[8ull * i + 5], 1u);
}

__device__ __forceinline__ bool read_filtered(const RecView& r, int include_npp)
{
	if (r.flag & (0x400 | 0x100 | 0x800 | 0x4)) return true;   // duplicate, secondary, supplementary, unmapped (BamReader.cpp:970-981)
	return !(r.flag & 0x2) && !include_npp;                     // proper pair unless include_not_properly_paired
}

__global__ __launch_bounds__(256) void indel_kernel(const uint8_t* __restrict__ infl, const int64_t* __restrict__ recoff, long long n_rec, const IndelTables w,
                                                    uint32_t* __restrict__ counts, int64_t* __restrict__ long_list, unsigned long long* __restrict__ long_count)
{
	for (long long li = (long long)blockIdx.x * blockDim.x + threadIdx.x; li < n_rec; li += (long long)gridDim.x * blockDim.x)
	{
		RecView r = load_rec(infl, recoff[li]);
		if (read_filtered(r, w.include_npp)) continue;
		if (r.tid < 0 || r.tid >= w.n_ref) continue;
		const int first = w.tab.tid_first[r.tid], last = w.tab.tid_last[r.tid];
		if (first >= last) continue;
		rec_apply_cg(r);
		if (r.n_cigar > (uint32_t)LONG_CIGAR) { long_list[atomicAdd(long_count, 1ull)] = li; continue; }   // wave-per-record path (indel_long_kernel)
		long long ref_len = 0; bool idn = false, unknown = false;
		for (uint32_t k = 0; k < r.n_cigar; ++k)
		{
			const uint32_t c = ld32(r.cigar + 4ull * k), op = c & 15u;
			if ((0x18Du >> op) & 1u) ref_len += c >> 4;
			idn |= op == 1u || op == 2u || op == 3u; unknown |= op == 6u || op > 8u;
		}
		if (ref_len == 0) ref_len = 1;                                        // bam_endpos
		const long long start1 = (long long)r.pos + 1, end1 = (long long)r.pos + ref_len;
		const int a = win_lower(w, r.tid, first, last, start1 - w.tid_maxlen[r.tid] + 1);
		const bool mq0 = r.mapq == 0;
		bool any_span = false;
		for (int i = a; i < last && w.tab.pos[i] <= end1; ++i)
		{
			if (w.win[i].end < start1) continue;
			atomicAdd(&counts[8ull * i], 1u);
			if (mq0) { atomicAdd(&counts[8ull * i + 1], 1u); continue; }
			if (start1 <= w.tab.pos[i] && end1 >= w.win[i].end) { atomicAdd(&counts[8ull * i + 2], 1u); any_span = true; }
		}
		if (!any_span || !idn) continue;
		long long gp = start1; int rp = 0;
		for (uint32_t k = 0; k < r.n_cigar; ++k)
		{
			const uint32_t c = ld32(r.cigar + 4ull * k), op = c & 15u; const int len = (int)(c >> 4);
			if (op == 1u || op == 2u || op == 3u)
			{
				for (int i = a; i < last && w.tab.pos[i] <= end1; ++i)
				{
					const int ws = w.tab.pos[i], we = w.win[i].end;
					if (start1 > ws || end1 < we) continue;   // (spanning records only)
					if (op == 3u) { if (gp <= ws && gp + len >= we) atomicAdd(&counts[8ull * i + 2], 0xFFFFFFFFu); }
					else if (gp >= ws && gp <= we) indel_event(w, r, i, op, len, gp, rp, counts);
				}
			}
			if ((0x18Du >> op) & 1u) gp += len;
			if (op == 0u || op == 1u || op == 4u || op == 7u || op == 8u) rp += len;
		}
		if (unknown)
			for (int i = a; i < last && w.tab.pos[i] <= end1; ++i)
				if (start1 <= w.tab.pos[i] && end1 >= w.win[i].end) atomicAdd(&counts[8ull * i + 6], 1u);
	}
}

// Records with long CIGARs: one wave per record. Pass 1 streams the operations (reference length, which kinds occur); the windows of the span are counted by
// the lanes in turn; pass 2 gives every operation its genome / read position with a wave prefix sum and looks up the windows around an I / D / N operation by
// binary search (a long read spans many windows of a dense table).
__global__ __launch_bounds__(256) void indel_long_kernel(const uint8_t* __restrict__ infl, const int64_t* __restrict__ recoff, const int64_t* __restrict__ long_list,
                                                         const unsigned long long* __restrict__ n_long_dev, const IndelTables w, uint32_t* __restrict__ counts)
{
	const int lane = threadIdx.x & 63;
	const long long wave = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((long long)gridDim.x * blockDim.x) >> 6;
	const long long n_long = (long long)*n_long_dev;
	for (long long wv = wave; wv < n_long; wv += n_waves)
	{
		RecView r = load_rec(infl, recoff[long_list[wv]]);   // (passed the read filters in indel_kernel)
		rec_apply_cg(r);
		long long ref_len = 0; bool idn = false, unknown = false;
		for (uint32_t k = lane; k < r.n_cigar; k += 64)
		{
			const uint32_t c = ld32(r.cigar + 4ull * k), op = c & 15u;
			if ((0x18Du >> op) & 1u) ref_len += c >> 4;
			idn |= op == 1u || op == 2u || op == 3u; unknown |= op == 6u || op > 8u;
		}
		ref_len = wave_sum(ref_len); idn = __any(idn); unknown = __any(unknown);
		if (ref_len == 0) ref_len = 1;
		const long long start1 = (long long)r.pos + 1, end1 = (long long)r.pos + ref_len;
		const int first = w.tab.tid_first[r.tid], last = w.tab.tid_last[r.tid];
		const int a = win_lower(w, r.tid, first, last, start1 - w.tid_maxlen[r.tid] + 1);
		const bool mq0 = r.mapq == 0;
		bool any_span = false;
		for (int i = a + lane; i < last && w.tab.pos[i] <= end1; i += 64)
		{
			if (w.win[i].end < start1) continue;
			atomicAdd(&counts[8ull * i], 1u);
			if (mq0) { atomicAdd(&counts[8ull * i + 1], 1u); continue; }
			if (start1 <= w.tab.pos[i] && end1 >= w.win[i].end)
			{
				atomicAdd(&counts[8ull * i + 2], 1u); any_span = true;
				if (unknown && idn) atomicAdd(&counts[8ull * i + 6], 1u);
			}
		}
		if (!__any(any_span) || !idn) continue;
		long long g_base = start1; long long rp_base = 0;
		for (uint32_t k0 = 0; k0 < r.n_cigar; k0 += 64u)
		{
			const uint32_t k = k0 + (uint32_t)lane;
			uint32_t op = 15u; int len = 0;
			if (k < r.n_cigar) { const uint32_t c = ld32(r.cigar + 4ull * k); op = c & 15u; len = (int)(c >> 4); }
			const long long g_own = ((0x18Du >> op) & 1u) ? len : 0, rp_own = (op == 0u || op == 1u || op == 4u || op == 7u || op == 8u) ? len : 0;
			long long g = g_own, rp = rp_own;
			#pragma unroll
			for (int o = 1; o < 64; o <<= 1) { const long long x = __shfl_up(g, o), y = __shfl_up(rp, o); if (lane >= o) { g += x; rp += y; } }
			const long long gp = g_base + g - g_own, rpos = rp_base + rp - rp_own;   // positions IN FRONT OF this lane's operation
			if (k < r.n_cigar && (op == 1u || op == 2u))
			{
				for (int i = win_lower(w, r.tid, first, last, gp - w.tid_maxlen[r.tid] + 1); i < last && w.tab.pos[i] <= gp; ++i)
				{
					const int ws = w.tab.pos[i], we = w.win[i].end;
					if (start1 <= ws && end1 >= we && gp <= we) indel_event(w, r, i, op, len, gp, (int)rpos, counts);
				}
			}
			else if (k < r.n_cigar && op == 3u)
			{
				for (int i = win_lower(w, r.tid, first, last, gp); i < last && w.tab.pos[i] <= gp + len; ++i)
				{
					const int ws = w.tab.pos[i], we = w.win[i].end;
					if (start1 <= ws && end1 >= we && gp + len >= we) atomicAdd(&counts[8ull * i + 2], 0xFFFFFFFFu);
				}
			}
			g_base += __shfl(g, 63); rp_base += __shfl(rp, 63);
		}
	}
}

void launch_indel(const uint8_t* infl, const int64_t* recoff, int64_t n_rec, const IndelTables& w, uint32_t* counts, int64_t* long_list, unsigned long long* long_count, hipStream_t s)
{
	if (n_rec <= 0) return;
	const int grid = (int)std::min<int64_t>((n_rec + 255) / 256, 256 * 32);
	hipLaunchKernelGGL(indel_kernel, dim3(grid), dim3(256), 0, s, infl, recoff, (long long)n_rec, w, counts, long_list, long_count); KCHECK();
}
void launch_indel_long(const uint8_t* infl, const int64_t* recoff, const int64_t* long_list, const unsigned long long* d_n_long, int64_t n_long_max, const IndelTables& w, uint32_t* counts, hipStream_t s)
{
	if (n_long_max <= 0) return;
	const int grid = (int)std::min<int64_t>((n_long_max + 3) / 4, 256 * 16);   // (sized for the most there can be; the waves stride over what there is)
	hipLaunchKernelGGL(indel_long_kernel, dim3(grid), dim3(256), 0, s, infl, recoff, long_list, d_n_long, w, counts); KCHECK();
}

} // namespace ngsqc
