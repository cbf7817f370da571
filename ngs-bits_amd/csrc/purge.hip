// Two FASTQ texts in device memory -> SeqPurge (src/SeqPurge: AnalysisWorker.cpp:79-457, OutputWorker.cpp:36-77): adapter and quality trimming of read pairs.
//   line index  the kernels of fastqin.hip (launch_fastq_line_index), once per side. Pair r is entry r of both texts.
//   plan        pg_plan_kernel: ONE WAVE PER PAIR. Both reads are packed into bit planes in LDS (two planes for A/C/G/T, one for N, one for any other byte;
//               read 2 reverse-complemented) by ballots; lanes take insert offsets, the counts of an offset come from funnel-shifted 64-bit words and
//               popcounts (purge_visit.h pg_offset_counts), the probabilities from the table built on the host (the device never evaluates a binomial);
//               the best (p, offset) by a wave reduction. Without an insert hit the adapter scans run with lanes over offsets, the first hit by ballot;
//               quality and N trimming likewise. With -ec the corrected bytes are written into the device text in place. One plan record of 8 int32 per
//               pair; the consensus pile-ups and the -ec histograms in LDS per workgroup, flushed once.
//   format      pg_sizes_kernel (the bytes a pair gives each of the four output streams, from the plan) -> BgzfStream::place -> pg_format_kernel: one wave
//               per entry writes its four lines, truncated to the plan's length, into the stream's window; the windows are deflated on the device.
// The accumulator (ngsqc_purge) takes the two texts in pieces cut anywhere; the pairs of a feed are the entries complete on both sides, the rest of either
// side waits as its carry: FastqFeed of fastq_feed.h, as the four output streams are FastqOutputs of fastq_outputs.h. The counters of TrimmingStatistics are
// summed on the host from the plan, bases_perc_trim_sum in pair order as doubles.
#include "join.h"
#include "purge_visit.h"

namespace ngsqc {
namespace {
constexpr int PG_ACONS = 2 * 40 * 5, PG_EC = 3 * PG_MAXLEN;

struct PgArgs
{
	uint8_t* text1; const uint32_t* lines1; uint64_t L1; uint8_t* text2; const uint32_t* lines2; uint64_t L2;
	int64_t n_pairs; unsigned long long pair_base;
	PgParams P; const double* tail;
	int32_t* plan; unsigned long long* acons; unsigned long long* ec; unsigned long long* err;
};

__device__ __forceinline__ int pg_wave_sum(int x)
{
	#pragma unroll
	for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
	return x;
}
__device__ __forceinline__ uint64_t pg_ballot(bool p) { return __builtin_amdgcn_ballot_w64(p); }

// the first offset of s at which the adapter is found, -1: none (lanes over offsets, the first hit by ballot)
__device__ int pg_adapter_scan(const uint8_t* s, int len, const uint8_t* adapter, const PgParams& P, const double* tail, int lane)
{
	for (int base = 0; base < len; base += 64)
	{
		const int off = base + lane;
		const uint64_t m = pg_ballot(off < len && pg_adapter_hit(s, len, off, adapter, P, tail));
		if (m) return base + (int)__builtin_ctzll(m);
	}
	return -1;
}
// FastqEntry::trimQuality: the new length (lanes over window starts from the end; then over the bases at the window's end)
__device__ int pg_trim_quality(const uint8_t* q, int count, const PgParams& P, int lane)
{
	if (count < P.qwin) return count;
	int found = -1;
	for (int top = count - P.qwin; top >= 0 && found < 0; top -= 64)
	{
		const int i = top - lane;
		const uint64_t m = pg_ballot(i >= 0 && pg_qwindow_ok(q, i, P.qwin, P.qoff, P.qcut));
		if (m) found = top - (int)__builtin_ctzll(m);
	}
	if (found < 0) return 0;
	int n = found + P.qwin;
	while (n > 0)
	{
		const int i = n - 1 - lane;
		const uint64_t stop = pg_ballot(i < 0 || pg_qbase_ok(q, i, P.qoff, P.qcut));
		if (stop) { n -= (int)__builtin_ctzll(stop); break; }
		n -= 64;
	}
	return n;
}
// FastqEntry::trimN: the new length
__device__ int pg_trim_n(const uint8_t* b, int count, const PgParams& P, int lane)
{
	if (count < P.ncut) return count;
	for (int base = 0; base + P.ncut <= count; base += 64)
	{
		const int i = base + lane;
		const uint64_t m = pg_ballot(i + P.ncut <= count && pg_nrun_at(b, i, P.ncut));
		if (m) return base + (int)__builtin_ctzll(m);
	}
	return count;
}
} // namespace

__global__ __launch_bounds__(256) void pg_plan_kernel(const PgArgs a)
{
	__shared__ uint64_t s_planes[4][4 * PG_W1 + 4 * PG_W2];
	__shared__ uint32_t s_acons[PG_ACONS], s_ec[PG_EC];
	__shared__ PgParams s_P;   // (the adapters are read through pointers: LDS, not the kernel's arguments)
	if (threadIdx.x == 0) s_P = a.P;
	for (int i = threadIdx.x; i < PG_ACONS; i += 256) s_acons[i] = 0;
	for (int i = threadIdx.x; i < PG_EC; i += 256) s_ec[i] = 0;
	__syncthreads();
	const int lane = threadIdx.x & 63;
	uint64_t* p1 = s_planes[threadIdx.x >> 6]; uint64_t* p2 = p1 + 4 * PG_W1;
	const long long wave = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((long long)gridDim.x * blockDim.x) >> 6;
	const PgParams& P = s_P;
	for (long long r = wave; r < a.n_pairs; r += n_waves)
	{
		const FqEntry e1 = fq_entry(a.text1, a.lines1, a.L1, (uint64_t)r), e2 = fq_entry(a.text2, a.lines2, a.L2, (uint64_t)r);
		uint8_t* b1 = a.text1 + e1.bases.start; uint8_t* q1 = a.text1 + e1.quals.start;
		uint8_t* b2 = a.text2 + e2.bases.start; uint8_t* q2 = a.text2 + e2.quals.start;
		const int len1 = (int)e1.bases.len, len2 = (int)e2.bases.len;
		int32_t* row = a.plan + PG_PLAN * r;
		// ---- what refuses the pair, in the order lengths, headers, bases of read 2, read length
		uint32_t kind = PG_OK;
		if (e1.bases.len != e1.quals.len || e2.bases.len != e2.quals.len) kind = PG_ERR_LENGTHS;
		else
		{
			int ok = 1;
			if (lane == 0) { uint32_t t1, t2; ok = pg_headers_match(a.text1 + e1.header.start, e1.header.len, a.text2 + e2.header.start, e2.header.len, t1, t2) ? 1 : 0; }
			ok = __builtin_amdgcn_readfirstlane(ok);
			if (!ok) kind = PG_ERR_HEADER;
			else
			{
				bool bad = false;
				for (int i = lane; i < len2; i += 64) bad |= pg_code(b2[i]) == 5u;
				if (pg_ballot(bad)) kind = PG_ERR_BASE;
				else if ((len1 > len2 ? len1 : len2) >= PG_MAXLEN) kind = PG_ERR_READLEN;
			}
		}
		if (kind)
		{
			if (lane == 0)
			{
				atomicMin(a.err, fq_error_word(a.pair_base + (unsigned long long)r, kind));
				row[0] = len1; row[1] = len2; row[2] = row[3] = row[4] = -1; row[5] = len1; row[6] = len2; row[7] = 0;
			}
			continue;
		}
		// ---- the bit planes (both lengths are below 1000 here)
		__builtin_amdgcn_wave_barrier();
		#pragma unroll 1
		for (int w = 0; w < PG_W1; ++w)
		{
			const int i = w * 64 + lane;
			const uint32_t c1 = pg_code_at(b1, len1, i, false), c2 = pg_code_at(b2, len2, i, true);
			#pragma unroll
			for (int pl = 0; pl < 4; ++pl)
			{
				const uint64_t m1 = pg_ballot(pg_plane_bit(c1, pl)), m2 = pg_ballot(pg_plane_bit(c2, pl));
				if (lane == 0) { p1[pl * PG_W1 + w] = m1; p2[pl * PG_W2 + w] = m2; }
			}
		}
		if (lane < 4) p2[lane * PG_W2 + PG_W2 - 1] = 0;
		__threadfence_block(); __builtin_amdgcn_wave_barrier();
		// ---- step 1: the insert match, lanes over offsets
		const int min_length = len1 < len2 ? len1 : len2;
		double best_p = 1.0; int best_offset = -1;
		for (int offset = 1 + lane; offset < min_length; offset += 64)
		{
			int m, x, inv;
			pg_offset_counts(p1, p2, offset, min_length - offset, m, x, inv);
			if (pg_counts_skip(m, x, min_length - offset, P.match_perc)) continue;
			double p;
			if (!pg_insert_candidate(b1, len1, b2, len2, offset, m, x, P, a.tail, p)) continue;
			if (p < best_p) { best_p = p; best_offset = offset; }
		}
		#pragma unroll
		for (int o = 32; o > 0; o >>= 1) { const double op = __shfl_xor(best_p, o); const int oo = __shfl_xor(best_offset, o); pg_better(best_p, best_offset, op, oo); }
		int l1 = len1, l2 = len2, fwd = -1, rev = -1;
		if (best_offset != -1)
		{
			const int new_length = len2 - best_offset;
			if (lane < 40)
			{
				if (new_length + lane < len1) { const int c = pg_acons_column(b1[new_length + lane]); if (c >= 0) atomicAdd(&s_acons[lane * 5 + c], 1u); }
				if (new_length + lane < len2) { const int c = pg_acons_column(b2[new_length + lane]); if (c >= 0) atomicAdd(&s_acons[200 + lane * 5 + c], 1u); }
			}
			l1 = len1 < new_length ? len1 : new_length; l2 = new_length;
			if (P.ec)
			{
				const int count = l1 < l2 ? l1 : l2;
				int mm = 0;
				for (int i = lane; i < count; i += 64)
				{
					const int c = pg_correct(b1, q1, b2, q2, i, count, P.qoff);
					mm += c != 0;
					if (c == 2) atomicAdd(&s_ec[PG_MAXLEN + count - i - 1], 1u);
					if (c == 3) atomicAdd(&s_ec[i], 1u);
				}
				mm = pg_wave_sum(mm);
				if (mm > 0 && lane == 0) atomicAdd(&s_ec[2 * PG_MAXLEN + mm], 1u);
				__threadfence_block(); __builtin_amdgcn_wave_barrier();   // the trimming below reads the corrected bytes
			}
		}
		else
		{
			// ---- steps 2 and 3: the adapters alone
			fwd = pg_adapter_scan(b1, len1, P.a1, P, a.tail, lane);
			rev = pg_adapter_scan(b2, len2, P.a2, P, a.tail, lane);
			if (fwd != -1 || rev != -1)
			{
				const int c1 = fwd != -1 ? fwd : rev, c2 = rev != -1 ? rev : fwd;
				l1 = l1 < c1 ? l1 : c1; l2 = l2 < c2 ? l2 : c2;
			}
		}
		int flags = 0;
		if (P.qcut > 0)
		{
			const int n1 = pg_trim_quality(q1, l1, P, lane), n2 = pg_trim_quality(q2, l2, P, lane);
			if (n1 < l1) flags |= PG_FLAG_Q1;
			if (n2 < l2) flags |= PG_FLAG_Q2;
			l1 = n1; l2 = n2;
		}
		if (P.ncut > 0)
		{
			const int n1 = pg_trim_n(b1, l1, P, lane), n2 = pg_trim_n(b2, l2, P, lane);
			if (n1 < l1) flags |= PG_FLAG_N1;
			if (n2 < l2) flags |= PG_FLAG_N2;
			l1 = n1; l2 = n2;
		}
		if (lane == 0) { row[0] = len1; row[1] = len2; row[2] = best_offset; row[3] = fwd; row[4] = rev; row[5] = l1; row[6] = l2; row[7] = flags; }
	}
	__syncthreads();
	for (int i = threadIdx.x; i < PG_ACONS; i += 256) if (s_acons[i]) atomicAdd(&a.acons[i], (unsigned long long)s_acons[i]);
	for (int i = threadIdx.x; i < PG_EC; i += 256) if (s_ec[i]) atomicAdd(&a.ec[i], (unsigned long long)s_ec[i]);
}

namespace {
struct PgOutArgs { const uint8_t* text1; const uint32_t* lines1; uint64_t L1; const uint8_t* text2; const uint32_t* lines2; uint64_t L2; int64_t n_pairs; const int32_t* plan; int min_len, out3; };
} // namespace

// sz[k][r]: the bytes pair r gives stream k
__global__ __launch_bounds__(256) void pg_sizes_kernel(const PgOutArgs a, uint64_t* __restrict__ sz0, uint64_t* __restrict__ sz1, uint64_t* __restrict__ sz2, uint64_t* __restrict__ sz3)
{
	const int64_t stride = (int64_t)gridDim.x * blockDim.x;
	for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < a.n_pairs; r += stride)
	{
		const int l1 = a.plan[PG_PLAN * r + 5], l2 = a.plan[PG_PLAN * r + 6];
		int s1, s2; pg_route(l1, l2, a.min_len, a.out3, s1, s2);
		const uint64_t n1 = s1 >= 0 ? pg_entry_bytes(fq_entry(a.text1, a.lines1, a.L1, (uint64_t)r), l1) : 0, n2 = s2 >= 0 ? pg_entry_bytes(fq_entry(a.text2, a.lines2, a.L2, (uint64_t)r), l2) : 0;
		sz0[r] = s1 == 0 ? n1 : 0; sz1[r] = s2 == 1 ? n2 : 0; sz2[r] = s1 == 2 ? n1 : 0; sz3[r] = s2 == 3 ? n2 : 0;
	}
}
// one wave per entry of stream k: the bytes of the entry that fall inside the window
__global__ __launch_bounds__(256) void pg_format_kernel(const PgOutArgs a, int k, const uint64_t* __restrict__ sz, const uint64_t* __restrict__ off, int64_t ws, Win w)
{
	const int lane = threadIdx.x & 63;
	const int64_t nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
	const bool read2 = k == 1 || k == 3;
	const uint8_t* text = read2 ? a.text2 : a.text1;
	for (int64_t r = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; r < a.n_pairs; r += nw)
	{
		const int64_t size = (int64_t)sz[r];
		if (!size) continue;
		const int64_t pos = (int64_t)off[r] - ws;
		const int64_t lo = max(pos, w.lo), hi = min(pos + size, w.hi);
		if (lo >= hi) continue;
		const FqEntry e = read2 ? fq_entry(a.text2, a.lines2, a.L2, (uint64_t)r) : fq_entry(a.text1, a.lines1, a.L1, (uint64_t)r);
		const uint32_t l = (uint32_t)a.plan[PG_PLAN * r + (read2 ? 6 : 5)];
		for (int64_t x = lo + lane; x < hi; x += 64) w.base[x] = pg_entry_byte(text, e, l, (uint32_t)(x - pos));
	}
}
} // namespace ngsqc

// ---------------------------------------------------------------- the accumulator behind the C ABI
#include "fastq_feed.h"
#include "fastq_outputs.h"
using namespace ngsqc::lib;

struct ngsqc_purge
{
	std::string err; bool failed = false;
	PgParams P{}; std::string a1, a2; CallSwitches sw;
	DevBuf<double> d_tail;
	FastqFeed in; std::string name[2] = {"in1", "in2"};   // (in front of out: fastq_outputs.h)
	std::unique_ptr<Timer> plan_clock;
	DevBuf<int32_t> d_plan; DevBuf<unsigned long long> d_acons, d_ec, d_err;
	FastqOutputs out; bool out3 = false;
	std::vector<int32_t> h_plan, all_plan;
	ngsqc_purge_stats st{};

	static void check_adapter(const char* s, const char* which, std::string& dst)
	{
		if (!s) throw ArgError(std::string("ngsqc_purge_create: no ") + which + " adapter");
		dst = s;
		if (dst.size() < 15) throw ArgError(std::string(which) + " adapter " + dst + " too short!");
		for (char c : dst) if (fq_base_class((uint8_t)c) > 4u) throw ArgError(std::string(which) + " adapter " + dst + " holds the byte '" + c + "': only A, C, G, T and N are allowed in an adapter");
	}
	void init(int dev, const ngsqc_purge_params* p)
	{
		if (!p) throw ArgError("ngsqc_purge_create: no parameters");
		check_adapter(p->a1, "Forward", a1); check_adapter(p->a2, "Reverse", a2);
		if (p->qwin < 1) throw ArgError("The quality trimming window (qwin) must be at least 1, it is " + std::to_string(p->qwin) + "!");
		memset(P.a1, 'N', PG_ADAPTER); memset(P.a2, 'N', PG_ADAPTER);
		memcpy(P.a1, a1.data(), std::min<size_t>(a1.size(), PG_ADAPTER)); memcpy(P.a2, a2.data(), std::min<size_t>(a2.size(), PG_ADAPTER));
		P.a_size = (int)std::min<size_t>(20, std::min(a1.size(), a2.size()));
		P.match_perc = p->match_perc; P.mep = p->mep; P.min_len = p->min_len; P.qcut = p->qcut; P.qwin = p->qwin; P.qoff = p->qoff; P.ncut = p->ncut; P.ec = p->ec ? 1 : 0;
		in.open(dev, 2); st.err_pair = -1;
		plan_clock.reset(new Timer(in.stream)); out.init("SeqPurge", 4, in.device, in.stream);
		std::vector<double> tail((size_t)PG_TAIL_SIZE); pg_build_tail(tail.data());
		d_tail.upload(tail, in.stream);
		d_acons.alloc(PG_ACONS); d_ec.alloc(PG_EC); d_err.alloc(1);
		HIPCHK(hipMemsetAsync(d_acons.p, 0, PG_ACONS * 8, in.stream)); HIPCHK(hipMemsetAsync(d_ec.p, 0, PG_EC * 8, in.stream)); HIPCHK(hipMemsetAsync(d_err.p, 0xff, 8, in.stream));
		HIPCHK(hipStreamSynchronize(in.stream));
	}
	void outputs(const char* o1, const char* o2, const char* o3a, const char* o3b, int level)
	{
		if (out.opened || st.pairs) throw ArgError("ngsqc_purge_outputs: the outputs are set once, before the first feed");
		if (!o1 || !o2) throw ArgError("ngsqc_purge_outputs: out1 and out2 are needed");
		if ((o3a != nullptr) != (o3b != nullptr)) throw ArgError("ngsqc_purge_outputs: out3_r1 and out3_r2 are set together");
		if (level < 0 || level > 9) throw ArgError("compression level " + std::to_string(level) + " is not in 0..9");
		const char* paths[4] = {o1, o2, o3a, o3b};
		out.open(paths, write_window_bytes(sw.write_window_pieces), level);
		out3 = o3a != nullptr;
	}
	void build_error(unsigned long long word)
	{
		const uint64_t pair = word >> 8, r = pair - (uint64_t)st.pairs; const int kind = (int)(word & 255);
		std::string l1[4], l2[4]; in.entry_lines(0, r, l1); in.entry_lines(1, r, l2);
		std::string m;
		if (kind == PG_ERR_LENGTHS)
		{
			const int which = l1[1].size() != l1[3].size() ? 1 : 2; const std::string* l = which == 1 ? l1 : l2;
			m = "Differing length of bases (" + std::to_string(l[1].size()) + ") and qualities (" + std::to_string(l[3].size()) + ") in read " + std::to_string(which) + " of pair " + std::to_string(pair) + ": '" + l[0] + "'.";
		}
		else if (kind == PG_ERR_HEADER)
		{
			uint32_t t1, t2; (void)pg_headers_match((const uint8_t*)l1[0].data(), (uint32_t)l1[0].size(), (const uint8_t*)l2[0].data(), (uint32_t)l2[0].size(), t1, t2);
			m = "Headers of reads do not match:\n" + l1[0].substr(0, t1) + "\n" + l2[0].substr(0, t2);
		}
		else if (kind == PG_ERR_BASE)
		{
			char c = '?'; for (size_t i = l2[1].size(); i-- > 0;) if (fq_base_class((uint8_t)l2[1][i]) == 5u) { c = l2[1][i]; break; }   // (the first of the reversed read)
			m = std::string("Could not convert base '") + c + "' to complement!";
		}
		else m = "Read length unsupported! A maximum read length of " + std::to_string(PG_MAXLEN) + " is supported!";
		err = m; failed = true; st.err_pair = (int64_t)pair; st.err_kind = kind;
	}
	void add_stats(int64_t n)
	{
		for (int64_t r = 0; r < n; ++r)
		{
			const int32_t* row = h_plan.data() + PG_PLAN * r;
			const int l1 = row[5], l2 = row[6];
			st.read_num += 2;
			if (row[2] >= 0) st.reads_trimmed_insert += 2;
			else if (row[3] >= 0 || row[4] >= 0) st.reads_trimmed_adapter += 2;
			st.reads_trimmed_q += ((row[7] & PG_FLAG_Q1) != 0) + ((row[7] & PG_FLAG_Q2) != 0);
			st.reads_trimmed_n += ((row[7] & PG_FLAG_N1) != 0) + ((row[7] & PG_FLAG_N2) != 0);
			if (l1 >= P.min_len && l2 >= P.min_len) {}
			else if (out3 && (l1 >= P.min_len || l2 >= P.min_len)) st.reads_removed += 1;
			else st.reads_removed += 2;
			++st.bases_remaining[l1]; ++st.bases_remaining[l2];
			if (row[0] > 0) st.bases_perc_trim_sum += (double)(row[0] - l1) / row[0];
			if (row[1] > 0) st.bases_perc_trim_sum += (double)(row[1] - l2) / row[1];
		}
	}
	int feed(const uint8_t* t1, int64_t n1, const uint8_t* t2, int64_t n2, int last)
	{
		if (n1 < 0 || n2 < 0 || (n1 && !t1) || (n2 && !t2)) throw ArgError("ngsqc_purge_feed: invalid text");
		if (out.finished) throw ArgError("ngsqc_purge_feed: the outputs are closed");
		if (failed) return NGSQC_E_FORMAT;
		HIPCHK(hipSetDevice(in.device));
		const uint8_t* tx[2] = {t1, t2}; const int64_t nn[2] = {n1, n2};
		const int64_t n = in.feed("ngsqc_purge_feed", tx, nn, last != 0, st.h2d_ms, st.index_ms, st.wait_ms);
		if (n < 0) return NGSQC_OK;
		const FastqFeed::Side* side = in.side; hipStream_t stream = in.stream;
		if (n)
		{
			d_plan.ensure_slack((size_t)n * PG_PLAN);
			PgArgs a{side[0].d_text.p, side[0].d_lines.p, side[0].L, side[1].d_text.p, side[1].d_lines.p, side[1].L, n, (unsigned long long)st.pairs, P, d_tail.p,
			         d_plan.p, d_acons.p, d_ec.p, d_err.p};
			plan_clock->start();
			const int64_t wgs = std::min<int64_t>((n + 3) / 4, 256 * 8);
			hipLaunchKernelGGL(pg_plan_kernel, dim3((unsigned)wgs), dim3(256), 0, stream, a); KCHECK();
			plan_clock->mark();
			h_plan.resize((size_t)n * PG_PLAN);
			unsigned long long e_word = FQ_NO_ERROR;
			HIPCHK(hipMemcpyAsync(h_plan.data(), d_plan.p, h_plan.size() * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
			HIPCHK(hipMemcpyAsync(&e_word, d_err.p, 8, hipMemcpyDeviceToHost, stream));
			const double w1 = wall_ms();
			HIPCHK(hipStreamSynchronize(stream));
			st.wait_ms += wall_ms() - w1;
			st.plan_ms += plan_clock->elapsed();
			if (e_word != FQ_NO_ERROR) { build_error(e_word); return NGSQC_E_FORMAT; }
			if (out.opened) write_out(n);
			else all_plan.insert(all_plan.end(), h_plan.begin(), h_plan.end());
			add_stats(n);
			st.pairs += n;
		}
		// the carry: what lies behind the last pair on either side; text left on a side behind the last piece is entries without a mate
		const int rest = in.cut_carry(n, last != 0);
		for (int k = 0; k < 2; ++k)
			if (last && (rest >> k & 1) && !failed) { err = "File " + name[k] + " has more entries than " + name[k ^ 1] + "!"; failed = true; st.err_pair = st.pairs; st.err_kind = 0; }
		return failed ? NGSQC_E_FORMAT : NGSQC_OK;
	}
	void write_out(int64_t n)
	{
		const FastqFeed::Side* side = in.side;
		PgOutArgs oa{side[0].d_text.p, side[0].d_lines.p, side[0].L, side[1].d_text.p, side[1].d_lines.p, side[1].L, n, d_plan.p, P.min_len, out3 ? 1 : 0};
		out.begin(n);
		hipLaunchKernelGGL(pg_sizes_kernel, dim3(grid_for(n)), dim3(256), 0, in.stream, oa, out.d_sz[0].p, out.d_sz[1].p, out.d_sz[2].p, out.d_sz[3].p); KCHECK();
		out.write(n, st.format_ms, st.deflate_ms, [&](int k, const Win& win, int64_t ws) {
			hipLaunchKernelGGL(pg_format_kernel, dim3(grid_for(n, 4)), dim3(256), 0, in.stream, oa, k, out.d_sz[k].p, out.d_off[k].p, ws, win); KCHECK();
		});
	}
	void result(ngsqc_purge_stats* o)
	{
		HIPCHK(hipSetDevice(in.device));
		if (!failed) out.finish();
		std::vector<unsigned long long> ac(PG_ACONS), ec(PG_EC);
		HIPCHK(hipMemcpyAsync(ac.data(), d_acons.p, ac.size() * 8, hipMemcpyDeviceToHost, in.stream)); HIPCHK(hipMemcpyAsync(ec.data(), d_ec.p, ec.size() * 8, hipMemcpyDeviceToHost, in.stream));
		HIPCHK(hipStreamSynchronize(in.stream));
		for (int i = 0; i < PG_ACONS; ++i) st.acons[i] = (int64_t)ac[i];
		for (int i = 0; i < PG_MAXLEN; ++i) { st.ec_mismatch_r1[i] = (int64_t)ec[i]; st.ec_mismatch_r2[i] = (int64_t)ec[PG_MAXLEN + i]; st.ec_errors_per_read[i] = (int64_t)ec[2 * PG_MAXLEN + i]; }
		if (o) *o = st;
	}
};

namespace { thread_local std::string g_purge_error; }

extern "C" {
int ngsqc_purge_create(int32_t device, const ngsqc_purge_params* params, ngsqc_purge** out)
{
	if (!out) return NGSQC_E_ARG;
	*out = nullptr;
	return fastq_guard((ngsqc_purge*)nullptr, g_purge_error, [&] { std::unique_ptr<ngsqc_purge> p(new ngsqc_purge); p->init(device, params); *out = p.release(); return NGSQC_OK; });
}
void ngsqc_purge_destroy(ngsqc_purge* p) { delete p; }
const char* ngsqc_purge_last_error(const ngsqc_purge* p) { return p ? p->err.c_str() : g_purge_error.c_str(); }
int ngsqc_purge_outputs(ngsqc_purge* p, const char* out1, const char* out2, const char* out3_r1, const char* out3_r2, int32_t compression_level)
{
	if (!p) return NGSQC_E_ARG;
	return fastq_guard(p, g_purge_error, [&] { p->outputs(out1, out2, out3_r1, out3_r2, compression_level); return NGSQC_OK; });
}
int ngsqc_purge_file_names(ngsqc_purge* p, const char* name1, const char* name2)
{
	if (!p || !name1 || !name2) return NGSQC_E_ARG;
	return fastq_guard(p, g_purge_error, [&] { p->name[0] = name1; p->name[1] = name2; return NGSQC_OK; });
}
int ngsqc_purge_feed(ngsqc_purge* p, const uint8_t* text1, int64_t n1, const uint8_t* text2, int64_t n2, int32_t last)
{
	if (!p) return NGSQC_E_ARG;
	return fastq_guard(p, g_purge_error, [&] { return p->feed(text1, n1, text2, n2, last); });
}
int ngsqc_purge_result(ngsqc_purge* p, ngsqc_purge_stats* st)
{
	if (!p) return NGSQC_E_ARG;
	return fastq_guard(p, g_purge_error, [&] { p->result(st); return p->failed ? NGSQC_E_FORMAT : NGSQC_OK; });
}
int ngsqc_purge_plan(ngsqc_purge* p, int64_t first, int64_t n, int32_t* out)
{
	if (!p) return NGSQC_E_ARG;
	return fastq_guard(p, g_purge_error, [&] {
		if (p->out.opened) throw ArgError("ngsqc_purge_plan: the plan is kept only when no outputs are set");
		if (first < 0 || n < 0 || (n && !out) || (uint64_t)(first + n) * PG_PLAN > p->all_plan.size()) throw ArgError("ngsqc_purge_plan: pairs out of range");
		std::copy(p->all_plan.begin() + first * PG_PLAN, p->all_plan.begin() + (first + n) * PG_PLAN, out);
		return NGSQC_OK; });
}
}
