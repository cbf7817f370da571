// SeqPurge's per-pair text (ngs-bits_amd/csrc/purge_visit.h: what the GPU library compiles into the kernels of csrc/purge.hip) on the CPU:
// tests/test_cpu_seqpurge_emul.py runs it over FASTQ texts against the Python model (tests/seqpurge_oracle.py). The work is cut as pg_plan_kernel cuts it - a
// wave per pair, ballots over 64 lanes for the bit planes, lanes over insert offsets, adapter offsets, quality windows and N runs - with the lanes run one after
// the other. Also here: the table of the binomial tail as the library builds it, and the sweep that holds "whole counts plus the mismatch budget" to the
// reference's loop with its early exit. Test infrastructure, never linked into the library.
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <chrono>
#include <vector>
#include "../../ngs-bits_amd/csrc/purge_visit.h"

using namespace ngsqc;

namespace {
struct Lines { std::vector<uint32_t> at; uint64_t L = 0; };
Lines index_lines(const uint8_t* t, int64_t n)
{
	Lines l; l.at.push_back(0);
	for (int64_t i = 0; i < n; ++i) if (t[i] == '\n') l.at.push_back((uint32_t)(i + 1));
	l.L = l.at.size() - 1; l.at.push_back((uint32_t)n);
	return l;
}
template <typename F> uint64_t ballot(F f) { uint64_t m = 0; for (int lane = 0; lane < 64; ++lane) if (f(lane)) m |= 1ull << lane; return m; }

int adapter_scan(const uint8_t* s, int len, const uint8_t* adapter, const PgParams& P, const double* tail)
{
	for (int base = 0; base < len; base += 64)
	{
		const uint64_t m = ballot([&](int lane) { const int off = base + lane; return off < len && pg_adapter_hit(s, len, off, adapter, P, tail); });
		if (m) return base + __builtin_ctzll(m);
	}
	return -1;
}
int trim_quality(const uint8_t* q, int count, const PgParams& P)
{
	if (count < P.qwin) return count;
	int found = -1;
	for (int top = count - P.qwin; top >= 0 && found < 0; top -= 64)
	{
		const uint64_t m = ballot([&](int lane) { const int i = top - lane; return i >= 0 && pg_qwindow_ok(q, i, P.qwin, P.qoff, P.qcut); });
		if (m) found = top - __builtin_ctzll(m);
	}
	if (found < 0) return 0;
	int n = found + P.qwin;
	while (n > 0)
	{
		const uint64_t stop = ballot([&](int lane) { const int i = n - 1 - lane; return i < 0 || pg_qbase_ok(q, i, P.qoff, P.qcut); });
		if (stop) { n -= __builtin_ctzll(stop); break; }
		n -= 64;
	}
	return n;
}
int trim_n(const uint8_t* b, int count, const PgParams& P)
{
	if (count < P.ncut) return count;
	for (int base = 0; base + P.ncut <= count; base += 64)
	{
		const uint64_t m = ballot([&](int lane) { const int i = base + lane; return i + P.ncut <= count && pg_nrun_at(b, i, P.ncut); });
		if (m) return base + __builtin_ctzll(m);
	}
	return count;
}
PgParams make_params(const char* a1, const char* a2, double match_perc, double mep, const int32_t* ip)
{
	PgParams P; memset(&P, 0, sizeof(P));
	const size_t n1 = strlen(a1), n2 = strlen(a2);
	memset(P.a1, 'N', PG_ADAPTER); memset(P.a2, 'N', PG_ADAPTER);
	memcpy(P.a1, a1, n1 < (size_t)PG_ADAPTER ? n1 : PG_ADAPTER); memcpy(P.a2, a2, n2 < (size_t)PG_ADAPTER ? n2 : PG_ADAPTER);
	size_t as = n1 < n2 ? n1 : n2; P.a_size = (int)(as < 20 ? as : 20);
	P.match_perc = match_perc; P.mep = mep; P.min_len = ip[0]; P.qcut = ip[1]; P.qwin = ip[2]; P.qoff = ip[3]; P.ncut = ip[4]; P.ec = ip[5];
	return P;
}
std::vector<double>& tail_table() { static std::vector<double> t; if (t.empty()) { t.resize(PG_TAIL_SIZE); pg_build_tail(t.data()); } return t; }
} // namespace

extern "C" {

int32_t purge_tail_size() { return PG_TAIL_SIZE; }
void purge_tail_table(double* out) { memcpy(out, tail_table().data(), sizeof(double) * PG_TAIL_SIZE); }
int32_t purge_tail_index(int32_t k, int32_t n) { return pg_tail_index(k, n); }

// Every state in which the reference's loop can leave early - positions compared in all (< 1000), invalid ones and matches seen so far, mismatches = budget + 1 -
// must be skipped by its percentage test (:170), as "mismatches over budget" skips it here; and every whole count within the budget is judged by the same
// expression on both sides. Returns the number of states where the two verdicts differ.
int64_t purge_sweep(double match_perc)
{
	int64_t bad = 0;
	for (int n_pos = 1; n_pos < PG_MAXLEN; ++n_pos)
	{
		const int budget = (int)(ceil((1.0 - match_perc / 100.0) * n_pos));
		const int x = budget + 1;
		if (x < 1 || x > n_pos) continue;   // the loop cannot leave early
		for (int inv = 0; inv + x <= n_pos; ++inv)
			for (int m = 0; m + inv + x <= n_pos; ++m)
				if (!pg_literal_skip(m, x, match_perc)) ++bad;   // (whole counts: mismatches >= x > budget: skipped)
	}
	return bad;
}

// texts: as the accumulator hands them to the device (the last piece with its final newline, no empty lines at the end); both are changed in place by -ec.
// ip: min_len, qcut, qwin, qoff, ncut, ec. plan: [cap][8]. acons: 400, ec_hist: 3000. out: [0] pairs, [1] error word (all ones: none), [2] / [3] where the carry
// of side 1 / 2 starts. Returns 0, or -1 when cap is too small.
int32_t purge_emul(uint8_t* text1, int64_t n1, uint8_t* text2, int64_t n2, int32_t last, uint64_t pair_base, const char* a1, const char* a2, double match_perc, double mep,
                   const int32_t* ip, int32_t* plan, int64_t cap, uint64_t* acons, uint64_t* ec_hist, uint64_t* out)
{
	const PgParams P = make_params(a1, a2, match_perc, mep, ip);
	const double* tail = tail_table().data();
	const Lines i1 = index_lines(text1, n1), i2 = index_lines(text2, n2);
	const uint64_t E1 = last ? (i1.L + 3) / 4 : i1.L / 4, E2 = last ? (i2.L + 3) / 4 : i2.L / 4, n = E1 < E2 ? E1 : E2;
	out[0] = n; out[1] = FQ_NO_ERROR; out[2] = 4 * n <= i1.L ? i1.at[4 * n] : (uint64_t)n1; out[3] = 4 * n <= i2.L ? i2.at[4 * n] : (uint64_t)n2;
	if ((int64_t)n > cap) return -1;
	std::vector<uint64_t> planes(4 * PG_W1 + 4 * PG_W2);
	uint64_t* p1 = planes.data(); uint64_t* p2 = p1 + 4 * PG_W1;
	for (uint64_t r = 0; r < n; ++r)
	{
		const FqEntry e1 = fq_entry(text1, i1.at.data(), i1.L, r), e2 = fq_entry(text2, i2.at.data(), i2.L, r);
		uint8_t* b1 = text1 + e1.bases.start; uint8_t* q1 = text1 + e1.quals.start; uint8_t* b2 = text2 + e2.bases.start; uint8_t* q2 = text2 + e2.quals.start;
		const int len1 = (int)e1.bases.len, len2 = (int)e2.bases.len;
		int32_t* row = plan + PG_PLAN * r;
		uint32_t kind = PG_OK;
		if (e1.bases.len != e1.quals.len || e2.bases.len != e2.quals.len) kind = PG_ERR_LENGTHS;
		else
		{
			uint32_t t1, t2;
			if (!pg_headers_match(text1 + e1.header.start, e1.header.len, text2 + e2.header.start, e2.header.len, t1, t2)) kind = PG_ERR_HEADER;
			else
			{
				bool bad = false;
				for (int i = 0; i < len2; ++i) bad |= pg_code(b2[i]) == 5u;
				if (bad) kind = PG_ERR_BASE;
				else if ((len1 > len2 ? len1 : len2) >= PG_MAXLEN) kind = PG_ERR_READLEN;
			}
		}
		if (kind)
		{
			const unsigned long long w = fq_error_word(pair_base + r, kind); if (w < out[1]) out[1] = w;
			row[0] = len1; row[1] = len2; row[2] = row[3] = row[4] = -1; row[5] = len1; row[6] = len2; row[7] = 0;
			continue;
		}
		for (int w = 0; w < PG_W1; ++w)
			for (int pl = 0; pl < 4; ++pl)
			{
				p1[pl * PG_W1 + w] = ballot([&](int lane) { return pg_plane_bit(pg_code_at(b1, len1, w * 64 + lane, false), pl); });
				p2[pl * PG_W2 + w] = ballot([&](int lane) { return pg_plane_bit(pg_code_at(b2, len2, w * 64 + lane, true), pl); });
			}
		for (int pl = 0; pl < 4; ++pl) p2[pl * PG_W2 + PG_W2 - 1] = 0;
		const int min_length = len1 < len2 ? len1 : len2;
		double lane_p[64]; int lane_o[64];
		for (int lane = 0; lane < 64; ++lane)
		{
			double best_p = 1.0; int best_offset = -1;
			for (int offset = 1 + lane; offset < min_length; offset += 64)
			{
				int m, x, inv;
				pg_offset_counts(p1, p2, offset, min_length - offset, m, x, inv);
				if (pg_counts_skip(m, x, min_length - offset, P.match_perc)) continue;
				double p;
				if (!pg_insert_candidate(b1, len1, b2, len2, offset, m, x, P, tail, p)) continue;
				if (p < best_p) { best_p = p; best_offset = offset; }
			}
			lane_p[lane] = best_p; lane_o[lane] = best_offset;
		}
		for (int o = 32; o > 0; o >>= 1)   // the xor butterfly of the wave reduction
		{
			double np[64]; int no[64];
			for (int lane = 0; lane < 64; ++lane) { np[lane] = lane_p[lane]; no[lane] = lane_o[lane]; pg_better(np[lane], no[lane], lane_p[lane ^ o], lane_o[lane ^ o]); }
			memcpy(lane_p, np, sizeof(np)); memcpy(lane_o, no, sizeof(no));
		}
		const int best_offset = lane_o[0];
		int l1 = len1, l2 = len2, fwd = -1, rev = -1;
		if (best_offset != -1)
		{
			const int new_length = len2 - best_offset;
			for (int lane = 0; lane < 40; ++lane)
			{
				if (new_length + lane < len1) { const int c = pg_acons_column(b1[new_length + lane]); if (c >= 0) ++acons[lane * 5 + c]; }
				if (new_length + lane < len2) { const int c = pg_acons_column(b2[new_length + lane]); if (c >= 0) ++acons[200 + lane * 5 + c]; }
			}
			l1 = len1 < new_length ? len1 : new_length; l2 = new_length;
			if (P.ec)
			{
				const int count = l1 < l2 ? l1 : l2;
				int mm = 0;
				for (int lane = 0; lane < 64; ++lane)
					for (int i = lane; i < count; i += 64)
					{
						const int c = pg_correct(b1, q1, b2, q2, i, count, P.qoff);
						mm += c != 0;
						if (c == 2) ++ec_hist[PG_MAXLEN + count - i - 1];
						if (c == 3) ++ec_hist[i];
					}
				if (mm > 0) ++ec_hist[2 * PG_MAXLEN + mm];
			}
		}
		else
		{
			fwd = adapter_scan(b1, len1, P.a1, P, tail);
			rev = adapter_scan(b2, len2, P.a2, P, tail);
			if (fwd != -1 || rev != -1)
			{
				const int c1 = fwd != -1 ? fwd : rev, c2 = rev != -1 ? rev : fwd;
				l1 = l1 < c1 ? l1 : c1; l2 = l2 < c2 ? l2 : c2;
			}
		}
		int flags = 0;
		if (P.qcut > 0)
		{
			const int k1 = trim_quality(q1, l1, P), k2 = trim_quality(q2, l2, P);
			if (k1 < l1) flags |= PG_FLAG_Q1;
			if (k2 < l2) flags |= PG_FLAG_Q2;
			l1 = k1; l2 = k2;
		}
		if (P.ncut > 0)
		{
			const int k1 = trim_n(b1, l1, P), k2 = trim_n(b2, l2, P);
			if (k1 < l1) flags |= PG_FLAG_N1;
			if (k2 < l2) flags |= PG_FLAG_N2;
			l1 = k1; l2 = k2;
		}
		row[0] = len1; row[1] = len2; row[2] = best_offset; row[3] = fwd; row[4] = rev; row[5] = l1; row[6] = l2; row[7] = flags;
	}
	return 0;
}

// the text of output stream k (0 out1, 1 out2, 2 out3_R1, 3 out3_R2) for the first n pairs, from the plan and the (corrected) texts; returns its size, or -1
// when cap is too small
int64_t purge_format(const uint8_t* text1, int64_t n1, const uint8_t* text2, int64_t n2, const int32_t* plan, int64_t n, int32_t min_len, int32_t out3, int32_t k, uint8_t* out, int64_t cap)
{
	const Lines i1 = index_lines(text1, n1), i2 = index_lines(text2, n2);
	const bool read2 = k == 1 || k == 3;
	int64_t at = 0;
	for (int64_t r = 0; r < n; ++r)
	{
		const int l1 = plan[PG_PLAN * r + 5], l2 = plan[PG_PLAN * r + 6];
		int s1, s2; pg_route(l1, l2, min_len, out3, s1, s2);
		if ((read2 ? s2 : s1) != k) continue;
		const FqEntry e = read2 ? fq_entry(text2, i2.at.data(), i2.L, (uint64_t)r) : fq_entry(text1, i1.at.data(), i1.L, (uint64_t)r);
		const int l = read2 ? l2 : l1;
		const int64_t size = (int64_t)pg_entry_bytes(e, l);
		if (at + size > cap) return -1;
		for (int64_t x = 0; x < size; ++x) out[at + x] = pg_entry_byte(read2 ? text2 : text1, e, (uint32_t)l, (uint32_t)x);
		at += size;
	}
	return at;
}

// seconds of the per-pair loop (with the scan for the line ends in front of it; the copies of the texts are made outside the clock), for the timing record of DESIGN.md
double purge_time(const uint8_t* text1, int64_t n1, const uint8_t* text2, int64_t n2, const char* a1, const char* a2, double match_perc, double mep, const int32_t* ip, int64_t* pairs)
{
	std::vector<uint8_t> t1(text1, text1 + n1), t2(text2, text2 + n2);
	const Lines i1 = index_lines(t1.data(), n1), i2 = index_lines(t2.data(), n2);
	const int64_t n = (int64_t)((i1.L < i2.L ? i1.L : i2.L) / 4);
	std::vector<int32_t> plan((size_t)n * PG_PLAN); std::vector<uint64_t> ac(400), ec(3000); uint64_t o[4];
	(void)tail_table();
	const auto c0 = std::chrono::steady_clock::now();
	purge_emul(t1.data(), n1, t2.data(), n2, 0, 0, a1, a2, match_perc, mep, ip, plan.data(), n, ac.data(), ec.data(), o);
	const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - c0).count();
	*pairs = (int64_t)o[0];
	return s;
}
}
