// One read pair as SeqPurge sees it (src/SeqPurge/AnalysisWorker.cpp:79-457 run, :19-77 correctErrors; src/cppNGS/FastqFileStream.cpp:52-117 trimQuality / trimN):
// the header check, the bit planes of the two reads, the counts and the verdict of one insert offset, one adapter window, one error-correction position, the
// predicates of quality and N trimming, and the table of the binomial tail - the text csrc/purge.hip compiles into its kernels, kept free of HIP so that
// tests/emul/purge_emul.cpp runs the same text on the CPU against the Python model (tests/seqpurge_oracle.py). Integer code, except where the reference has
// doubles: the percentage test, the ceil of the mismatch budget, p > mep, p1 * p2 > mep and sum / window >= cutoff, written as the reference writes them.
// Built with -ffp-contract=off: no compare sees a fused product.
#pragma once
#include "fastq_visit.h"

namespace ngsqc {
namespace {
constexpr int PG_MAXLEN = 1000;           // Auxilary.h:12
constexpr int PG_OVERLAP = 10;            // TrimmingParameters::adapter_overlap
constexpr int PG_ADAPTER = 20;            // the bases of an adapter that are ever looked at: max(adapter_overlap, a_size)
constexpr int PG_W1 = 16, PG_W2 = 17;     // 64-bit words of a plane: positions 0..999; read 2 has one zero word more (a funnel shift reads words w and w + 1, w <= 15)
constexpr int PG_TAIL_SIZE = PG_MAXLEN * (PG_MAXLEN + 1) / 2;
constexpr int PG_PLAN = 8;                // int32 per pair: len1_in, len2_in, insert_offset, adapter_fwd, adapter_rev, len1_out, len2_out, flags
enum { PG_OK = 0, PG_ERR_LENGTHS = 1, PG_ERR_HEADER = 2, PG_ERR_BASE = 3, PG_ERR_READLEN = 4 };   // the order they are looked for
enum { PG_FLAG_Q1 = 1, PG_FLAG_Q2 = 2, PG_FLAG_N1 = 4, PG_FLAG_N2 = 8 };
enum { PG_LO = 0, PG_HI = 1, PG_N = 2, PG_OTHER = 3 };   // planes: the two bits of A C G T (0..3), "N", "any other byte"

struct PgParams
{
	uint8_t a1[PG_ADAPTER], a2[PG_ADAPTER];   // the front of the adapters (at least 15 bases each; bytes behind their end are never read)
	int a_size; double match_perc, mep; int min_len, qcut, qwin, qoff, ncut, ec;
};

// tail[n][k], 0 <= k <= n < 1000: BasicStatistics::matchProbability(0.25, k, n) = the sum over i = k..n of C(n,i) 3^(n-i) / 4^n
FQ_DEV int pg_tail_index(int k, int n) { return n * (n + 1) / 2 + k; }
FQ_DEV double pg_tail(const double* tail, int k, int n) { return tail[pg_tail_index(k, n)]; }

// The table, built once on the host in long double, the smallest term first: term(n) = 4^-n (a power of two), term(i - 1) = term(i) * 3i / (n - i + 1), and the
// tail of k is the running sum from i = n down to k. Where the terms rise towards the mode (i > n/4: every tail that can come near a sensible mep) that is the
// ascending order; at most 1000 additions and 2000 roundings of the terms at 2^-64 each keep the result within 2 ulp of the correctly rounded double.
inline void pg_build_tail(double* tail)
{
	for (int n = 0; n < PG_MAXLEN; ++n)
	{
		long double term = 1.0L;
		for (int i = 0; i < n; ++i) term *= 0.25L;
		long double sum = 0.0L;
		for (int i = n; i >= 0; --i)
		{
			sum += term;
			tail[pg_tail_index(i, n)] = (double)sum;
			term = term * (long double)(3 * i) / (long double)(n - i + 1);
		}
	}
}

// 0..3: A C G T, 4: N, 5: anything else
FQ_DEV uint32_t pg_code(uint32_t c) { return fq_base_class(c); }
FQ_DEV uint32_t pg_complement(uint32_t c) { return c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : 'N'; }   // (of A C G T N)
// position i of a read as the insert match sees it: read 1 as given, read 2 reverse-complemented (code ^ 3 for A C G T); 6: behind the end
FQ_DEV uint32_t pg_code_at(const uint8_t* s, int len, int i, bool revcomp)
{
	if (i >= len) return 6u;
	const uint32_t c = pg_code(revcomp ? s[len - 1 - i] : s[i]);
	return revcomp && c < 4u ? c ^ 3u : c;
}
FQ_DEV bool pg_plane_bit(uint32_t code, int plane)
{
	return plane == PG_LO ? (code < 4u && (code & 1u)) : plane == PG_HI ? (code < 4u && (code & 2u)) : plane == PG_N ? code == 4u : code == 5u;
}

// The first space-separated token of both headers; "/1" and "/2" are chopped only when both are there (:110-120). t1 / t2: the lengths that were compared.
FQ_DEV bool pg_headers_match(const uint8_t* h1, uint32_t n1, const uint8_t* h2, uint32_t n2, uint32_t& t1, uint32_t& t2)
{
	t1 = 0; while (t1 < n1 && h1[t1] != ' ') ++t1;
	t2 = 0; while (t2 < n2 && h2[t2] != ' ') ++t2;
	if (t1 >= 2 && t2 >= 2 && h1[t1 - 2] == '/' && h1[t1 - 1] == '1' && h2[t2 - 2] == '/' && h2[t2 - 1] == '2') { t1 -= 2; t2 -= 2; }
	if (t1 != t2) return false;
	for (uint32_t i = 0; i < t1; ++i) if (h1[i] != h2[i]) return false;
	return true;
}

FQ_DEV int pg_popc(uint64_t x) { return __builtin_popcountll(x); }
// the 64 bits of a plane from bit position `at` on (the words behind the plane's data are zero)
FQ_DEV uint64_t pg_funnel(const uint64_t* plane, int at)
{
	const int w = at >> 6, s = at & 63;
	return s ? (plane[w] >> s) | (plane[w + 1] << (64 - s)) : plane[w];
}
// Whole counts of an offset: seq1[i] against seq2[i + offset] for i < n_pos = min_length - offset (:151-168 without the early exit). p1: [4][PG_W1], p2: [4][PG_W2].
// Either base N: invalid. A byte of read 1 outside ACGTN is not N and equals nothing: a mismatch (read 2 holds none: the pair is refused).
FQ_DEV void pg_offset_counts(const uint64_t* p1, const uint64_t* p2, int offset, int n_pos, int& matches, int& mismatches, int& invalid)
{
	int m = 0, inv = 0;
	for (int w = 0; w * 64 < n_pos; ++w)
	{
		const int left = n_pos - w * 64;
		const uint64_t mask = left >= 64 ? ~0ull : (1ull << left) - 1ull;
		const uint64_t lo2 = pg_funnel(p2 + PG_LO * PG_W2, offset + w * 64), hi2 = pg_funnel(p2 + PG_HI * PG_W2, offset + w * 64), n2 = pg_funnel(p2 + PG_N * PG_W2, offset + w * 64);
		const uint64_t lo1 = p1[PG_LO * PG_W1 + w], hi1 = p1[PG_HI * PG_W1 + w], n1 = p1[PG_N * PG_W1 + w], o1 = p1[PG_OTHER * PG_W1 + w];
		const uint64_t nn = (n1 | n2) & mask;
		inv += pg_popc(nn);
		m += pg_popc(~(lo1 ^ lo2) & ~(hi1 ^ hi2) & ~o1 & ~nn & mask);
	}
	matches = m; invalid = inv; mismatches = n_pos - inv - m;
}
// the reference's own loop over the bytes, early exit included (seq2: the reverse complement of read 2) - what the whole counts are checked against
FQ_DEV void pg_offset_counts_literal(const uint8_t* seq1, const uint8_t* seq2, int offset, int min_length, double match_perc, int& matches, int& mismatches, int& invalid)
{
	const int max_mismatches = (int)(ceil((1.0 - match_perc / 100.0) * (min_length - offset)));
	matches = 0; mismatches = 0; invalid = 0;
	for (int j = offset; j < min_length; ++j)
	{
		const uint8_t b1 = seq1[j - offset], b2 = seq2[j];
		if (b1 == 'N' || b2 == 'N') ++invalid;
		else if (b1 == b2) ++matches;
		else { ++mismatches; if (mismatches > max_mismatches) break; }
	}
}
// :170 (with the budget of :146-166 as an explicit test: once the loop has left early the percentage test always fails - tests/test_cpu_seqpurge_emul.py sweeps it)
FQ_DEV bool pg_counts_skip(int matches, int mismatches, int n_pos, double match_perc)
{
	const int max_mismatches = (int)(ceil((1.0 - match_perc / 100.0) * n_pos));
	if (mismatches > max_mismatches) return true;
	return (matches + mismatches) == 0 || 100.0 * matches / (matches + mismatches) < match_perc;
}
FQ_DEV bool pg_literal_skip(int matches, int mismatches, double match_perc)
{
	return (matches + mismatches) == 0 || 100.0 * matches / (matches + mismatches) < match_perc;
}
// matches and mismatches of n bytes against the front of an adapter (:187-229)
FQ_DEV void pg_adapter_counts(const uint8_t* s, int n, const uint8_t* adapter, int& matches, int& mismatches)
{
	matches = 0; mismatches = 0;
	for (int i = 0; i < n; ++i)
	{
		const uint8_t b1 = s[i], b2 = adapter[i];
		if (b1 == 'N' || b2 == 'N') continue;
		if (b1 == b2) ++matches; else ++mismatches;
	}
}
// An offset whose counts passed :170: the tail test and the adapter check (:178-259). b1 / b2: the reads as given. true: a candidate with probability p.
FQ_DEV bool pg_insert_candidate(const uint8_t* b1, int len1, const uint8_t* b2, int len2, int offset, int matches, int mismatches, const PgParams& P, const double* tail, double& p)
{
	p = pg_tail(tail, matches, matches + mismatches);
	if (p > P.mep) return false;
	const int at = len2 - offset;                                   // (:183 takes read 2's length for read 1 as well: the slice may be short or empty)
	int n1 = len1 - at; n1 = n1 < 0 ? 0 : (n1 > PG_OVERLAP ? PG_OVERLAP : n1);
	const int n2 = offset > PG_OVERLAP ? PG_OVERLAP : offset;
	int a1_m, a1_x, a2_m, a2_x;
	pg_adapter_counts(b1 + (n1 ? at : 0), n1, P.a1, a1_m, a1_x);
	pg_adapter_counts(b2 + at, n2, P.a2, a2_m, a2_x);
	if (offset < 10)
	{
		int max_mm = 2;
		if (offset < 6) max_mm = 1;
		if (offset < 3) max_mm = 0;
		return a1_x <= max_mm || a2_x <= max_mm;
	}
	const double p1 = pg_tail(tail, a1_m, a1_m + a1_x), p2 = pg_tail(tail, a2_m, a2_m + a2_x);
	return !(p1 * p2 > P.mep);
}
// the better of two lanes' candidates: the smaller p, the smaller offset among equal ones (-1: none; a lane keeps its first candidate of a p: strict '<', :261)
FQ_DEV void pg_better(double& p, int& offset, double op, int ooffset)
{
	if (ooffset < 0) return;
	if (offset < 0 || op < p || (op == p && ooffset < offset)) { p = op; offset = ooffset; }
}
// does the adapter start at `offset` of s (:309-337, :360-389)? Windows at the read's end are shorter; 0/0 is NaN and does not skip, tail(0, 0) = 1 does.
FQ_DEV bool pg_adapter_hit(const uint8_t* s, int len, int offset, const uint8_t* adapter, const PgParams& P, const double* tail)
{
	int n = len - offset; n = n > P.a_size ? P.a_size : n;
	int matches, mismatches;
	pg_adapter_counts(s + offset, n, adapter, matches, mismatches);
	if (100.0 * matches / (matches + mismatches) < P.match_perc) return false;
	return !(pg_tail(tail, matches, matches + mismatches) > P.mep);
}
// Error correction at position i of read 1 against count - 1 - i of read 2 (:23-70), in place. 0: the bases agree, 1: a mismatch left as it is (equal
// qualities), 2: read 2 corrected, 3: read 1 corrected. A byte of read 1 outside ACGTN, which the reference cannot complement, puts N into read 2.
FQ_DEV int pg_correct(uint8_t* b1, uint8_t* q1, uint8_t* b2, uint8_t* q2, int i, int count, int qoff)
{
	const int i2 = count - i - 1;
	if (b1[i] == pg_complement(b2[i2])) return 0;
	const int v1 = (int)q1[i] - qoff, v2 = (int)q2[i2] - qoff;
	if (v1 > v2) { b2[i2] = (uint8_t)pg_complement(b1[i]); q2[i2] = q1[i]; return 2; }
	if (v1 < v2) { b1[i] = (uint8_t)pg_complement(b2[i2]); q1[i] = q2[i2]; return 3; }
	return 1;
}
// trimQuality (:52-87): does the window that starts at i reach the cutoff? (The reference's running double sum holds integers: it is exact, and equal to this one.)
FQ_DEV bool pg_qwindow_ok(const uint8_t* q, int i, int window, int qoff, int cutoff)
{
	double sum = 0;
	for (int k = 0; k < window; ++k) sum += (int)q[i + k] - qoff;
	return sum / window >= cutoff;
}
FQ_DEV bool pg_qbase_ok(const uint8_t* q, int i, int qoff, int cutoff) { return (int)q[i] - qoff >= cutoff; }
// trimN (:89-117): do num_n Ns start at i?
FQ_DEV bool pg_nrun_at(const uint8_t* b, int i, int num_n)
{
	for (int k = 0; k < num_n; ++k) if (b[i + k] != 'N') return false;
	return true;
}
// which stream takes which read of a pair (OutputWorker.cpp:38-55): 0 out1, 1 out2, 2 out3_R1, 3 out3_R2; -1: the read is dropped
FQ_DEV void pg_route(int l1, int l2, int min_len, int out3, int& s1, int& s2)
{
	s1 = s2 = -1;
	if (l1 >= min_len && l2 >= min_len) { s1 = 0; s2 = 1; }
	else if (out3 && l1 >= min_len) s1 = 2;
	else if (out3 && l2 >= min_len) s2 = 3;
}
FQ_DEV uint64_t pg_entry_bytes(const FqEntry& e, int l) { return (uint64_t)e.header.len + e.header2.len + 2ull * (uint64_t)l + 4ull; }
// byte k of an entry whose bases and qualities are cut to l
FQ_DEV uint8_t pg_entry_byte(const uint8_t* text, const FqEntry& e, uint32_t l, uint32_t k)
{
	if (k < e.header.len) return text[e.header.start + k];
	if (k == e.header.len) return '\n';
	k -= e.header.len + 1;
	if (k < l) return text[e.bases.start + k];
	if (k == l) return '\n';
	k -= l + 1;
	if (k < e.header2.len) return text[e.header2.start + k];
	if (k == e.header2.len) return '\n';
	k -= e.header2.len + 1;
	return k < l ? text[e.quals.start + k] : (uint8_t)'\n';
}
// the consensus pile-up column of a base, -1: none
FQ_DEV int pg_acons_column(uint32_t c) { const uint32_t k = pg_code(c); return k < 5u ? (int)k : -1; }
} // namespace
} // namespace ngsqc
