// One FASTQ entry as ReadQC sees it (src/cppNGS/FastqFileStream.cpp:3-44 FastqEntry::validate, :133-156 readEntry; src/cppNGS/StatisticsReads.cpp:26-81
// update(const FastqEntry&)): the newline mask of 16 bytes of text, the four lines of an entry from the line index, validation, the class of one character,
// and the per-read mean with its bins - the text csrc/fastqin.hip compiles into its kernels, kept free of HIP so that tests/emul/fastqin_emul.cpp runs the
// same text on the CPU against the Python model (tests/fastq_model.py). Plain integer code, except the mean (the reference's double expressions).
#pragma once
#include <cstdint>
#include <cmath>

#ifndef FQ_DEV
#ifdef __HIPCC__
#define FQ_DEV __host__ __device__ __forceinline__
#else
#define FQ_DEV inline
#endif
#endif

namespace ngsqc {
namespace {
constexpr uint32_t FQ_BLOCK = 4096;         // bytes of text per workgroup of the line index: 256 lanes, one 16-byte load each
constexpr uint32_t FQ_LEN_DENSE = 1u << 20; // read lengths below this are counted in a dense histogram; longer reads leave their length in a list
// error kinds in the order FastqEntry::validate throws them; 6: an entry with an empty header line (which the reference does not validate) that update() cannot take
enum { FQ_OK = 0, FQ_ERR_HEADER = 1, FQ_ERR_HEADER2 = 2, FQ_ERR_LENGTH = 3, FQ_ERR_BASE = 4, FQ_ERR_QUALITY = 5, FQ_ERR_EMPTY_HEADER = 6 };
constexpr unsigned long long FQ_NO_ERROR = ~0ull;

// bit k of the result: byte k of the 16 bytes (four little-endian words, in memory order) is '\n'
FQ_DEV uint32_t fq_newline_mask4(uint32_t w)
{
	const uint32_t x = w ^ 0x0a0a0a0au;
	const uint32_t t = ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x | 0x7f7f7f7fu);   // 0x80 in exactly the bytes of x that are 0 (no carry crosses a byte)
	return ((t >> 7) * 0x01020408u) >> 24;                                     // bits 0, 8, 16, 24 -> bits 0..3 (all partial products land on distinct bits)
}
FQ_DEV uint32_t fq_newline_mask16(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3)
{
	return fq_newline_mask4(w0) | (fq_newline_mask4(w1) << 4) | (fq_newline_mask4(w2) << 8) | (fq_newline_mask4(w3) << 12);
}
// the bits of a lane's mask whose bytes lie in front of the end of the text (pos: offset of the lane's first byte)
FQ_DEV uint32_t fq_mask_in_range(uint32_t mask, uint64_t pos, uint64_t n)
{
	return pos + 16 <= n ? mask : pos >= n ? 0u : mask & ((1u << (uint32_t)(n - pos)) - 1u);
}

// Line j of the text: [start, start + len), the '\n' and one '\r' in front of it left out. lines[j] is the offset of the first byte of line j, for j in
// 0 .. n_lines (lines[n_lines] = the byte behind the last '\n'). A line at or behind n_lines (the missing lines of an incomplete last entry) is empty.
struct FqLine { uint32_t start, len; };
FQ_DEV FqLine fq_line(const uint8_t* text, const uint32_t* lines, uint64_t n_lines, uint64_t j)
{
	FqLine l{0u, 0u};
	if (j >= n_lines) return l;
	l.start = lines[j];
	uint32_t end = lines[j + 1] - 1u;   // the '\n'
	if (end > l.start && text[end - 1] == '\r') --end;
	l.len = end - l.start;
	return l;
}
struct FqEntry { FqLine header, bases, header2, quals; };
FQ_DEV FqEntry fq_entry(const uint8_t* text, const uint32_t* lines, uint64_t n_lines, uint64_t r)
{
	FqEntry e;
	e.header = fq_line(text, lines, n_lines, 4 * r); e.bases = fq_line(text, lines, n_lines, 4 * r + 1);
	e.header2 = fq_line(text, lines, n_lines, 4 * r + 2); e.quals = fq_line(text, lines, n_lines, 4 * r + 3);
	return e;
}

// what can be said without looking at the bases and qualities (validate's first three checks, in its order). An entry with an empty header is not validated
// (FastqFileStream.cpp:151); update() then reads qualities[i] for every base: differing lengths are kind 6 there.
FQ_DEV uint32_t fq_entry_kind(const uint8_t* text, const FqEntry& e)
{
	if (e.header.len == 0) return e.bases.len != e.quals.len ? (uint32_t)FQ_ERR_EMPTY_HEADER : (uint32_t)FQ_OK;
	if (text[e.header.start] != '@') return FQ_ERR_HEADER;
	if (e.header2.len == 0 || text[e.header2.start] != '+') return FQ_ERR_HEADER2;
	if (e.bases.len != e.quals.len) return FQ_ERR_LENGTH;
	return FQ_OK;
}
// 0..4: A, C, G, T, N (the order of ngsqc_read_stats.bases); 5: anything else
FQ_DEV uint32_t fq_base_class(uint32_t c) { return c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : c == 'T' ? 3u : c == 'N' ? 4u : 5u; }
FQ_DEV bool fq_quality_ok(uint32_t c, int long_read) { return c >= 33u && c <= (long_read ? 126u : 74u); }
// the kind of a character error inside an entry (bases are checked in front of qualities, :21-43)
FQ_DEV uint32_t fq_char_kind(bool header_empty, bool bad_base, bool bad_quality)
{
	if (!bad_base && !bad_quality) return FQ_OK;
	return header_empty ? (uint32_t)FQ_ERR_EMPTY_HEADER : bad_base ? (uint32_t)FQ_ERR_BASE : (uint32_t)FQ_ERR_QUALITY;
}
// the lowest entry wins and, within it, the lowest kind
FQ_DEV unsigned long long fq_error_word(uint64_t entry, uint32_t kind) { return ((unsigned long long)entry << 8) | kind; }

// StatisticsReads.cpp:70-80 for cycles > 0: rq = the bin of read_qualities_[std::round(mean)] (-1: outside 0..99), qd = the bin of Histogram(0,60,1).inc(mean, true)
FQ_DEV void fq_mean_bins(uint64_t qsum, uint32_t cycles, int& rq, int& qd)
{
	const double mean = (double)qsum / (double)cycles;
	const long long r = (long long)round(mean);
	rq = r >= 0 && r < 100 ? (int)r : -1;
	const double v = mean < 0.0 ? 0.0 : (mean > 60.0 ? 60.0 : mean);
	int b = (int)floor((v - 0.0) / (60.0 - 0.0) * 60.0); b = b < 0 ? 0 : (b > 59 ? 59 : b);
	qd = b;
}

// one cycle of an entry: the class of its base, its quality value (c - 33; 0 for a character outside the range, which is an error) and whether that is in range
struct FqChar { uint32_t cls, q; bool ok; };
FQ_DEV FqChar fq_char(uint32_t base_c, uint32_t qual_c, int long_read)
{
	FqChar r; r.cls = fq_base_class(base_c); r.ok = fq_quality_ok(qual_c, long_read); r.q = r.ok ? qual_c - 33u : 0u;
	return r;
}
} // namespace
} // namespace ngsqc
