// The device's FASTQ reader (ngs-bits_amd/csrc/fastq_visit.h: the text the GPU library compiles into the kernels of csrc/fastqin.hip) on the CPU:
// tests/test_cpu_readqc_emul.py runs it over FASTQ texts against the Python model. The work is cut as the kernels cut it - 16 bytes per lane and 256 lanes per
// block for the line index, the 64 strided slices of a wave's lanes for an entry - with the lanes run one after the other. Test infrastructure, never linked
// into the library.
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>
#include "../../ngs-bits_amd/csrc/fastq_visit.h"

using namespace ngsqc;

extern "C" {

int32_t fastq_block() { return (int32_t)FQ_BLOCK; }

// acc: [0] forward, [1] reverse, [2] bases sequenced, [3..7] A C G T N, [8..107] base qualities, [108..207] read qualities, [208..327] the two mean histograms.
// out: [0] lines, [1] entries, [2] carry start, [3] error word (all ones: none), [4] entries with a header, [5] longest read. len_hist: len_cap + 1 counters.
// cyc: [320][7]. lines_out (n + 2 values): the line index.
void fastq_emul(const uint8_t* text_in, int64_t n, int32_t last, int32_t reverse, int32_t long_read, uint64_t entry_base,
                uint64_t* acc, uint64_t* out, uint64_t* len_hist, int64_t len_cap, uint64_t* cyc, uint32_t* lines)
{
	const int64_t blocks = (n + FQ_BLOCK - 1) / FQ_BLOCK;
	std::vector<uint8_t> text((size_t)(blocks ? blocks : 1) * FQ_BLOCK, 0xA);   // the padding holds newlines: the mask must take them off
	if (n) memcpy(text.data(), text_in, (size_t)n);
	// pass 1: newlines per block
	auto lane_mask = [&](int64_t blk, uint32_t t) {
		const uint64_t pos = (uint64_t)blk * FQ_BLOCK + t * 16u; uint32_t w[4]; memcpy(w, text.data() + pos, 16);
		return fq_mask_in_range(fq_newline_mask16(w[0], w[1], w[2], w[3]), pos, (uint64_t)n); };
	std::vector<uint64_t> base((size_t)blocks + 1, 0);
	for (int64_t b = 0; b < blocks; ++b) { uint32_t c = 0; for (uint32_t t = 0; t < 256; ++t) c += (uint32_t)__builtin_popcount(lane_mask(b, t)); base[(size_t)b + 1] = base[(size_t)b] + c; }
	// pass 2: the start of every line
	lines[0] = 0;
	for (int64_t b = 0; b < blocks; ++b)
	{
		uint64_t rank = base[(size_t)b];
		for (uint32_t t = 0; t < 256; ++t)
		{
			uint32_t m = lane_mask(b, t); const uint64_t pos = (uint64_t)b * FQ_BLOCK + t * 16u;
			while (m) { const uint32_t k = (uint32_t)__builtin_ctz(m); m &= m - 1; lines[rank + 1] = (uint32_t)(pos + k + 1); ++rank; }
		}
	}
	const uint64_t L = base[(size_t)blocks], E = last ? (L + 3) / 4 : L / 4;
	out[0] = L; out[1] = E; out[2] = 4 * E <= L ? lines[4 * E] : (uint64_t)n; out[3] = FQ_NO_ERROR; out[4] = 0; out[5] = 0;
	// entries: a wave each
	const uint8_t* tx = text.data();
	for (uint64_t r = 0; r < E; ++r)
	{
		const FqEntry e = fq_entry(tx, lines, L, r);
		const uint32_t kind = fq_entry_kind(tx, e);
		if (kind) { const unsigned long long w = fq_error_word(entry_base + r, kind); if (w < out[3]) out[3] = w; continue; }
		const bool header_empty = e.header.len == 0;
		if (!header_empty) ++out[4];
		const uint32_t cycles = e.bases.len;
		++acc[reverse ? 1 : 0]; acc[2] += cycles; if (cycles > out[5]) out[5] = cycles;
		if ((int64_t)cycles <= len_cap) ++len_hist[cycles];
		const uint8_t* b = tx + e.bases.start; const uint8_t* q = tx + e.quals.start;
		uint64_t wsum = 0; bool bb = false, bq = false;
		for (uint32_t lane = 0; lane < 64; ++lane)
		{
			uint32_t qsum = 0;
			for (uint32_t i = lane; i < cycles; i += 64)
			{
				const FqChar c = fq_char(b[i], q[i], long_read);
				if (c.cls < 5) { ++acc[3 + c.cls]; if (i < 320) ++cyc[7 * i + c.cls]; }
				bb |= c.cls == 5; bq |= !c.ok;
				qsum += c.q; if (i < 320) cyc[7 * i + (reverse ? 6 : 5)] += c.q;
				++acc[8 + c.q];
			}
			wsum += qsum;
		}
		const uint32_t ckind = fq_char_kind(header_empty, bb, bq);
		if (ckind) { const unsigned long long w = fq_error_word(entry_base + r, ckind); if (w < out[3]) out[3] = w; }
		if (cycles > 0)
		{
			int rq, qd; fq_mean_bins(wsum, cycles, rq, qd);
			if (rq >= 0) ++acc[108 + rq];
			++acc[208 + (reverse ? 60 : 0) + qd];
		}
	}
}
}
