// The host's view of a FASTQ text that the device has indexed: where the text ends once the empty lines at its end are taken off, the four lines of an entry
// from the line offsets fetched from the device, and the message of FastqEntry::validate (src/cppNGS/FastqFileStream.cpp:3-44) for the entry the device named.
// The one copy for the three accumulators (ngsqc_fastq in fastqin.hip; ngsqc_purge and ngsqc_fqedit through fastq_feed.h). Free of HIP, as fastq_visit.h is:
// tests/emul/fastq_text_main.cpp runs it on the CPU under AddressSanitizer and UBSan.
#pragma once
#include "fastq_visit.h"
#include <string>
#include <vector>

namespace ngsqc {
// the end of the text once the empty lines at its end ("" or "\r") are taken off
inline size_t fq_strip_empty_lines(const uint8_t* t, size_t n)
{
	for (;;)
	{
		if (n >= 1 && t[n - 1] == '\n' && (n == 1 || t[n - 2] == '\n')) { n -= 1; continue; }
		if (n >= 2 && t[n - 1] == '\n' && t[n - 2] == '\r' && (n == 2 || t[n - 3] == '\n')) { n -= 2; continue; }
		return n;
	}
}

// Entry r of a text of n_lines lines is lines 4r .. 4r + 3; those at or behind n_lines (the missing lines of an incomplete last entry) are empty. The host
// fetches lines[j0 .. j1] of the device's index (fq_line of fastq_visit.h), j0 = 4r, j1 = min(4r + 4, n_lines): j1 - j0 + 1 offsets, one when j1 <= j0.
inline size_t fq_entry_offsets(uint64_t r, uint64_t n_lines)
{
	const uint64_t j0 = 4 * r, j1 = j0 + 4 < n_lines ? j0 + 4 : n_lines;
	return (size_t)(j1 > j0 ? j1 - j0 : 0) + 1;
}
// ... and the four lines from those offsets and the host's copy of the text, the '\n' and one '\r' in front of it left out as fq_line leaves them out
inline void fq_entry_lines(const uint8_t* text, const std::vector<uint32_t>& lo, std::string ln[4])
{
	for (size_t k = 0; k < 4; ++k)
	{
		ln[k].clear();
		if (k + 1 >= lo.size()) continue;
		size_t b = lo[k], e = lo[k + 1] - 1;   // the '\n'
		if (e > b && text[e - 1] == '\r') --e;
		ln[k].assign((const char*)text + b, e - b);
	}
}

// the text FastqEntry::validate throws for kind 1 .. 5 (FQ_ERR_HEADER .. FQ_ERR_QUALITY) on the entry of these four lines
inline std::string fq_validate_message(int kind, const std::string ln[4], int long_read)
{
	const std::string &header = ln[0], &bases = ln[1], &header2 = ln[2], &quals = ln[3];
	std::string m = "Invalid Fastq file entry: ";
	if (kind == FQ_ERR_HEADER) m += "First header line does not start with '@': '" + header + "'.";
	else if (kind == FQ_ERR_HEADER2) m += "Second header line does not start with '+': '" + header2 + "'.";
	else if (kind == FQ_ERR_LENGTH) m += "Differing length of bases (" + std::to_string(bases.size()) + ") and qualities string (" + std::to_string(bases.size()) + ") in sequence '" + header + "'.";   // (both numbers are the bases': :17)
	else if (kind == FQ_ERR_BASE)
	{
		char c = '?'; for (char x : bases) if (fq_base_class((uint8_t)x) == 5u) { c = x; break; }
		m += std::string("Invalid base '") + c + "' encountered in sequence '" + header + "'.";
	}
	else
	{
		char c = '?'; for (char x : quals) if (!fq_quality_ok((uint8_t)x, long_read)) { c = x; break; }
		m += std::string("Invalid ") + (long_read ? "nanopore " : "") + "quality character '" + c + "' with value '" + std::to_string((int)(signed char)c) + "' encountered in sequence '" + header + "'.";
	}
	return m;
}
} // namespace ngsqc
