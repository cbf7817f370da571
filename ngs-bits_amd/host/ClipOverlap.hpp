// What BamClipOverlap prints behind its pass (src/BamClipOverlap/main.cpp:549-553), shared by the tool and the C entry of the tests (hostapi.cpp).
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>

namespace ngsbits {

// QString::number(x, 'f', 2)
inline std::string clipPercent(double x)
{
	if (std::isnan(x)) return "nan";
	if (std::isinf(x)) return x < 0 ? "-inf" : "inf";
	char b[64]; snprintf(b, sizeof(b), "%.2f", x);
	return b;
}

// counts: reads, saved, clipped, mismatch, bases, bases clipped (ngsqc_clip_overlap). The reference counts the first four in `int`. lost: the message of the
// "Lost Reads" check (:550), empty when every read was saved.
inline std::string clipSummary(const int64_t* counts, std::string& lost)
{
	const int reads = (int)counts[0], saved = (int)counts[1], clipped = (int)counts[2], mismatch = (int)counts[3];
	const unsigned long long bases = (unsigned long long)counts[4], bases_clipped = (unsigned long long)counts[5];
	lost.clear();
	if (saved != reads) { lost = "Lost Reads: " + std::to_string(reads - saved) + "/" + std::to_string(reads); return ""; }
	std::string s;
	s += "Overlap mismatch filtering was used for " + std::to_string(mismatch) + " of " + std::to_string(reads) + " reads (" + clipPercent((double)mismatch / (double)reads * 100) + " %).\n";
	s += "Softclipped " + std::to_string(clipped) + " of " + std::to_string(reads) + " reads (" + clipPercent((double)clipped / (double)reads * 100) + " %).\n";
	s += "Softclipped " + std::to_string(bases_clipped) + " of " + std::to_string(bases) + " basepairs (" + clipPercent((double)bases_clipped / (double)bases * 100) + " %).\n";
	return s;
}

} // namespace ngsbits
