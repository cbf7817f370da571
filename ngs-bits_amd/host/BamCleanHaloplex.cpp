// BamCleanHaloplex - drop-in for src/BamCleanHaloplex/main.cpp:15-69 on the MI355X path: same flags, default, help text and output. The loop of main() (:41-62:
// the candidate test, the sum of the CIGAR's M lengths, setIsUnmapped / setIsSecondaryAlignment on a read below -min_match, BamWriter::writeAlignment for every
// read) runs as one pass over the BAM on the GPU, and the BGZF writer deflates on the GPU as well (ngsqc_clean_haloplex: csrc/haloplex.hip, csrc/deflate.hip).
// The reference counts its reads in `int`; the counts here are 64-bit.
#include "Statistics.hpp"
using namespace ngsbits;

static bool ends_with(const std::string& s, const std::string& e) { return s.size() >= e.size() && s.compare(s.size() - e.size(), e.size(), e) == 0; }

// BamWriter::BamWriter (src/cppNGS/BamWriter.cpp:9-30), checked before a device is opened
static void check_bam_output(const std::string& out)
{
	if (ends_with(out, ".cram")) NB_THROW(FileAccessException, "CRAM output is not supported: " + out + ". Write a '.bam' file.");
	if (!ends_with(out, ".bam")) NB_THROW(FileAccessException, "Could not write file: " + out + ". File extension has to be '.bam' or '.cram'.");
}

// QString::number(100.0 * x / n, 'f', 2) (:67-68): without reads the quotient is not a number, which Qt prints as "nan" whatever its sign
static std::string percent(int64_t x, int64_t n)
{
	if (n == 0) return "nan";
	char b[64];
	snprintf(b, sizeof(b), "%.2f", 100.0 * (double)x / (double)n);
	return b;
}

class ConcreteTool : public ToolBase
{
public:
	ConcreteTool(int argc, char** argv) : ToolBase(argc, argv) {}
	void setup() override
	{
		setDescription("BAM cleaning for Haloplex.");
		addInfile("in", "Input BAM/CRAM file.", false);
		addOutfile("out", "Output BAM/CRAM file.", false);
		addInt("min_match", "Minimum number of CIGAR matches (M).", true, 30);
		addInfile("ref", "Reference genome for CRAM support (mandatory if CRAM is used).", true);
		// --changelog (src/BamCleanHaloplex/main.cpp)
		changeLog(2020, 11, 27, "Added CRAM support.");
	}
	void main() override
	{
		const std::string out = getOutfile("out");
		check_bam_output(out);
		const int min_match = getInt("min_match");
		stamp("arguments");
		ngsqc_set_cram_skip(0);   // (every record is written whole: a CRAM input is decoded with its read names and tags, which the QC tools' default leaves out)
		BamReader reader(getInfile("in"), getInfile("ref"));
		stamp("open");
		ngsqc_haloplex_counts c{0, 0, 0};
		reader.check(ngsqc_clean_haloplex(reader.handle(), min_match, out.c_str(), &c));
		stamp("verdicts, gather, deflate and write");
		printf("overall reads: %lld\n", (long long)c.reads);
		printf("mapped reads : %lld (%s%%)\n", (long long)c.candidates, percent(c.candidates, c.reads).c_str());
		printf("removed reads: %lld (%s%%)\n", (long long)c.failed, percent(c.failed, c.reads).c_str());
	}
};
int main(int argc, char** argv) { ConcreteTool tool(argc, argv); return tool.execute(); }
