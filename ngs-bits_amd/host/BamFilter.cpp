// BamFilter - drop-in for src/BamFilter/main.cpp:11-134 on the MI355X path: same flags, defaults, help text and output. The loop of main() (:88-129: the mate
// cache by read name, alignment_pass, BamWriter::writeAlignment) runs as one pass over the BAM on the GPU, and the BGZF writer deflates on the GPU as well
// (ngsqc_filter_pairs: csrc/pairs.hip, csrc/deflate.hip).
#include "Statistics.hpp"
using namespace ngsbits;

static bool ends_with(const std::string& s, const std::string& e) { return s.size() >= e.size() && s.compare(s.size() - e.size(), e.size(), e) == 0; }

class ConcreteTool : public ToolBase
{
public:
	ConcreteTool(int argc, char** argv) : ToolBase(argc, argv) {}
	void setup() override
	{
		setDescription("Filter alignments in BAM/CRAM file (no input sorting required).");
		addInfile("in", "Input BAM/CRAM file.", false);
		addOutfile("out", "Output BAM/CRAM file.", false);
		addInt("minMQ", "Minimum mapping quality.", true, 30);
		addInt("maxMQ", "Maximium mapping quality.", true, 256);
		addInt("maxMM", "Maximum number of mismatches in aligned read, -1 to disable.", true, 4);
		addInt("maxGap", "Maximum number of gaps (indels) in aligned read, -1 to disable.", true, 1);
		addInt("minDup", "Minimum number of duplicates.", true, 0);
		addInt("maxIS", "Maximum insert size, -1 to disable.", true, -1);
		addInfile("ref", "Reference genome for CRAM support (mandatory if CRAM is used).", true);
		addFlag("write_cram", "Writes a CRAM file as output.");
		// --changelog (src/BamFilter/main.cpp)
		changeLog(2020, 11, 27, "Added CRAM support.");
		changeLog(2024, 2, 15, "Added option to remove large fragments.");
		changeLog(2026, 7, 30, "Added option to filter by max. mapping quality.");
	}
	void main() override
	{
		// (-write_cram is accepted and ignored, as in the reference: the extension of -out decides)
		const std::string out = getOutfile("out");
		// BamWriter::BamWriter (src/cppNGS/BamWriter.cpp:9-30), checked before a device is opened
		if (ends_with(out, ".cram")) NB_THROW(FileAccessException, "CRAM output is not supported: " + out + ". Write a '.bam' file.");
		if (!ends_with(out, ".bam")) NB_THROW(FileAccessException, "Could not write file: " + out + ". File extension has to be '.bam' or '.cram'.");
		ngsqc_pair_filter p{getInt("minMQ"), getInt("maxMQ"), getInt("maxMM"), getInt("maxGap"), getInt("minDup"), getInt("maxIS")};
		stamp("arguments");
		BamReader reader(getInfile("in"), getInfile("ref"));
		stamp("open");
		int64_t passed = 0, dropped = 0;
		reader.check(ngsqc_filter_pairs(reader.handle(), &p, out.c_str(), &passed, &dropped));
		stamp("filter, gather, deflate and write");
		printf("pairs passed: %lld\npairs dropped: %lld\n", (long long)passed, (long long)dropped);
	}
};
int main(int argc, char** argv) { ConcreteTool tool(argc, argv); return tool.execute(); }
