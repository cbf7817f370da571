// BamDownsample - drop-in for src/BamDownsample/main.cpp:18-101 on the MI355X path: same flags, help text and output. The loop of main() (:55-93: the mate cache
// by read name, one rand() per single-end record and per closed pair, BamWriter::writeAlignment) runs as one pass over the BAM on the GPU, the decisions come
// from glibc's rand() stream restated on the device, and the BGZF writer deflates on the GPU as well (ngsqc_downsample: csrc/downsample.hip, csrc/deflate.hip).
#include "Statistics.hpp"
#include <chrono>
using namespace ngsbits;

static bool ends_with(const std::string& s, const std::string& e) { return s.size() >= e.size() && s.compare(s.size() - e.size(), e.size(), e) == 0; }

class ConcreteTool : public ToolBase
{
public:
	ConcreteTool(int argc, char** argv) : ToolBase(argc, argv) {}
	void setup() override
	{
		setDescription("Downsamples a BAM file to the given percentage of reads.");
		addInfile("in", "Input BAM/CRAM file.", false);
		addFloat("percentage", "Percentage of reads to keep.", false);
		addOutfile("out", "Output BAM/CRAM file.", false);
		addFlag("test", "Test mode: fix random number generator seed and write kept read names to STDOUT.");
		addInfile("ref", "Reference genome for CRAM support (mandatory if CRAM is used).", true);
		// --changelog (src/BamDownsample/main.cpp)
		changeLog(2020, 11, 27, "Added CRAM support.");
	}
	void main() override
	{
		const bool test = getFlag("test");
		// srand(test ? 1 : QTime::currentTime().msec()) (:36): the milliseconds of the current second, 0 .. 999
		const uint32_t seed = test ? 1u : (uint32_t)(std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::system_clock::now().time_since_epoch()).count() % 1000);
		const double percentage = getFloat("percentage");
		if (percentage <= 0 || percentage >= 100) { char b[64]; snprintf(b, sizeof(b), "%g", percentage); NB_THROW(CommandLineParsingException, std::string("Invalid percentage ") + b + "!"); }   // (QString::number(double): 'g', 6 digits)
		const std::string out = getOutfile("out");
		// BamWriter::BamWriter (src/cppNGS/BamWriter.cpp:9-30), checked before a device is opened
		if (ends_with(out, ".cram")) NB_THROW(FileAccessException, "CRAM output is not supported: " + out + ". Write a '.bam' file.");
		if (!ends_with(out, ".bam")) NB_THROW(FileAccessException, "Could not write file: " + out + ". File extension has to be '.bam' or '.cram'.");
		stamp("arguments");
		BamReader reader(getInfile("in"), getInfile("ref"));
		stamp("open");
		ngsqc_downsample_params p{percentage, seed, test ? 1 : 0};
		ngsqc_downsample_counts c{0, 0, 0, 0, 0};
		char* names = nullptr;
		reader.check(ngsqc_downsample(reader.handle(), &p, out.c_str(), &c, &names));
		stamp("join, decide, gather, deflate and write");
		// "KEPT SE: name" / "KEPT PE: name" in the order of the deciding records (:67, :85), from the library's "SE\tname\n" / "PE\tname\n" lines
		for (const char* q = names; q && *q; )
		{
			const char* e = strchr(q, '\n');
			if (!e) break;
			printf("KEPT %.2s: %.*s\n", q, (int)(e - q - 3), q + 3);
			q = e + 1;
		}
		free(names);
		printf("SE reads                    : %lld\n", (long long)c.se);
		printf("SE reads (written)          : %lld\n", (long long)c.se_written);
		printf("PE reads                    : %lld\n", (long long)c.pe);
		printf("PE reads (written)          : %lld\n", (long long)c.pe_written);
		printf("PE reads unmatched (skipped): %lld\n", (long long)c.pe_unmatched);
	}
};
int main(int argc, char** argv) { ConcreteTool tool(argc, argv); return tool.execute(); }
