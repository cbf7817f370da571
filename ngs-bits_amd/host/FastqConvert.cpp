// FastqConvert - drop-in for src/FastqConvert/main.cpp on the MI355X path: same flags, defaults, help text and output text. Every quality byte gets -31 in byte
// arithmetic (:36-39) while the GPU formats the output (ngsqc_fqedit_feed: csrc/fqedit.hip, NGSQC_FQEDIT_CONVERT); a quality ')' becomes a line feed, as in the
// reference. The input is inflated here.
#include "FastqEdit.hpp"
using namespace ngsbits;

class ConcreteTool : public ToolBase
{
public:
	ConcreteTool(int argc, char** argv) : ToolBase(argc, argv) {}
	void setup() override
	{
		setDescription("Converts the quality scores from Illumina 1.5 offset to Sanger/Illumina 1.8 offset.");
		addInfile("in", "Input gzipped FASTQ file.", false);
		addOutfile("out", "Output gzipped FASTQ file.", false);
		// optional
		addInt("compression_level", "Output FASTQ compression level from 1 (fastest) to 9 (best compression).", true, 1);
		// --changelog (src/FastqConvert/main.cpp)
		changeLog(2020, 7, 15, "Added 'compression_level' parameter.");
	}
	void main() override
	{
		FastqEditRun r;
		r.params.op = NGSQC_FQEDIT_CONVERT;
		r.in1 = getInfile("in"); r.out1 = getOutfile("out"); r.compression_level = getInt("compression_level");
		stamp("arguments");
		runFastqEdit(r, "FastqConvert");
	}
};
int main(int argc, char** argv) { ConcreteTool tool(argc, argv); return tool.execute(); }
