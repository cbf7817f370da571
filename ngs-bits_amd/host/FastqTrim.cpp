// FastqTrim - drop-in for src/FastqTrim/main.cpp on the MI355X path: same flags, defaults, help text and output text. The loop of main() (:47-73) is a plan
// record per entry on the GPU (ngsqc_fqedit_feed: csrc/fqedit.hip, NGSQC_FQEDIT_TRIM), which also formats and deflates the output; the input is inflated here.
#include "FastqEdit.hpp"
using namespace ngsbits;

class ConcreteTool : public ToolBase
{
public:
	ConcreteTool(int argc, char** argv) : ToolBase(argc, argv) {}
	void setup() override
	{
		setDescription("Trims start/end bases from all reads in a FASTQ file.");
		addInfile("in", "Input gzipped FASTQ file.", false);
		addOutfile("out", "Output gzipped FASTQ file.", false);
		// optional
		addInt("start", "Trim this number of bases from the start of the read.", true, 0);
		addInt("end", "Trim this number of bases from the end of the read.", true, 0);
		addInt("len", "Restrict read length to this value (after trimming from start/end).", true, 0);
		addInt("max_len", "Only trim reads smaller than the given length. Used e.g. to remove UMIs at the read end from read-throughs.", true, 0);
		addInt("compression_level", "Output FASTQ compression level from 1 (fastest) to 9 (best compression).", true, 1);
		addFlag("long_read", "Support long reads (> 1kb).");
		// --changelog (src/FastqTrim/main.cpp)
		changeLog(2023, 6, 15, "Added support for long reads.");
		changeLog(2020, 7, 15, "Added 'compression_level' parameter.");
		changeLog(2016, 8, 26, "Added 'len' parameter.");
	}
	void main() override
	{
		FastqEditRun r;
		r.params.op = NGSQC_FQEDIT_TRIM; r.params.long_read = getFlag("long_read") ? 1 : 0;
		r.params.start = getInt("start"); r.params.end = getInt("end"); r.params.len = getInt("len"); r.params.max_len = getInt("max_len");
		r.in1 = getInfile("in"); r.out1 = getOutfile("out"); r.compression_level = getInt("compression_level");
		stamp("arguments");
		runFastqEdit(r, "FastqTrim");
	}
};
int main(int argc, char** argv) { ConcreteTool tool(argc, argv); return tool.execute(); }
