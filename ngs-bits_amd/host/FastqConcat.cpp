// FastqConcat - drop-in for src/FastqConcat/main.cpp on the MI355X path: same flags, defaults, help text and output text. The loop of main() (:40-51) runs on
// the GPU (ngsqc_fqedit_feed3: csrc/fqedit.hip, NGSQC_FQEDIT_COPY): the identity plan over the files one after the other, every file ending inside the one
// accumulator, the output deflated on the device. -long_read is accepted: the reference's streams do not validate here, so it changes nothing.
#include "FastqEdit.hpp"
using namespace ngsbits;

class ConcreteTool : public ToolBase
{
public:
	ConcreteTool(int argc, char** argv) : ToolBase(argc, argv) {}
	void setup() override
	{
		setDescription("Concatinates several FASTQ files into one output FASTQ file.");
		addInfileList("in", "Input (gzipped) FASTQ files.", false);
		addOutfile("out", "Output gzipped FASTQ file.", false);
		// optional
		addInt("compression_level", "Output FASTQ compression level from 1 (fastest) to 9 (best compression).", true, 1);
		addFlag("long_read", "Support long reads (> 1kb).");
		// --changelog (src/FastqConcat/main.cpp)
		changeLog(2023, 6, 15, "Added support for long reads.");
		changeLog(2020, 7, 15, "Added 'compression_level' parameter.");
		changeLog(2019, 4, 8, "Initial version of this tool");
	}
	void main() override
	{
		FastqEditRun r;
		r.params.op = NGSQC_FQEDIT_COPY; r.params.long_read = getFlag("long_read") ? 1 : 0;
		r.list1 = getInfileList("in"); r.out1 = getOutfile("out"); r.compression_level = getInt("compression_level");
		stamp("arguments");
		runFastqEdit(r, "FastqConcat");
	}
};
int main(int argc, char** argv) { ConcreteTool tool(argc, argv); return tool.execute(); }
