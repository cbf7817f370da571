// FastqExtractUMI - drop-in for src/FastqExtractUMI/main.cpp on the MI355X path: same flags, defaults, help text and output text. The loop of main() (:48-74)
// runs on the GPU (ngsqc_fqedit_feed: csrc/fqedit.hip, NGSQC_FQEDIT_UMI): the UMI bases are cut from both reads and the format kernel composes the text that
// goes into both headers from the two reads. The two inputs are inflated here, in step; the run ends silently at the shorter one.
#include "FastqEdit.hpp"
using namespace ngsbits;

class ConcreteTool : public ToolBase
{
public:
	ConcreteTool(int argc, char** argv) : ToolBase(argc, argv) {}
	void setup() override
	{
		setDescription("Cuts UMI bases from the beginning of reads and adds them to read headers.");
		addInfile("in1", "Input FASTQ file 1.", false);
		addInfile("in2", "Input FASTQ file 2.", false);
		addOutfile("out1", "Output filename for read 1 FASTQ.", false);
		addOutfile("out2", "Output filename for read 2 FASTQ.", false);
		// optional
		addInt("cut1", "Number of bases from the head of read 1 to use as UMI.", true, 0);
		addInt("cut2", "Number of bases from the head of read 2 to use as UMI.", true, 0);
		addInt("compression_level", "Output FASTQ compression level from 1 (fastest) to 9 (best compression).", true, 1);
		// --changelog (src/FastqExtractUMI/main.cpp)
		changeLog(2020, 7, 15, "Added 'compression_level' parameter.");
	}
	void main() override
	{
		FastqEditRun r;
		r.params.op = NGSQC_FQEDIT_UMI; r.params.cut1 = getInt("cut1"); r.params.cut2 = getInt("cut2");
		r.in1 = getInfile("in1"); r.in2 = getInfile("in2"); r.out1 = getOutfile("out1"); r.out2 = getOutfile("out2"); r.compression_level = getInt("compression_level");
		stamp("arguments");
		runFastqEdit(r, "FastqExtractUMI");
	}
};
int main(int argc, char** argv) { ConcreteTool tool(argc, argv); return tool.execute(); }
