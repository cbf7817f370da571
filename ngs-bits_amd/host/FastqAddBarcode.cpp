// FastqAddBarcode - drop-in for src/FastqAddBarcode/main.cpp on the MI355X path: same flags, defaults, help text and output text. The loop of main() (:44-73)
// runs on the GPU (ngsqc_fqedit_feed3: csrc/fqedit.hip, NGSQC_FQEDIT_BARCODE_ADD): the format kernel composes ":" length ",0:" bases "," from the barcode read
// in a third device text and splices it behind the first token of both headers. The three lists are processed triple by triple into one pair of outputs;
// every triple ends silently at its shortest file. Lists of different lengths, which the reference indexes past the end of, are refused.
#include "FastqEdit.hpp"
using namespace ngsbits;

class ConcreteTool : public ToolBase
{
public:
	ConcreteTool(int argc, char** argv) : ToolBase(argc, argv) {}
	void setup() override
	{
		setDescription("Adds barcodes from separate FASTQ file to read headers.");
		addInfileList("in1", "Input FASTQ file 1.", false);
		addInfileList("in2", "Input FASTQ file 2.", false);
		addInfileList("in_barcode", "Input barcode file.", false);
		addOutfile("out1", "Output filename for read 1 FASTQ.", false);
		addOutfile("out2", "Output filename for read 2 FASTQ.", false);
		// optional
		addInt("compression_level", "Output FASTQ compression level from 1 (fastest) to 9 (best compression).", true, 1);
		// --changelog (src/FastqAddBarcode/main.cpp)
		changeLog(2020, 7, 15, "Added 'compression_level' parameter.");
	}
	void main() override
	{
		FastqEditRun r;
		r.params.op = NGSQC_FQEDIT_BARCODE_ADD;
		r.out1 = getOutfile("out1"); r.out2 = getOutfile("out2"); r.compression_level = getInt("compression_level");
		r.list1 = getInfileList("in1"); r.list2 = getInfileList("in2"); r.list3 = getInfileList("in_barcode");
		if (r.list1.size() != r.list2.size() || r.list1.size() != r.list3.size())
			NB_THROW(ArgumentException, "The lists 'in1', 'in2' and 'in_barcode' must have the same number of files (" + std::to_string(r.list1.size()) + ", " + std::to_string(r.list2.size()) + " and " + std::to_string(r.list3.size()) + " given)!");
		stamp("arguments");
		runFastqEdit(r, "FastqAddBarcode");
	}
};
int main(int argc, char** argv) { ConcreteTool tool(argc, argv); return tool.execute(); }
