// FastqExtractBarcode - drop-in for src/FastqExtractBarcode/main.cpp on the MI355X path: same flags, defaults, help text and output text. The loop of main()
// (:44-60) runs on the GPU (ngsqc_fqedit_feed3: csrc/fqedit.hip, NGSQC_FQEDIT_BARCODE_CUT): two plan rows per entry of the one input, the main stream without
// the first cut bytes of the bases and quality lines, the index stream with those bytes. Where the reference's QByteArray(read1.bases, cut) reads behind a
// line shorter than the cut, the bytes that exist are taken.
#include "FastqEdit.hpp"
using namespace ngsbits;

class ConcreteTool : public ToolBase
{
public:
	ConcreteTool(int argc, char** argv) : ToolBase(argc, argv) {}
	void setup() override
	{
		setDescription("Cuts bases from the beginning of reads and stores them in an additional fastq.");
		addInfile("in", "input fastq file1.", false);
		addString("out_main", "output filename for main fastq.", false);
		addString("out_index", "output filename for index fastq.", true, "index.fastq.gz");
		// optional
		addInt("cut", "number of bases from the beginning of reads to use as barcodes.", true, 0);
		addInt("compression_level", "Output FASTQ compression level from 1 (fastest) to 9 (best compression).", true, 1);
		// --changelog (src/FastqExtractBarcode/main.cpp)
		changeLog(2020, 7, 15, "Added 'compression_level' parameter.");
	}
	void main() override
	{
		FastqEditRun r;
		r.params.op = NGSQC_FQEDIT_BARCODE_CUT; r.params.cut1 = getInt("cut");
		r.in1 = getInfile("in"); r.out1 = getString("out_main"); r.out2 = getString("out_index"); r.compression_level = getInt("compression_level");
		stamp("arguments");
		runFastqEdit(r, "FastqExtractBarcode");
	}
};
int main(int argc, char** argv) { ConcreteTool tool(argc, argv); return tool.execute(); }
