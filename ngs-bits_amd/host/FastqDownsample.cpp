// FastqDownsample - drop-in for src/FastqDownsample/main.cpp on the MI355X path: same flags, help text and output. The loop of main() (:58-71: one rand() per
// read pair, in file order) runs on the GPU (ngsqc_fqedit_feed3: csrc/fqedit.hip, NGSQC_FQEDIT_DOWNSAMPLE): the decisions come from glibc's rand() stream
// restated on the device (csrc/downsample.hip), the plan kernel reads the decision of every pair, and with -test the headers of the kept pairs are gathered on
// the device. The check that both files ended (:74-81) uses the entries the library saw on each side.
#include "FastqEdit.hpp"
#include <chrono>
using namespace ngsbits;

class ConcreteTool : public ToolBase
{
public:
	ConcreteTool(int argc, char** argv) : ToolBase(argc, argv) {}
	void setup() override
	{
		setDescription("Downsamples paired-end FASTQ files.");
		addInfile("in1", "Forward input gzipped FASTQ file(s).", false);
		addInfile("in2", "Reverse input gzipped FASTQ file(s).", false);
		addFloat("percentage", "Percentage of reads to keep.", false);
		addOutfile("out1", "Forward output gzipped FASTQ file.", false);
		addOutfile("out2", "Reverse output gzipped FASTQ file.", false);
		// optional
		addFlag("test", "Test mode: fix random number generator seed and write kept read names to STDOUT.");
		addInt("compression_level", "Output FASTQ compression level from 1 (fastest) to 9 (best compression).", true, 1);
		// --changelog (src/FastqDownsample/main.cpp)
		changeLog(2020, 7, 15, "Initial version of this tool.");
	}
	void main() override
	{
		FastqEditRun r;
		r.params.op = NGSQC_FQEDIT_DOWNSAMPLE;
		r.in1 = getInfile("in1"); r.in2 = getInfile("in2"); r.out1 = getOutfile("out1"); r.out2 = getOutfile("out2");
		r.percentage = getFloat("percentage");
		if (r.percentage <= 0 || r.percentage >= 100) { char b[64]; snprintf(b, sizeof(b), "%g", r.percentage); NB_THROW(CommandLineParsingException, std::string("Invalid percentage ") + b + "!"); }   // (QString::number(double): 'g', 6 digits)
		const bool test = getFlag("test");
		r.compression_level = getInt("compression_level");
		// srand(test ? 1 : QTime::currentTime().msec()) (:51): the milliseconds of the current second, 0 .. 999
		r.seed = test ? 1u : (uint32_t)(std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::system_clock::now().time_since_epoch()).count() % 1000);
		r.want_headers = test;
		stamp("arguments");
		FastqEditExtra x;
		const ngsqc_fqedit_stats st = runFastqEdit(r, "FastqDownsample", &x);
		// "KEPT PAIR: header" while the pairs are read (:69), then the check of the ends (:74-81), then the counts (:84-85)
		for (size_t at = 0; at < x.kept_headers.size(); )
		{
			const size_t e = x.kept_headers.find('\n', at);
			if (e == std::string::npos) break;
			printf("KEPT PAIR: %.*s\n", (int)(e - at), x.kept_headers.data() + at);
			at = e + 1;
		}
		fflush(stdout);
		if (x.side_entries[0] > x.side_entries[1]) NB_THROW(FileParseException, "File " + r.in1 + " has more entries than " + r.in2 + "!");
		if (x.side_entries[1] > x.side_entries[0]) NB_THROW(FileParseException, "File " + r.in2 + " has more entries than " + r.in1 + "!");
		printf("PE reads read   : %lld\n", (long long)st.entries);
		printf("PE reads written: %lld\n", (long long)st.written[0]);
	}
};
int main(int argc, char** argv) { ConcreteTool tool(argc, argv); return tool.execute(); }
