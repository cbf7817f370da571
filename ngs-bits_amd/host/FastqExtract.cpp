// FastqExtract - drop-in for src/FastqExtract/main.cpp on the MI355X path: same flags, defaults, help text, messages and output text. The id list (:39-52) is
// read here and goes into a table in device memory (ngsqc_fqedit_ids); the loop of main() (:61-90) - validation, the id of every header, the lookup and the cut to
// the listed length - runs on the GPU (ngsqc_fqedit_feed: csrc/fqedit.hip, NGSQC_FQEDIT_EXTRACT), which also formats and deflates the output.
#include "FastqEdit.hpp"
#include <regex>
using namespace ngsbits;

// Helper::toInt (cppCORE, which is not part of the reference tree; the message as its public source has it): the whole trimmed text is a decimal int
static int to_int(const std::string& t, const std::string& name)
{
	const std::string s = trimmed(t);
	bool ok = std::regex_match(s, std::regex("[+-]?[0-9]+"));
	long long x = 0;
	if (ok) { try { x = std::stoll(s); } catch (...) { ok = false; } }
	if (!ok || x < INT32_MIN || x > INT32_MAX) NB_THROW(ArgumentException, "Could not convert " + name + " '" + t + "' to integer");
	return (int)x;
}

class ConcreteTool : public ToolBase
{
public:
	ConcreteTool(int argc, char** argv) : ToolBase(argc, argv) {}
	void setup() override
	{
		setDescription("Extracts reads from a FASTQ file according to an ID list. Trims the reads if lengths are given.");
		addInfile("in", "Input FASTQ file (gzipped or plain).", false);
		addInfile("ids", "Input TSV file containing IDs (without the '@') in the first column and optional length in the second column.", false);
		addOutfile("out", "Output FASTQ file.", false);
		// optional
		addFlag("v", "Invert match: keep non-matching reads.");
		addInt("compression_level", "Output FASTQ compression level from 1 (fastest) to 9 (best compression).", true, 1);
		addFlag("long_read", "Support long reads (> 1kb).");
		// --changelog (src/FastqExtract/main.cpp)
		changeLog(2023, 4, 18, "Added support for long reads.");
		changeLog(2020, 7, 15, "Added 'compression_level' parameter.");
	}
	void main() override
	{
		FastqEditRun r;
		r.params.op = NGSQC_FQEDIT_EXTRACT; r.params.long_read = getFlag("long_read") ? 1 : 0; r.params.invert = getFlag("v") ? 1 : 0;
		// the ids and lengths, in file order: a later duplicate replaces the earlier one in the library, as QHash::insert does
		std::ifstream f(getInfile("ids"), std::ios::binary);
		if (!f) NB_THROW(FileAccessException, "Could not open file for reading: '" + getInfile("ids") + "'!");
		std::string line;
		while (std::getline(f, line))
		{
			line = trimmed(line);
			if (line.empty() || line[0] == '#') continue;
			const std::vector<std::string> parts = split(line, '\t');
			r.ids.push_back(parts[0]);
			r.id_lengths.push_back(parts.size() > 1 ? to_int(parts[1], "length value") : -1);
		}
		r.in1 = getInfile("in"); r.out1 = getOutfile("out"); r.compression_level = getInt("compression_level");
		stamp("arguments and ids");
		runFastqEdit(r, "FastqExtract");
	}
};
int main(int argc, char** argv) { ConcreteTool tool(argc, argv); return tool.execute(); }
