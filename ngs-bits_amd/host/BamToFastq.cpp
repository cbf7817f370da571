// BamToFastq - drop-in for src/BamToFastq/main.cpp on the MI355X path: same flags, defaults, help text, messages and report. The loop of main() (:135-196: the
// mate cache by read name, -fix, -remove_duplicates, alignmentToFastq) runs as one pass over the BAM on the GPU, and both FASTQ.GZ files are deflated on the
// GPU as well (ngsqc_bam_to_fastq: csrc/fastq.hip, csrc/join.h, csrc/deflate.hip). The files are BGZF (valid gzip); their decompressed text is the reference's.
#include "Statistics.hpp"
#include <regex>
using namespace ngsbits;

// Helper::toInt: the whole (trimmed) text is a decimal int
static bool to_int(const std::string& t, int& v)
{
	const std::string s = trimmed(t);
	if (!std::regex_match(s, std::regex("[+-]?[0-9]+"))) return false;
	try { const long long x = std::stoll(s); if (x < INT32_MIN || x > INT32_MAX) return false; v = (int)x; return true; }
	catch (...) { return false; }
}

// BedLine::fromString (src/cppNGS/BedFile.cpp:37-70): ':' and '-' become tabs, runs of spaces a tab, ',' is dropped from the numbers; invalid: a default BedLine
static BedLine bedline_from_string(std::string s)
{
	for (char& c : s) if (c == ':' || c == '-') c = '\t';
	s = std::regex_replace(s, std::regex("[ ]+"), "\t");
	std::vector<std::string> parts;
	size_t b = 0;
	for (size_t i = 0; i <= s.size(); ++i) if (i == s.size() || s[i] == '\t') { parts.push_back(s.substr(b, i - b)); b = i + 1; }
	if (parts.size() < 3) return BedLine(Chromosome(), 0, -1);
	for (int k = 1; k <= 2; ++k) parts[(size_t)k].erase(std::remove(parts[(size_t)k].begin(), parts[(size_t)k].end(), ','), parts[(size_t)k].end());
	int start = 0, end = 0;
	if (!to_int(parts[1], start) || !to_int(parts[2], end)) return BedLine(Chromosome(), 0, -1);
	return BedLine(Chromosome(parts[0]), start, end);
}
static bool bedline_valid(const BedLine& l) { return l.chr().isValid() && l.start() >= 0 && l.start() <= l.end(); }

class ConcreteTool : public ToolBase
{
public:
	ConcreteTool(int argc, char** argv) : ToolBase(argc, argv) {}
	void setup() override
	{
		setDescription("Converts a coordinate-sorted BAM file to FASTQ files.");
		addInfile("in", "Input BAM/CRAM file.", false, true);
		addOutfile("out1", "Read 1 output FASTQ.GZ file.", false);
		// optional
		addOutfile("out2", "Read 2 output FASTQ.GZ file (required for pair-end samples).", true);
		addString("reg", "Export only reads in the given region. Format: chr:start-end.", true);
		addFlag("remove_duplicates", "Does not export reads marked as duplicates in SAM flags into the FASTQ file.");
		addInt("compression_level", "Output FASTQ compression level from 1 (fastest) to 9 (best compression).", true, 1);
		addInt("write_buffer_size", "Output write buffer size (number of FASTQ entry pairs).", true, 100);
		addInfile("ref", "Reference genome for CRAM support (mandatory if CRAM is used).", true);
		addInt("extend", "Extend all reads to the given length. Base 'N' and base qualiy '2' are used for extension.", true, 0);
		addFlag("fix", "Keep only one read pair if several have the same name (note: needs much memory as read names are kept in memory).");
		// --changelog (src/BamToFastq/main.cpp)
		changeLog(2024, 12, 13, "Added 'fix' parameter.");
		changeLog(2024, 12, 9, "Added 'extend' parameter.");
		changeLog(2020, 11, 27, "Added CRAM support.");
		changeLog(2020, 5, 29, "Massive speed-up by writing in background. Added 'compression_level' parameter.");
		changeLog(2020, 3, 21, "Added 'reg' parameter.");
		changeLog(2023, 3, 22, "Added mode for single-end samples (long reads).");
	}
	void main() override
	{
		const double t_start = now_s();
		const std::string out1 = getOutfile("out1"), out2 = getOutfile("out2"), reg = getString("reg");
		const bool fix = getFlag("fix"), remove_duplicates = getFlag("remove_duplicates");
		const int compression_level = getInt("compression_level"), extend = getInt("extend");
		(void)getInt("write_buffer_size");   // (the size of the reference's hand-over queue: it does not change the output)
		const bool is_pe = !trimmed(out2).empty();
		// checked before a device is opened
		BedLine region;
		if (reg != "")
		{
			region = bedline_from_string(reg);
			if (!bedline_valid(region)) NB_THROW(CommandLineParsingException, "Given region '" + reg + "' is not valid!");
		}
		// FastqOutfileStream::FastqOutfileStream (src/cppNGS/FastqFileStream.cpp:160-172), out1 first
		if (compression_level < 0 || compression_level > 9)
			NB_THROW(ArgumentException, "Invalid gzip compression level '" + std::to_string(compression_level) + "' given for FASTQ file '" + out1 + "'!");
		stamp("arguments");
		ngsqc_fastq_params p{remove_duplicates ? 1 : 0, fix ? 1 : 0, extend, compression_level, -1, 0, 0};
		std::unique_ptr<BamReader> reader;
		if (reg != "")
		{
			// BamReader::setRegion (BamReader.cpp:734-768): only the BGZF blocks the index names for the region are sent to the GPU
			reader.reset(new BamReader(getInfile("in"), getInfile("ref"), false, BedFile(region.chr(), region.start(), region.end())));
			const int tid = reader->chromosomeID(region.chr());
			if (tid < 0) NB_THROW(ArgumentException, "Chromosome '" + region.chr().str() + "' not known in BAM/CRAM file " + getInfile("in"));
			p.reg_tid = tid; p.reg_start = region.start(); p.reg_end = region.end();
		}
		else reader.reset(new BamReader(getInfile("in"), getInfile("ref")));
		stamp("open");
		ngsqc_fastq_counts c{};
		const int rc = ngsqc_bam_to_fastq(reader->handle(), &p, out1.c_str(), is_pe ? out2.c_str() : nullptr, &c);
		if (rc == NGSQC_E_FORMAT)
		{
			const std::string msg = ngsqc_last_error(reader->handle());
			if (msg.rfind("Could not convert base", 0) == 0) NB_THROW(ProgrammingException, msg);   // (Sequence::complement)
		}
		if (rc == NGSQC_E_IO) NB_THROW(FileAccessException, ngsqc_last_error(reader->handle()));
		reader->check(rc);
		stamp("join, format, deflate and write");
		if (is_pe)
		{
			printf("Pair reads (written)            : %lld\n", (long long)c.paired);
			printf("Unpaired reads (skipped)        : %lld\n", (long long)c.unpaired);
			printf("Unmatched paired reads (skipped): %lld\n", (long long)c.unmatched);
		}
		else printf("Reads (written)                 : %lld\n", (long long)c.single_end);
		if (remove_duplicates) printf("Duplicate tagged reads (skipped): %lld\n", (long long)c.duplicates);
		if (fix) printf("Duplicate name reads (skipped)  : %lld\n", (long long)c.fixed);
		printf("\n");
		printf("Maximum cached reads            : %lld\n", (long long)c.max_cached);
		const double el = now_s() - t_start;
		printf("Time elapsed                    : %.0fm %.0fs %.0fms\n", std::floor(el / 60), std::floor(std::fmod(el, 60.0)), std::floor(std::fmod(el * 1000.0, 1000.0)));
	}
};
int main(int argc, char** argv) { ConcreteTool tool(argc, argv); return tool.execute(); }
