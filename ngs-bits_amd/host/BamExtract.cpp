// BamExtract - drop-in for src/BamExtract/main.cpp:15-83 on the MI355X path: same flags, help text and output. The ID file is read here as the reference reads
// it (:35-44); the loop of main() (:63-76: the lookup of every alignment's name in the set, BamWriter::writeAlignment into one of two files) runs as one pass over
// the BAM on the GPU, with the set in device memory, and the BGZF writers deflate on the GPU as well (ngsqc_extract_reads: csrc/extract.hip, csrc/deflate.hip).
#include "Statistics.hpp"
using namespace ngsbits;

static bool ends_with(const std::string& s, const std::string& e) { return s.size() >= e.size() && s.compare(s.size() - e.size(), e.size(), e) == 0; }

// BamWriter::BamWriter (src/cppNGS/BamWriter.cpp:9-30), checked before a device is opened
static void check_bam_output(const std::string& out)
{
	if (ends_with(out, ".cram")) NB_THROW(FileAccessException, "CRAM output is not supported: " + out + ". Write a '.bam' file.");
	if (!ends_with(out, ".bam")) NB_THROW(FileAccessException, "Could not write file: " + out + ". File extension has to be '.bam' or '.cram'.");
}

// The lines of the ID file as :37-43 keeps them: split at '\n' (a last line without one counts), QByteArray::trimmed() (the bytes \t \n \v \f \r and space,
// at both ends only), empty lines and lines that begin with '#' skipped. The names laid end to end in `bytes`, their lengths in `lens`; duplicates stay in
// (the library counts the distinct ones).
static void load_ids(const std::string& path, std::string& bytes, std::vector<int32_t>& lens)
{
	// (a path that does not exist never gets here: the command line's check of an input file refuses it. Left for this one: a path that opens and cannot be
	// read, such as a directory, where QFile::open fails as well - the first read says so)
	std::ifstream f(path, std::ios::binary);
	if (f) f.peek();
	if (!f.is_open() || f.bad()) NB_THROW(FileAccessException, "Could not open file for reading: '" + path + "'!");
	f.clear();   // (an empty file: the end of the file is no error)
	const std::string text((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
	auto blank = [](char c) { return c == '\t' || c == '\n' || c == '\v' || c == '\f' || c == '\r' || c == ' '; };
	for (size_t o = 0; o < text.size(); )
	{
		size_t e = text.find('\n', o);
		if (e == std::string::npos) e = text.size();
		size_t a = o, b = e;
		while (a < b && blank(text[a])) ++a;
		while (b > a && blank(text[b - 1])) --b;
		if (b > a && text[a] != '#') { bytes.append(text, a, b - a); lens.push_back((int32_t)(b - a)); }
		o = e + 1;
	}
}

class ConcreteTool : public ToolBase
{
public:
	ConcreteTool(int argc, char** argv) : ToolBase(argc, argv) {}
	void setup() override
	{
		setDescription("Extract reads from BAM/CRAM by read name.");
		addInfile("in", "Input BAM/CRAM file.", false);
		addInfile("ids", "Input text file containing read names (one per line).", false);
		addOutfile("out", "Output BAM/CRAM file with matching reads.", false);
		addOutfile("out2", "Output BAM/CRAM file with not matching reads.", true);
		addInfile("ref", "Reference genome for CRAM support (mandatory if CRAM is used).", true);
		// --changelog (src/BamExtract/main.cpp)
		changeLog(2023, 11, 30, "Initial implementation.");
	}
	void main() override
	{
		const std::string out = getOutfile("out"), out2 = getOutfile("out2");
		check_bam_output(out);
		if (!out2.empty()) check_bam_output(out2);
		std::string bytes; std::vector<int32_t> lens;
		load_ids(getInfile("ids"), bytes, lens);
		stamp("read names loaded");
		// "Read IDs" comes before the BAM is opened (:45): the distinct names, as QSet::count() gives them (a line of more than 254 bytes counts too)
		int64_t distinct = 0;
		{
			std::vector<std::pair<const char*, int32_t>> v; v.reserve(lens.size());
			size_t o = 0;
			for (int32_t l : lens) { v.emplace_back(bytes.data() + o, l); o += (size_t)l; }
			auto less = [](const std::pair<const char*, int32_t>& a, const std::pair<const char*, int32_t>& b) {
				const int c = memcmp(a.first, b.first, (size_t)std::min(a.second, b.second));
				return c ? c < 0 : a.second < b.second;
			};
			std::sort(v.begin(), v.end(), less);
			for (size_t i = 0; i < v.size(); ++i) if (i == 0 || less(v[i - 1], v[i])) ++distinct;
			printf("Read IDs: %lld\n", (long long)distinct);
			fflush(stdout);
		}
		stamp("arguments");
		BamReader reader(getInfile("in"), getInfile("ref"));
		stamp("open");
		ngsqc_extract_counts c{0, 0, 0};
		reader.check(ngsqc_extract_reads(reader.handle(), bytes.data(), lens.data(), (int64_t)lens.size(), out.c_str(), out2.empty() ? nullptr : out2.c_str(), &c));
		// (the line above was printed from the host's count, before a device existed; the set on the device must hold as many)
		if (c.names != distinct) NB_THROW(ProgrammingException, "BamExtract: " + std::to_string(distinct) + " read IDs counted, " + std::to_string(c.names) + " distinct names in the device's set!");
		stamp("name set, match, gather, deflate and write");
		printf("Reads written to 'out': %lld\n", (long long)c.out);
		if (!out2.empty()) printf("Reads written to 'out2': %lld\n", (long long)c.out2);
	}
};
int main(int argc, char** argv) { ConcreteTool tool(argc, argv); return tool.execute(); }
