// BamRemoveVariants - drop-in for src/BamRemoveVariants/main.cpp:16-278 on the MI355X path: same flags, help text and output. The VCF.GZ is read here into a
// table of lines (host/RmVariants.hpp: what TabixIndexedFile::getMatchingLines and Variant(VcfLine) make of every line); the loop of main() (:138-272: the
// look-up of every alignment's variants, alignment_pass / mask_alignment, the mate cache by read name, BamWriter::writeAlignment) runs as one pass over the BAM on
// the GPU, the masked bases are stored in the gathered copy there, and the BGZF writer deflates on the GPU as well (ngsqc_remove_variants: csrc/rmvar.hip,
// csrc/deflate.hip). An alignment with no chromosome (tid < 0) indexes chrs_[-1] in the reference, which is undefined there: here it overlaps no variant and
// is kept as it is. The tabix index has to exist, as TabixIndexedFile::load demands (src/cppNGS/TabixIndexedFile.cpp:29-32), but is not read: every record meets
// the whole table on the device.
#include "Statistics.hpp"
#include "RmVariants.hpp"
using namespace ngsbits;

static bool ends_with(const std::string& s, const std::string& e) { return s.size() >= e.size() && s.compare(s.size() - e.size(), e.size(), e) == 0; }

class ConcreteTool : public ToolBase
{
public:
	ConcreteTool(int argc, char** argv) : ToolBase(argc, argv) {}
	void setup() override
	{
		setDescription("Removes reads which contain the provided variants");
		addInfile("in", "Input BAM/CRAM file.", false);
		addOutfile("out", "Output BAM/CRAM file.", false);
		addInfile("vcf", "Input indexed VCF.GZ file.", false);
		addInfile("ref", "Reference genome for CRAM support (mandatory if CRAM is used).", true);
		addFlag("mask", "Replace variant bases with reference instead of removing the read (SNV only)");
		addFlag("single_end", "Input file is from single-end sequencing (e.g. lrGS).");
		addFlag("keep_indels", "Do not remove InDels in mask mode.");
		// --changelog (src/BamRemoveVariants/main.cpp)
		changeLog(2024, 7, 24, "Inital commit.");
		changeLog(2025, 1, 17, "Added mask option.");
		changeLog(2025, 1, 20, "Added single-end mode.");
	}
	void main() override
	{
		const std::string out = getOutfile("out"), vcf = getInfile("vcf");
		// BamWriter::BamWriter (src/cppNGS/BamWriter.cpp:9-30), checked before a device is opened
		if (ends_with(out, ".cram")) NB_THROW(FileAccessException, "CRAM output is not supported: " + out + ". Write a '.bam' file.");
		if (!ends_with(out, ".bam")) NB_THROW(FileAccessException, "Could not write file: " + out + ". File extension has to be '.bam' or '.cram'.");
		// TabixIndexedFile::load (TabixIndexedFile.cpp:25-32)
		{ std::ifstream f(vcf, std::ios::binary); if (f) f.peek(); if (!f.is_open() || f.bad()) NB_THROW(FileParseException, "Could not open data file " + vcf); }
		if (!fileExists(vcf + ".csi") && !fileExists(vcf + ".tbi")) NB_THROW(FileAccessException, "Could not determine tabix index of file " + vcf);
		ngsqc_rm_params p{getFlag("mask") ? 1 : 0, getFlag("single_end") ? 1 : 0, getFlag("keep_indels") ? 1 : 0};
		stamp("arguments");
		BamReader reader(getInfile("in"), getInfile("ref"));
		stamp("open");
		std::vector<std::string> ref_names;
		for (const Chromosome& c : reader.chromosomes()) ref_names.push_back(c.str());
		const RmVariantTable table = loadRmVariants(vcf, ref_names);
		stamp("variant table");
		ngsqc_rm_counts c{0, 0, 0, 0, -1, 0, -1};
		const int rc = ngsqc_remove_variants(reader.handle(), table.lines.data(), (int64_t)table.lines.size(), &p, out.c_str(), &c);
		// (a line Variant(VcfLine) refuses throws where an alignment first visits it, main.cpp:45 / :79)
		if (rc != NGSQC_OK && c.err_code == NGSQC_RMERR_INVALID_LINE && c.err_variant >= 0 && (size_t)c.err_variant < table.lines.size()) NB_THROW(Exception, table.invalid_message[(size_t)c.err_variant]);
		reader.check(rc);
		stamp("verdicts, join, gather, deflate and write");
		printf("pairs passed: %lld\npairs dropped: %lld\nreads modified: %lld\nskipped reads: %lld\n", (long long)c.passed, (long long)c.dropped, (long long)c.modified, (long long)c.skipped);
	}
};
int main(int argc, char** argv) { ConcreteTool tool(argc, argv); return tool.execute(); }
