// BamClipOverlap - drop-in for src/BamClipOverlap/main.cpp:8-554 on the MI355X path: same flags, help text and summary lines. The loop of main() (:62-547: the
// preconditions, the mate map by read name, the overlap of every pair, NGSHelper::softClipAlignment, BamWriter::writeAlignment) runs as one pass over the BAM on
// the GPU, the clipped records are rewritten there, and the BGZF writer deflates on the GPU as well (ngsqc_clip_overlap: csrc/clip.hip, csrc/clip_visit.h,
// csrc/deflate.hip). The reads whose mate never comes are written behind all others in file order (the reference: in QHash order). -v is accepted and adds
// nothing: the per-pair log of the reference exists in the tests' restatement only (tests/bamclipoverlap_oracle.py), which reproduces the reference's logs.
#include "Statistics.hpp"
#include "ClipOverlap.hpp"
using namespace ngsbits;

static bool ends_with(const std::string& s, const std::string& e) { return s.size() >= e.size() && s.compare(s.size() - e.size(), e.size(), e) == 0; }

class ConcreteTool : public ToolBase
{
public:
	ConcreteTool(int argc, char** argv) : ToolBase(argc, argv) {}
	void setup() override
	{
		setDescription("Softclipping of overlapping reads.");
		setExtendedDescription({"Overlapping reads will be soft-clipped from start to end. There are several parameters available for handling of mismatches in overlapping reads. "
		                        "Within the overlap the higher base quality will be kept for each basepair."});
		addInfile("in", "Input BAM/CRAM file. Needs to be sorted by name.", false);
		addOutfile("out", "Output BAM file.", false);
		addFlag("overlap_mismatch_mapq", "Set mapping quality of pair to 0 if mismatch is found in overlapping reads.");
		addFlag("overlap_mismatch_remove", "Remove pair if mismatch is found in overlapping reads.");
		addFlag("overlap_mismatch_baseq", "Reduce base quality if mismatch is found in overlapping reads.");
		addFlag("overlap_mismatch_basen", "Set base to N if mismatch is found in overlapping reads.");
		addFlag("ignore_indels", "Turn off indel detection in overlap.");
		addFlag("v", "Verbose mode.");
		addInfile("ref", "Reference genome for CRAM support (mandatory if CRAM is used).", true);
		// --changelog (src/BamClipOverlap/main.cpp)
		changeLog(2020, 11, 27, "Added CRAM support.");
		changeLog(2018, 1, 11, "Updated base quality handling within overlap.");
		changeLog(2017, 1, 16, "Added overlap mismatch filter.");
	}
	void main() override
	{
		const std::string out = getOutfile("out");
		// BamWriter::BamWriter (src/cppNGS/BamWriter.cpp:9-30), checked before a device is opened
		if (ends_with(out, ".cram")) NB_THROW(FileAccessException, "CRAM output is not supported: " + out + ". Write a '.bam' file.");
		if (!ends_with(out, ".bam")) NB_THROW(FileAccessException, "Could not write file: " + out + ". File extension has to be '.bam' or '.cram'.");
		const int mode = (getFlag("overlap_mismatch_mapq") ? NGSQC_CLIP_MAPQ : 0) | (getFlag("overlap_mismatch_remove") ? NGSQC_CLIP_REMOVE : 0)
		               | (getFlag("overlap_mismatch_baseq") ? NGSQC_CLIP_BASEQ : 0) | (getFlag("overlap_mismatch_basen") ? NGSQC_CLIP_BASEN : 0);
		(void)getFlag("v");
		stamp("arguments");
		BamReader reader(getInfile("in"), getInfile("ref"));
		stamp("open");
		int64_t counts[6] = {0, 0, 0, 0, 0, 0};
		ngsqc_clip_error err{-1, 0, 0, 0};
		reader.check(ngsqc_clip_overlap(reader.handle(), out.c_str(), mode, getFlag("ignore_indels") ? 1 : 0, -1, counts, &err));
		stamp("join, plan, gather, deflate and write");
		std::string lost;
		const std::string text = clipSummary(counts, lost);
		if (!lost.empty()) NB_THROW(ToolFailedException, lost);
		fputs(text.c_str(), stderr);
	}
};
int main(int argc, char** argv) { ConcreteTool tool(argc, argv); return tool.execute(); }
