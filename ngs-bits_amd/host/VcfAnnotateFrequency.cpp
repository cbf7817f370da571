// VcfAnnotateFrequency - drop-in for src/VcfAnnotateFrequency/main.cpp on the MI355X path (same flags, help text, output). The reference calls
// BamReader::getVariantDetails once per variant (src/cppNGS/BamReader.cpp:888-946: an indexed pileup per SNV, an indexed getIndels per indel); here the SNV
// sites and the indel windows of the whole VCF go to the GPU in one decode of the BAM (ngsqc_variant_details), opened through the index over the variants only.
#include "Statistics.hpp"
#include "Variant.hpp"
#include <cmath>
using namespace ngsbits;

static std::string numberF4(double x) { char b[64]; snprintf(b, sizeof(b), "%.4f", x); return b; }   // QByteArray::number(x, 'f', 4)

class ConcreteTool : public ToolBase
{
public:
	ConcreteTool(int argc, char** argv) : ToolBase(argc, argv) {}
	void setup() override
	{
		setDescription("Annotates VCF variants with allele frequency and depth from a BAM/CRAM file.");
		addInfile("in", "Input variant list to annotate in VCF(.GZ) format.", false, true);
		addInfile("bam", "Input BAM/CRAM file.", false, true);
		addOutfile("out", "Output variant list file in VCF format.", false);
		addFlag("depth", "Annotate an additional INFO field entry containing the depth.");
		addString("name", "INFO field entry prefix in output file.", true, "N");
		addInfile("ref", "Reference genome FASTA file. If unset 'reference_genome' from the 'settings.ini' file is used.", true, false);
		changeLog(2025, 11, 28, "Initial version.");
	}
	void main() override
	{
		const bool with_depth = getFlag("depth");
		std::string ref_file = getInfile("ref");
		const std::string name = getString("name");
		if (ref_file == "") ref_file = settingsString("reference_genome");
		if (ref_file == "") NB_THROW(CommandLineParsingException, "Reference genome FASTA unset in both command-line and settings.ini file!");

		VcfFile vcf; vcf.load(getInfile("in"), false);   // setAllowMultiSample(false): the first sample is kept
		FastaFileIndex reference(ref_file);
		const size_t n = vcf.lines.size();

		// every variant: an SNV site of the pileup or an indel window of getIndels (BamReader.cpp:888-946); the device wants both sorted, the output keeps the input order
		struct Job { int tid = -1; bool snv = false, window = false; int start = 0, end = 0; int kind = NGSQC_ALLELE_NONE; std::string allele, slice; char obs = 'N'; };
		std::vector<Job> jobs(n);
		std::vector<Variant> vars; vars.reserve(n);
		for (size_t i = 0; i < n; ++i) vars.push_back(Variant::fromVcf(vcf.lines[i]));
		// the index-driven open: only the BAM ranges of the variants' windows are decoded (a VCF of a few hundred lines on a 30x genome)
		BedFile roi;
		for (size_t i = 0; i < n; ++i)
		{
			const Variant& v = vars[i]; Job& j = jobs[i]; const Chromosome chr(v.chr);
			if (v.isSNV()) { j.snv = true; j.start = j.end = v.start; j.obs = v.obs[0]; }
			else
			{
				const std::pair<int, int> reg = variantIndelRegion(v.start, v.end, v.ref, v.obs, [&](int p, int l) { return reference.seq(chr, p, l); });
				j.start = reg.first - 1; j.end = reg.second + 1;
				// a window that starts in front of the contig: no read starts at or before it, depth and count stay 0 (getIndels :984) - nothing to ask the device
				if (j.start < 1) continue;
				j.window = true;
				// the query allele: Variant::normalize("-") (:930-955); a complex variant counts min(insertions, deletions)
				Variant q = v; q.normalize("-", false);
				if (q.ref == "-") { j.kind = NGSQC_ALLELE_INS; j.allele = q.obs; }
				else if (q.obs == "-") { j.kind = NGSQC_ALLELE_DEL; j.allele = q.ref; j.slice = reference.seq(chr, j.start, j.end - j.start + (int)q.ref.size()); j.slice.resize((size_t)(j.end - j.start) + q.ref.size(), '\0'); }
			}
			roi.append(BedLine(chr, j.start, j.end));
		}
		roi.sort(); roi.merge(false);
		BamReader reader(getInfile("bam"), ref_file, false, roi);
		std::vector<size_t> site_of, win_of;
		for (size_t i = 0; i < n; ++i) { jobs[i].tid = reader.chromosomeID(Chromosome(vars[i].chr)); if (jobs[i].snv) site_of.push_back(i); else if (jobs[i].window) win_of.push_back(i); }
		auto by_pos = [&](size_t a, size_t b) { return jobs[a].tid != jobs[b].tid ? jobs[a].tid < jobs[b].tid : jobs[a].start < jobs[b].start; };
		std::stable_sort(site_of.begin(), site_of.end(), by_pos); std::stable_sort(win_of.begin(), win_of.end(), by_pos);
		std::vector<ngsqc_region> sites; std::vector<size_t> site_line;
		for (size_t i : site_of) { if (jobs[i].tid < 0) NB_THROW(FileAccessException, "Could not find chromosome '" + vars[i].chr + "' in BAM/CRAM file " + getInfile("bam")); sites.push_back(ngsqc_region{jobs[i].tid, jobs[i].start, jobs[i].start}); site_line.push_back(i); }
		std::vector<ngsqc_indel_window> wins; std::vector<size_t> win_line;
		for (size_t i : win_of)
		{
			const Job& j = jobs[i];
			if (j.tid < 0) NB_THROW(FileAccessException, "Could not find chromosome '" + vars[i].chr + "' in BAM/CRAM file " + getInfile("bam"));
			wins.push_back(ngsqc_indel_window{j.tid, j.start, j.end, j.kind, (int32_t)j.allele.size(), j.allele.c_str(), j.kind == NGSQC_ALLELE_DEL ? j.slice.data() : nullptr});
			win_line.push_back(i);
		}
		std::vector<int64_t> sc(sites.size() * 8 + 1), wc(wins.size() * NGSQC_INDEL_NCOUNTERS + 1);
		ngsqc_variant_params prm{0, 0, 1, 13};   // getVariantDetails(reference, variant, false): getPileup(..., 1 /*min_mapq*/, false, 13 /*min_baseq*/)
		reader.check(ngsqc_variant_details(reader.handle(), sites.data(), (int64_t)sites.size(), wins.data(), (int64_t)wins.size(), &prm, sc.data(), wc.data()));
		std::vector<long long> depth(n, 0); std::vector<double> freq(n, 0.0);
		for (size_t k = 0; k < sites.size(); ++k)
		{
			const int64_t* c = sc.data() + 8 * k; const size_t i = site_line[k];
			depth[i] = c[0] + c[1] + c[2] + c[3] + c[5];   // Pileup::depth(true)
			const char b = jobs[i].obs; const int bi = b == 'A' ? 0 : b == 'C' ? 1 : b == 'G' ? 2 : b == 'T' ? 3 : b == 'N' ? 4 : -1;
			if (bi < 0) NB_THROW(ArgumentException, std::string("Unknown base '") + b + "' in counting function!");
			if (depth[i] != 0) freq[i] = c[bi] / (double)depth[i];
		}
		for (size_t k = 0; k < wins.size(); ++k)
		{
			const int64_t* c = wc.data() + NGSQC_INDEL_NCOUNTERS * k; const size_t i = win_line[k];
			depth[i] = c[NGSQC_W_DEPTH];
			const long long obs = jobs[i].kind == NGSQC_ALLELE_NONE ? std::min(c[NGSQC_W_INS], c[NGSQC_W_DEL]) : c[NGSQC_W_MATCH];
			freq[i] = std::min(1.0, obs / (double)depth[i]);   // (more events than depth in a window, :955)
		}

		// INFO: the new keys first, then the old ones (setInfo); header lines for the new keys behind the INFO lines of the input (VcfHeader::addInfoLine)
		for (size_t i = 0; i < n; ++i)
		{
			VcfRecord& r = vcf.lines[i];
			std::vector<std::string> keys = {name + "_AF"}, values = {depth[i] == 0 || !std::isfinite(freq[i]) ? std::string("0") : numberF4(freq[i])};
			if (with_depth) { keys.push_back(name + "_DP"); values.push_back(std::to_string(depth[i])); }
			keys.insert(keys.end(), r.info_keys.begin(), r.info_keys.end()); values.insert(values.end(), r.info_values.begin(), r.info_values.end());
			r.info_keys = keys; r.info_values = values;
		}
		const std::string sample = name == "N" ? "normal sample" : name;
		vcf.info_lines.push_back({name + "_AF", "1", "Float", "Variant allele frequency in " + sample});
		if (with_depth) vcf.info_lines.push_back({name + "_DP", "1", "Integer", "Read depth in " + sample});
		vcf.store(getOutfile("out"));
	}
};
int main(int argc, char** argv) { ConcreteTool tool(argc, argv); return tool.execute(); }
