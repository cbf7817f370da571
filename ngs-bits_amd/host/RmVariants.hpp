// The variant table of BamRemoveVariants: the data lines of an indexed VCF.GZ as TabixIndexedFile::getMatchingLines (src/cppNGS/TabixIndexedFile.cpp:96-129)
// and alignment_pass / mask_alignment (src/BamRemoveVariants/main.cpp:41-45, :75-79) see them, for ngsqc_remove_variants (include/ngsqc.h).
//   span      what htslib's VCF preset gives a line (tbx_parse1): [POS, POS + len(REF) - 1], or up to END when INFO holds END=<n> behind POS - 1.
//   kind      Variant(VcfLine(chr, POS, REF, [ALT])) (VariantList.cpp:49-64): the ALT column is ONE allele there (a comma makes it invalid, as a lower-case base
//             does: the columns are not upper-cased on this path) - INVALID with the message the constructor throws, else normalize("-", true) and isSNV():
//             SNV with its two bases, or OTHER. "<NON_REF>" is a valid allele of nine characters: never an SNV (the branches of main.cpp:55 and :89 that
//             ask for it behind isSNV() cannot be reached), so such a line is OTHER.
//   tid       chromosomes are matched through Chromosome::num() (TabixIndexedFile.cpp:40-45, :101): of the VCF's names with one number the last one
//             named is looked up, and its lines go to the first reference of the BAM with that number; every other line gets tid -1 and matches nothing.
// The whole file is read with zlib; the index is not needed. A tabix index exists for sorted files only: a file whose lines of one chromosome are not in one
// block, or not in the order of POS, is refused.
#pragma once
#include "Variant.hpp"
#include "../../include/ngsqc.h"
#include <map>

namespace ngsbits {

struct RmVariantTable
{
	std::vector<ngsqc_rm_variant> lines;     // one per data line, in file order
	std::vector<std::string> invalid_message;   // what a visit of an INVALID line throws ("" for the others)
};

inline RmVariantTable loadRmVariants(const std::string& path, const std::vector<std::string>& ref_names)
{
	gzFile f = gzopen(path.c_str(), "rb");
	if (!f) NB_THROW(FileParseException, "Could not open data file " + path);
	struct Close { gzFile f; ~Close() { gzclose(f); } } closer{f};
	RmVariantTable t;
	std::vector<std::string> names;                 // the VCF's chromosomes in the order of their first line (tbx_seqnames)
	std::vector<int> name_of_line;
	std::map<std::string, int> name_id;
	std::string line; std::vector<char> buf(1 << 16); long long line_number = 0; int prev_pos = 0;
	while (true)
	{
		line.clear(); bool got = false;
		while (gzgets(f, buf.data(), (int)buf.size())) { got = true; line += buf.data(); if (!line.empty() && line.back() == '\n') break; }
		if (!got) break;
		if (!line.empty() && line.back() == '\n') line.pop_back();
		++line_number;
		if (line.empty() || line[0] == '#') continue;
		const std::vector<std::string> c = split(line, '\t');
		if (c.size() < 5) NB_THROW(FileParseException, "VCF data line with less than 5 tab-separated columns in line number " + std::to_string(line_number) + " of " + path);
		char* e = nullptr; const long pl = strtol(c[1].c_str(), &e, 10);
		const int pos = (c[1].empty() || *e || pl < INT32_MIN || pl > INT32_MAX) ? 0 : (int)pl;   // QByteArray::toInt: 0 when it is no number
		auto it = name_id.find(c[0]);
		const bool new_block = name_of_line.empty() || names[(size_t)name_of_line.back()] != c[0];
		if (new_block && it != name_id.end()) NB_THROW(FileParseException, "VCF file is not sorted, as its tabix index requires: chromosome '" + c[0] + "' comes again in line number " + std::to_string(line_number) + " of " + path);
		if (!new_block && pos < prev_pos) NB_THROW(FileParseException, "VCF file is not sorted, as its tabix index requires: position " + std::to_string(pos) + " behind " + std::to_string(prev_pos) + " in line number " + std::to_string(line_number) + " of " + path);
		if (it == name_id.end()) { it = name_id.emplace(c[0], (int)names.size()).first; names.push_back(c[0]); }
		name_of_line.push_back(it->second); prev_pos = pos;
		ngsqc_rm_variant v{-1, pos, pos + (int)c[3].size() - 1, pos, NGSQC_RMVAR_INVALID, 0, 0, 0};
		if (c.size() > 7)   // INFO END (tbx_parse1)
		{
			size_t s = c[7].rfind("END=", 0) == 0 ? 4 : std::string::npos;
			if (s == std::string::npos) { s = c[7].find(";END="); if (s != std::string::npos) s += 5; }
			if (s != std::string::npos && s < c[7].size() && c[7][s] != '.') { const long long end = strtoll(c[7].c_str() + s, nullptr, 0); if (end > (long long)pos - 1 && end <= INT32_MAX) v.end = (int)end; }
		}
		std::string msg;
		try
		{
			VcfRecord r; r.chr = c[0]; r.pos = pos; r.ref = c[3]; r.alt = {c[4]};
			if (!Chromosome(c[0]).isValid()) NB_THROW(Exception, "Cannot convert invalid VCF variant to GSvar variant: " + r.toString());
			const Variant var = Variant::fromVcf(r);
			v.start = var.start;
			if (var.isSNV()) { v.kind = NGSQC_RMVAR_SNV; v.ref = (uint8_t)var.ref[0]; v.obs = (uint8_t)var.obs[0]; }
			else v.kind = NGSQC_RMVAR_OTHER;
		}
		catch (Exception& ex) { msg = ex.what(); }
		t.lines.push_back(v); t.invalid_message.push_back(msg);
	}
	// Chromosome::num() of a VCF name -> the name looked up (the last one named wins, TabixIndexedFile.cpp:40-45), -> the first reference of the BAM
	std::map<int, int> name_of_num, tid_of_num;
	for (size_t i = 0; i < names.size(); ++i) name_of_num[Chromosome(names[i]).num()] = (int)i;
	for (size_t i = 0; i < ref_names.size(); ++i) tid_of_num.emplace(Chromosome(ref_names[i]).num(), (int)i);
	for (size_t i = 0; i < t.lines.size(); ++i)
	{
		const int num = Chromosome(names[(size_t)name_of_line[i]]).num();
		auto tt = tid_of_num.find(num);
		if (name_of_num[num] == name_of_line[i] && tt != tid_of_num.end()) t.lines[i].tid = tt->second;
	}
	return t;
}

} // namespace ngsbits
