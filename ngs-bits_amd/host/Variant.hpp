// Variant::normalize / minBlock / indelRegion (src/cppNGS/VariantList.cpp:273-291, 1283-1384) and Variant(const VcfLine&) (:49-64): the windows of
// BamReader::getVariantDetails (BamReader.cpp:888-946).
#pragma once
#include "Vcf.hpp"

namespace ngsbits {

inline void variantNormalize(int& start, std::string& ref, std::string& obs)
{
	auto multi = [&] { return (ref.size() != 1 || obs.size() != 1) && !ref.empty() && !obs.empty(); };
	if (multi() && ref[0] == obs[0]) { ref.erase(0, 1); obs.erase(0, 1); start += 1; }   // common first base
	while (multi() && ref.back() == obs.back()) { ref.pop_back(); obs.pop_back(); }     // common suffix
	while (multi() && ref[0] == obs[0]) { ref.erase(0, 1); obs.erase(0, 1); start += 1; }   // common prefix
}
inline std::string variantMinBlock(const std::string& seq)
{
	const size_t len = seq.size();
	for (size_t size = 1; size <= len / 2; ++size)
	{
		if (len % size) continue;
		std::string rep; for (size_t k = 0; k < len / size; ++k) rep += seq.substr(0, size);
		if (rep == seq) return seq.substr(0, size);
	}
	return seq;
}
// seq(pos, len): FastaFileIndex::seq of the variant's chromosome
template <typename Seq> std::pair<int, int> variantIndelRegion(int start, int end, std::string ref, std::string obs, const Seq& seq)
{
	if (ref == "-") ref = "";
	if (obs == "-") obs = "";
	variantNormalize(start, ref, obs);
	if (!ref.empty() && !obs.empty()) return {start, end};   // SNV or complex: the original position
	const int start_orig = start, end_orig = end;
	const std::string block = variantMinBlock(ref + obs); const int bl = (int)block.size();
	bool is_repeat = false;
	end -= bl - 1;
	while (seq(end + bl, bl) == block) { end += bl; is_repeat = true; }
	if (ref.empty()) start += 1;   // insertion: start and end are in front of the inserted bases
	while (seq(start - bl, bl) == block) { start -= bl; is_repeat = true; }
	if (is_repeat) return {start, end + bl - 1};
	return {start_orig, end_orig};
}

// Variant(const VcfLine&): start, end, ref, obs after normalize("-", true) (GSvar form: an insertion sits on the base in front of it)
struct Variant
{
	std::string chr; int start = 0, end = 0; std::string ref, obs;
	bool isSNV() const { return ref.size() == 1 && obs.size() == 1 && ref != "-" && obs != "-"; }
	void normalize(const std::string& empty_seq, bool to_gsvar_format)
	{
		variantNormalize(start, ref, obs);
		end = start + (int)ref.size() - 1;
		if (ref.empty()) { ref = empty_seq; end += 1; }
		if (obs.empty()) obs = empty_seq;
		if (to_gsvar_format && ref == empty_seq) { start -= 1; end -= 1; }
	}
	static bool onlyACGT(const std::string& s) { if (s.empty()) return false; for (char c : s) if (c != 'A' && c != 'C' && c != 'G' && c != 'T') return false; return true; }
	static Variant fromVcf(const VcfRecord& v)
	{
		bool valid = v.pos >= 0 && onlyACGT(v.ref) && !v.alt.empty();
		for (const std::string& a : v.alt) valid = valid && (onlyACGT(a) || a == "<NON_REF>");
		if (!valid) NB_THROW(Exception, "Cannot convert invalid VCF variant to GSvar variant: " + v.toString());
		if (v.alt.size() > 1) NB_THROW(Exception, "Cannot convert multi-allelic VCF variant to GSvar variant: " + v.toString());
		Variant o; o.chr = v.chr; o.start = v.pos; o.end = v.pos + (int)v.ref.size() - 1; o.ref = v.ref; o.obs = v.altString();
		o.normalize("-", true);
		return o;
	}
};

} // namespace ngsbits
