// VcfFile: load and store as src/cppNGS/VcfFile.cpp / VcfLine.cpp do it (the subset VcfAnnotateFrequency needs). The header is parsed into its parts and
// written back in the order VcfHeader::storeHeaderInformation uses (VcfLine.cpp:172-194): ##fileformat, the other comment lines, INFO, FILTER, FORMAT lines.
// IDs used in the data lines without a header line get a "no description available" line while the file loads (VcfFile.cpp:160-240). Data lines keep their
// columns except what VcfFile::storeLineInformation (:533-592) rewrites: REF / ALT upper case, QUAL through QByteArray::number (%g), Flag INFO keys.
#pragma once
#include "core.hpp"
#include <zlib.h>
#include <cstdio>

namespace ngsbits {

struct VcfInfoFormatLine { std::string id, number, type, description; };
struct VcfFilterLine { std::string id, description; };

struct VcfRecord
{
	std::string chr, id, ref, qual, filter, format; int pos = 0;
	std::vector<std::string> alt, info_keys, info_values, samples;
	bool has_format = false;
	std::string altString() const { return join(alt, ","); }
	std::string toString() const { return chr + ":" + std::to_string(pos) + " " + ref + ">" + altString(); }   // VcfLine::toString
};

class VcfFile
{
public:
	std::string fileformat;
	std::vector<std::pair<std::string, std::string>> comments;   // key, value
	std::vector<VcfInfoFormatLine> info_lines, format_lines;
	std::vector<VcfFilterLine> filter_lines;
	std::vector<std::string> sample_names;
	std::vector<VcfRecord> lines;

	// setAllowMultiSample(false): only the first sample column is kept (VcfFile.cpp:101, 252)
	void load(const std::string& path, bool allow_multi_sample = false)
	{
		gzFile f = gzopen(path.c_str(), "rb");   // (plain or gzip: VersatileFile)
		if (!f) NB_THROW(FileAccessException, "Could not open file for reading: '" + path + "'!");
		struct Close { gzFile f; ~Close() { gzclose(f); } } closer{f};
		std::string line; std::vector<char> buf(1 << 16); int line_number = 0;
		std::vector<std::string> info_ids, format_ids, filter_ids;
		auto has = [](const std::vector<std::string>& v, const std::string& x) { return std::find(v.begin(), v.end(), x) != v.end(); };
		while (true)
		{
			line.clear(); bool got = false;
			while (gzgets(f, buf.data(), (int)buf.size())) { got = true; line += buf.data(); if (!line.empty() && line.back() == '\n') break; }
			if (!got) break;
			while (!line.empty() && (line.back() == '\n' || line.back() == '\r')) line.pop_back();
			++line_number;
			if (trimmed(line).empty()) continue;
			if (line.rfind("##", 0) == 0) parseHeaderLine(line_number, line);
			else if (line.rfind("#CHROM", 0) == 0)
			{
				std::vector<std::string> h = split(line.substr(1), '\t');
				if (h.size() < 8) NB_THROW(FileParseException, "VCF file header line with less than 8 fields found: '" + trimmed(line) + "'");
				if (h.size() == 9) NB_THROW(FileParseException, "VCF file header line has only FORMAT column but no sample columns.");
				const size_t n = allow_multi_sample ? h.size() : std::min<size_t>(10, h.size());
				for (size_t i = 9; i < n; ++i) sample_names.push_back(h[i]);
				for (auto& l : format_lines) format_ids.push_back(l.id);
				for (auto& l : info_lines) info_ids.push_back(l.id);
				for (auto& l : filter_lines) filter_ids.push_back(l.id);
			}
			else
			{
				std::vector<std::string> c = split(line, '\t');
				if (c.size() < 8) NB_THROW(FileParseException, "VCF data line needs at least 8 tab-separated columns! Found " + std::to_string(c.size()) + " column(s) in line number " + std::to_string(line_number) + ": " + line);
				VcfRecord r;
				r.chr = c[0]; r.pos = atoi(c[1].c_str()); r.id = c[2]; r.ref = upper(c[3]);
				for (const std::string& a : split(c[4], ',')) r.alt.push_back(upper(a));
				if (c[5] == ".") r.qual = ".";
				else
				{
					char* e = nullptr; const double q = strtod(c[5].c_str(), &e);
					if (c[5].empty() || *e) NB_THROW(ArgumentException, "Quality '" + c[5] + "' is no float - variant.");
					char b[64]; snprintf(b, sizeof(b), "%g", q); r.qual = b;   // QByteArray::number(double): 'g', precision 6
				}
				r.filter = c[6];
				for (const std::string& fl : split(c[6], ';'))
					if (!has(filter_ids, fl) && fl != "PASS" && fl != ".") { filter_lines.push_back({fl, "no description available"}); filter_ids.push_back(fl); }
				if (c[7] != ".")
					for (const std::string& kv : split(c[7], ';'))
					{
						const size_t eq = kv.find('=');
						const std::string key = eq == std::string::npos ? kv : kv.substr(0, eq);
						if (!has(info_ids, key)) { info_lines.push_back({key, "1", "String", "no description available"}); info_ids.push_back(key); }
						r.info_keys.push_back(key); r.info_values.push_back(eq == std::string::npos ? "TRUE" : kv.substr(eq + 1));
					}
				if (c.size() >= 9)
				{
					r.has_format = true; r.format = c[8];
					bool first = true;
					for (const std::string& fm : split(c[8], ':'))
					{
						if (fm == "GT" && !first) NB_THROW(FileParseException, "First Format entry is not a genotype ('GT') for line " + std::to_string(line_number) + ": " + line);
						first = false;
						if (!has(format_ids, fm) && fm != ".")
						{
							format_lines.push_back({fm, "1", "String", "no description available"});
							if (fm == "GT") std::rotate(format_lines.begin(), format_lines.end() - 1, format_lines.end());
							format_ids.push_back(fm);
						}
					}
					if (c.size() < 10) NB_THROW(FileParseException, "Format column but no sample columns present in line " + std::to_string(line_number) + ": " + line);
					const size_t last = allow_multi_sample ? c.size() : 10;
					for (size_t i = 9; i < last; ++i) r.samples.push_back(c[i]);
				}
				lines.push_back(r);
			}
		}
	}

	const VcfInfoFormatLine* infoLine(const std::string& id) const { for (auto& l : info_lines) if (l.id == id) return &l; return nullptr; }

	void store(const std::string& path) const
	{
		std::string o = "##fileformat=" + (fileformat.empty() ? std::string("VCFv4.2") : fileformat) + "\n";
		for (auto& c : comments) o += "##" + c.first + "=" + c.second + "\n";
		for (auto& l : info_lines) o += "##INFO=<ID=" + l.id + ",Number=" + l.number + ",Type=" + l.type + ",Description=\"" + l.description + "\">\n";
		for (auto& l : filter_lines) o += "##FILTER=<ID=" + l.id + ",Description=\"" + l.description + "\">\n";
		for (auto& l : format_lines) o += "##FORMAT=<ID=" + l.id + ",Number=" + l.number + ",Type=" + l.type + ",Description=\"" + l.description + "\">\n";
		o += "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO";
		if (!sample_names.empty()) { o += "\tFORMAT"; for (auto& s : sample_names) o += "\t" + s; }
		o += "\n";
		for (const VcfRecord& r : lines)
		{
			o += r.chr + "\t" + std::to_string(r.pos) + "\t" + (r.id.empty() ? "." : r.id) + "\t" + r.ref + "\t" + r.altString() + "\t" + r.qual + "\t" + (r.filter.empty() ? "." : r.filter) + "\t";
			if (r.info_keys.empty()) o += ".";
			for (size_t k = 0; k < r.info_keys.size(); ++k)
			{
				if (k) o += ";";
				const VcfInfoFormatLine* l = infoLine(r.info_keys[k]);
				if (r.info_values[k] == "TRUE" && l && l->type == "Flag") o += r.info_keys[k];
				else o += r.info_keys[k] + "=" + r.info_values[k];
			}
			if (!sample_names.empty()) { o += "\t" + r.format; for (auto& s : r.samples) o += "\t" + s; }
			o += "\n";
		}
		FILE* f = fopen(path.c_str(), "wb");
		if (!f) NB_THROW(FileAccessException, "Could not open file for writing: '" + path + "'!");
		fwrite(o.data(), 1, o.size(), f);
		fclose(f);
	}

private:
	static std::string upper(std::string s) { for (auto& ch : s) ch = (char)toupper((unsigned char)ch); return s; }
	void parseHeaderLine(int line_number, const std::string& line)
	{
		if (line_number == 1)
		{
			if (line.rfind("##fileformat", 0) != 0) NB_THROW(FileParseException, "Malformed first line for the fileformat: " + trimmed(line));
			std::vector<std::string> p = split(line, '=');
			if (p.size() < 2) NB_THROW(FileParseException, "Malformed fileformat line " + trimmed(line));
			fileformat = p[1];
		}
		else if (line.rfind("##INFO", 0) == 0) { VcfInfoFormatLine l; if (parseInfoFormat(line.substr(8), l, "INFO", info_lines)) info_lines.push_back(l); }
		else if (line.rfind("##FORMAT", 0) == 0)
		{
			VcfInfoFormatLine l;
			if (parseInfoFormat(line.substr(10), l, "FORMAT", format_lines)) { format_lines.push_back(l); if (l.id == "GT" && format_lines.size() > 1) std::rotate(format_lines.begin(), format_lines.end() - 1, format_lines.end()); }
		}
		else if (line.rfind("##FILTER=<ID=", 0) == 0)
		{
			// VcfHeader::setFilterLine (VcfLine.cpp:257-286)
			std::vector<std::string> parts = split(line.size() >= 15 ? line.substr(13, line.size() - 15) : std::string(), '=');
			if (!parts.empty() && parts[0].size() >= 11 && parts[0].compare(parts[0].size() - 11, 11, "Description") == 0)
			{
				std::vector<std::string> rest(parts.begin() + 1, parts.end());
				parts = {parts[0], join(rest, "=")};
			}
			if (parts.size() != 2) NB_THROW(FileParseException, "Malformed FILTER line " + std::to_string(line_number) + " : conains more/less than two parts: " + line);
			std::vector<std::string> first = split(parts[0], ',');
			if (first.size() != 2 || trimmed(first[1]) != "Description") NB_THROW(FileParseException, "Malformed FILTER line " + std::to_string(line_number) + ": second field is not a description field " + trimmed(line));
			filter_lines.push_back({first[0], parts[1].substr(std::min<size_t>(1, parts[1].size()))});
		}
		else
		{
			// VcfHeader::setCommentLine (:288-307)
			std::vector<std::string> p = split(line.substr(2), '=');
			if (p.size() < 2) NB_THROW(FileParseException, "Malformed header line " + std::to_string(line_number) + " is not a key=value pair: " + trimmed(line));
			std::vector<std::string> rest(p.begin() + 1, p.end());
			comments.emplace_back(p[0], join(rest, "="));
		}
	}
	// VcfHeader::parseInfoFormatLine (:318-403); false: a duplicate ID (skipped)
	static bool parseInfoFormat(const std::string& line, VcfInfoFormatLine& out, const std::string& type, const std::vector<VcfInfoFormatLine>& have)
	{
		std::vector<std::string> c = split(line, ',');
		if (c.size() < 4) NB_THROW(FileParseException, "Malformed " + type + " line: has less than 4 entries " + trimmed(line));
		std::vector<std::string> idp = split(c[0], '=');
		if (idp[0].rfind("ID", 0) != 0 || idp.size() < 2) NB_THROW(FileParseException, "Malformed " + type + " line: does not start with ID-field " + idp[0]);
		out.id = idp[1];
		std::vector<std::string> np = split(c[1], '=');
		if (trimmed(np[0]).rfind("Number", 0) != 0 || np.size() < 2) NB_THROW(FileParseException, "Malformed " + type + " line: second field is not a number field " + np[0]);
		out.number = np[1];
		std::vector<std::string> tp = split(c[2], '=');
		if (trimmed(tp[0]) != "Type" || tp.size() < 2) NB_THROW(FileParseException, "Malformed " + type + " line: third field is not a type field " + trimmed(line) + "'");
		static const std::vector<std::string> info_types = {"Integer", "Float", "Flag", "Character", "String"}, format_types = {"Integer", "Float", "Character", "String"};
		const auto& types = type == "INFO" ? info_types : format_types;
		if (std::find(types.begin(), types.end(), tp[1]) == types.end()) NB_THROW(FileParseException, "Malformed " + type + " line: undefined value for type " + trimmed(line) + "'");
		out.type = tp[1];
		std::vector<std::string> dp = split(c[3], '=');
		if (trimmed(dp[0]) != "Description" || dp.size() < 2) NB_THROW(FileParseException, "Malformed " + type + " line: fourth field is not a description field " + trimmed(line));
		std::vector<std::string> desc = {dp[1]}; desc.insert(desc.end(), c.begin() + 4, c.end());
		std::string d = join(desc, ",");
		d = d.size() >= 1 ? d.substr(1) : d;                  // '"'
		d = d.size() >= 2 ? d.substr(0, d.size() - 2) : "";   // '">'
		out.description = d;
		for (auto& l : have) if (l.id == out.id) { fprintf(stderr, "Duplicate metadata information for field named '%s'. Skipping metadata line.\n", out.id.c_str()); return false; }
		return true;
	}
};

} // namespace ngsbits
