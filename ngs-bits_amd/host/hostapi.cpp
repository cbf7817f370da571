// A small C entry into the host layer for bench.py and the C-ABI tests: the region tables they pass to libngsqc_hip.so come from the PRODUCT's
// BedFile / Chromosome code (load, sort, merge, chunk; BedFile.cpp / Chromosome.cpp of the reference), not from the oracle's BED loader - so the measured path and
// the parity tests exercise host/core.cpp as well. Built as bin/libngsqc_hostapi.so; not part of the C ABI of include/ngsqc.h.
#include "core.hpp"
#include "Variant.hpp"
#include "RmVariants.hpp"
#include "ClipOverlap.hpp"
#include "FastqReader.hpp"
#include <cstring>
using namespace ngsbits;

extern "C" {

// mode: 0 as loaded, 1 merge(), 2 merge(true, true), 3 sort + merge, 4 merge + chunk(100), 5 sort + merge + chunk(100)  (the operations the reference applies to its ROI:
// Statistics.cpp:352-387, 1000-1010; BedCoverage / BedLowCoverage main.cpp). ref_names: the BAM's references in tid order. out: rows (tid or -1, start 1-based, end).
// Returns the number of lines (also when it exceeds cap: call again with a larger buffer), -1 on an error (message in err).
long long ngsbits_bed_regions(const char* bed_path, const char* const* ref_names, int n_ref, int mode, int* out, long long cap, char* err, int err_cap)
{
	try
	{
		BedFile bed; bed.load(bed_path, false);
		if (mode == 3 || mode == 5) bed.sort();
		if (mode == 1 || mode == 3 || mode == 4 || mode == 5) bed.merge();
		if (mode == 2) bed.merge(true, true);
		if (mode == 4 || mode == 5) bed.chunk(100);
		std::vector<std::pair<int, int>> tid_of;   // Chromosome::num() -> first tid with that number
		for (int t = 0; t < n_ref; ++t) { const int num = Chromosome(ref_names[t]).num(); bool have = false; for (auto& p : tid_of) have = have || p.first == num; if (!have) tid_of.emplace_back(num, t); }
		for (long long i = 0; i < bed.count() && i < cap; ++i)
		{
			int tid = -1; for (auto& p : tid_of) if (p.first == bed[i].chr().num()) tid = p.second;
			out[3 * i] = tid; out[3 * i + 1] = bed[i].start(); out[3 * i + 2] = bed[i].end();
		}
		return bed.count();
	}
	catch (std::exception& e) { if (err && err_cap > 0) { strncpy(err, e.what(), (size_t)err_cap - 1); err[err_cap - 1] = 0; } return -1; }
}


static int fail(const std::exception& e, char* err, int err_cap) { if (err && err_cap > 0) { strncpy(err, e.what(), (size_t)err_cap - 1); err[err_cap - 1] = 0; } return -1; }

// VcfFile::load (setAllowMultiSample(false)) + VcfFile::store of VcfAnnotateFrequency (host/Vcf.hpp). 0, or -1 with the message in err.
int ngsbits_vcf_roundtrip(const char* in_path, const char* out_path, char* err, int err_cap)
{
	try { VcfFile v; v.load(in_path, false); v.store(out_path); return 0; }
	catch (std::exception& e) { return fail(e, err, err_cap); }
}

// Variant(const VcfLine&) of a VCF line (pos, ref, alt; upper-cased as VcfFile::load does) and the window of getVariantDetails: *start / *end after normalize("-", true), ref / obs (64 bytes
// each), and for an indel Variant::indelRegion over the FASTA (region = -1 / -1 for an SNV). 0, or -1 with the message in err.
int ngsbits_variant_region(const char* fasta, const char* chr, int pos, const char* ref, const char* alt, int* start, int* end, char* ref_out, char* obs_out,
                           int* reg_first, int* reg_second, char* err, int err_cap)
{
	try
	{
		VcfRecord r; r.chr = chr; r.pos = pos; r.ref = ref; r.alt = split(alt, ',');
		for (auto& c : r.ref) c = (char)toupper((unsigned char)c);
		for (auto& a : r.alt) for (auto& c : a) c = (char)toupper((unsigned char)c);   // (as VcfFile::load stores them)
		const Variant v = Variant::fromVcf(r);
		*start = v.start; *end = v.end;
		snprintf(ref_out, 64, "%s", v.ref.c_str()); snprintf(obs_out, 64, "%s", v.obs.c_str());
		*reg_first = *reg_second = -1;
		if (!v.isSNV())
		{
			FastaFileIndex g(fasta); const Chromosome c(chr);
			const std::pair<int, int> reg = variantIndelRegion(v.start, v.end, v.ref, v.obs, [&](int p, int l) { return g.seq(c, p, l); });
			*reg_first = reg.first; *reg_second = reg.second;
		}
		return 0;
	}
	catch (std::exception& e) { return fail(e, err, err_cap); }
}

// The variant table of BamRemoveVariants (host/RmVariants.hpp: loadRmVariants) for the references of a BAM in tid order. out: rows (tid or -1, beg, end, start, kind,
// ref, obs), one per data line in file order. Returns the number of lines (also when it exceeds cap), -1 on an error (message in err).
long long ngsbits_rm_variants(const char* vcf_path, const char* const* ref_names, int n_ref, int* out, long long cap, char* err, int err_cap)
{
	try
	{
		const RmVariantTable t = loadRmVariants(vcf_path, std::vector<std::string>(ref_names, ref_names + n_ref));
		for (long long i = 0; i < (long long)t.lines.size() && i < cap; ++i)
		{
			const ngsqc_rm_variant& v = t.lines[(size_t)i];
			int* o = out + 7 * i;
			o[0] = v.tid; o[1] = v.beg; o[2] = v.end; o[3] = v.start; o[4] = v.kind; o[5] = v.ref; o[6] = v.obs;
		}
		return (long long)t.lines.size();
	}
	catch (std::exception& e) { return fail(e, err, err_cap); }
}

// The three summary lines of BamClipOverlap for the counts of ngsqc_clip_overlap (host/ClipOverlap.hpp), as the tool prints them. Returns the length of the text
// (also when it exceeds cap), -1 with the "Lost Reads" message in err when a read is missing.
long long ngsbits_clip_summary(const long long* counts, char* out, long long cap, char* err, int err_cap)
{
	int64_t c[6]; for (int i = 0; i < 6; ++i) c[i] = counts[i];
	std::string lost; const std::string text = clipSummary(c, lost);
	if (!lost.empty()) { if (err && err_cap > 0) { strncpy(err, lost.c_str(), (size_t)err_cap - 1); err[err_cap - 1] = 0; } return -1; }
	if (out && cap > 0) { strncpy(out, text.c_str(), (size_t)cap - 1); out[cap - 1] = 0; }
	return (long long)text.size();
}
// The text of a FASTQ file as ReadQC's reader delivers it (host/FastqReader.hpp: gzip with any number of members, BGZF, plain text), read in pieces of `piece`
// bytes and laid end to end in out. Returns the length of the text (also when it exceeds cap: then out holds its first cap bytes), -1 on an error (message in
// err). *n_pieces: the pieces delivered.
long long ngsbits_fastq_text(const char* path, long long piece, unsigned char* out, long long cap, long long* n_pieces, char* err, int err_cap)
{
	try
	{
		if (piece <= 0) NB_THROW(ArgumentException, "piece size must be positive");
		FastqTextReader r(path);
		std::vector<uint8_t> buf((size_t)piece);
		long long total = 0, pieces = 0;
		for (;;)
		{
			const size_t n = r.read(buf.data(), buf.size());
			if (n == 0) break;
			if (total < cap) memcpy(out + total, buf.data(), (size_t)std::min<long long>((long long)n, cap - total));
			total += (long long)n; ++pieces;
		}
		if (n_pieces) *n_pieces = pieces;
		return total;
	}
	catch (std::exception& e) { return fail(e, err, err_cap); }
}
}
