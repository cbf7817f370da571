// What FastqTrim, FastqExtract, FastqExtractUMI, FastqConvert, FastqExtractBarcode, FastqAddBarcode, FastqDownsample and FastqConcat share above ngsqc_fqedit_*
// (csrc/fqedit.hip): the check of FastqOutfileStream's constructor (src/cppNGS/FastqFileStream.cpp:160-172), the loop that inflates the input on the host and
// feeds its text - file by file where a tool takes lists - and the mapping of the library's return codes to the reference's exceptions. Every entry is
// planned, formatted and deflated on the GPU; the outputs are BGZF whose decompressed text is the reference's.
#pragma once
#include "Statistics.hpp"
#include "FastqReader.hpp"

namespace ngsbits {

struct FastqEditRun
{
	ngsqc_fqedit_params params{};
	std::string in1, in2, out1, out2;   // in2: FastqExtractUMI, FastqDownsample; out2: the tools with two outputs
	int compression_level = 1;
	std::vector<std::string> ids; std::vector<int32_t> id_lengths;   // FastqExtract
	// the tools that take lists of files (FastqConcat: list1; FastqAddBarcode: all three, of one length): file i of every list makes one input that ends
	// before file i + 1 begins. Empty: in1 / in2.
	std::vector<std::string> list1, list2, list3;
	// FastqDownsample
	uint32_t seed = 1; double percentage = 0; bool want_headers = false;
};
// what FastqDownsample needs beyond the statistics
struct FastqEditExtra { std::string kept_headers; int64_t side_entries[3] = {0, 0, 0}; };

inline void checkFastqEdit(ngsqc_fqedit* e, int rc)
{
	if (rc == NGSQC_OK) return;
	const std::string m = ngsqc_fqedit_last_error(e);
	if (rc == NGSQC_E_FORMAT) NB_THROW(FileParseException, m);
	if (rc == NGSQC_E_IO) NB_THROW(FileAccessException, m);
	if (rc == NGSQC_E_ARG) NB_THROW(ArgumentException, m);
	NB_THROW(ProgrammingException, m);
}

inline ngsqc_fqedit_stats runFastqEdit(const FastqEditRun& r, const char* tool, FastqEditExtra* extra = nullptr)
{
	constexpr size_t PIECE = (size_t)16 << 20;   // text bytes per side and feed
	const int op = r.params.op;
	const int sides = op == NGSQC_FQEDIT_BARCODE_ADD ? 3 : (op == NGSQC_FQEDIT_UMI || op == NGSQC_FQEDIT_DOWNSAMPLE) ? 2 : 1;
	const bool two_out = sides > 1 || op == NGSQC_FQEDIT_BARCODE_CUT;
	if (r.compression_level < 0 || r.compression_level > 9)   // (the stream of out1 is made first in every tool)
		NB_THROW(ArgumentException, "Invalid gzip compression level '" + std::to_string(r.compression_level) + "' given for FASTQ file '" + r.out1 + "'!");
	std::vector<std::string> files[3] = {r.list1, r.list2, r.list3};
	if (files[0].empty()) { files[0] = {r.in1}; files[1] = {r.in2}; }
	ngsqc_fqedit* e = nullptr;
	{ const int rc = ngsqc_fqedit_create(0, &r.params, &e); if (rc != NGSQC_OK) checkFastqEdit(nullptr, rc); }
	std::unique_ptr<ngsqc_fqedit, void (*)(ngsqc_fqedit*)> guard(e, ngsqc_fqedit_destroy);
	if (op == NGSQC_FQEDIT_EXTRACT)
	{
		std::string blob; std::vector<int32_t> len;
		for (const std::string& id : r.ids) { blob += id; len.push_back((int32_t)id.size()); }
		checkFastqEdit(e, ngsqc_fqedit_ids(e, blob.data(), len.data(), r.id_lengths.data(), (int64_t)len.size()));
	}
	if (op == NGSQC_FQEDIT_DOWNSAMPLE) checkFastqEdit(e, ngsqc_fqedit_downsample(e, r.seed, r.percentage, r.want_headers ? 1 : 0));
	checkFastqEdit(e, ngsqc_fqedit_outputs(e, r.out1.c_str(), two_out ? r.out2.c_str() : nullptr, r.compression_level));
	stamp("device");
	double inflate_s = 0; int64_t text_bytes = 0;
	std::vector<uint8_t> b[3];
	for (int k = 0; k < 3; ++k) b[k].resize(k < sides ? PIECE : 1);
	for (size_t i = 0; i < files[0].size(); ++i)
	{
		std::unique_ptr<FastqTextReader> rd[3];
		for (int k = 0; k < sides; ++k) rd[k].reset(new FastqTextReader(files[k][i]));
		for (;;)
		{
			const double t0 = now_s();
			size_t n[3] = {0, 0, 0};
			for (int k = 0; k < sides; ++k) n[k] = rd[k]->read(b[k].data(), b[k].size());
			inflate_s += now_s() - t0;
			if (n[0] + n[1] + n[2] == 0) break;
			checkFastqEdit(e, ngsqc_fqedit_feed3(e, b[0].data(), (int64_t)n[0], sides > 1 ? b[1].data() : nullptr, (int64_t)n[1], sides > 2 ? b[2].data() : nullptr, (int64_t)n[2], 0));
			text_bytes += (int64_t)(n[0] + n[1] + n[2]);
		}
		checkFastqEdit(e, ngsqc_fqedit_feed3(e, nullptr, 0, nullptr, 0, nullptr, 0, 1));   // the file (pair, triple) ends
	}
	ngsqc_fqedit_stats st{};
	checkFastqEdit(e, ngsqc_fqedit_result(e, &st));
	if (extra)
	{
		checkFastqEdit(e, ngsqc_fqedit_side_entries(e, extra->side_entries));
		if (r.want_headers) { char* t = nullptr; int64_t n = 0; checkFastqEdit(e, ngsqc_fqedit_kept_headers(e, &t, &n)); extra->kept_headers.assign(t, (size_t)n); }
	}
	stamp("inflate, copy, kernels and outputs");
	if (getenv("NGSQC_TIMING"))
		fprintf(stderr, "[ngsqc] %s: %lld entries, %lld text bytes in pieces of %zu per side; host inflate %.1f ms (1 thread), H2D %.1f ms, line index %.1f ms, plan kernel %.1f ms, "
		                "format kernels %.1f ms, deflate and copy-out %.1f ms, host waited %.1f ms for the device\n",
		        tool, (long long)st.entries, (long long)text_bytes, PIECE, inflate_s * 1e3, st.h2d_ms, st.index_ms, st.plan_ms, st.format_ms, st.deflate_ms, st.wait_ms);
	return st;
}

} // namespace ngsbits
