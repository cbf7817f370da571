// What FastqTrim, FastqExtract, FastqExtractUMI and FastqConvert share above ngsqc_fqedit_* (csrc/fqedit.hip): the check of FastqOutfileStream's constructor
// (src/cppNGS/FastqFileStream.cpp:160-172), the loop that inflates the input on the host and feeds its text, and the mapping of the library's return codes to
// the reference's exceptions. Every entry is planned, formatted and deflated on the GPU; the outputs are BGZF whose decompressed text is the reference's.
#pragma once
#include "Statistics.hpp"
#include "FastqReader.hpp"

namespace ngsbits {

struct FastqEditRun
{
	ngsqc_fqedit_params params{};
	std::string in1, in2, out1, out2;   // in2 / out2: FastqExtractUMI only
	int compression_level = 1;
	std::vector<std::string> ids; std::vector<int32_t> id_lengths;   // FastqExtract
};

inline void checkFastqEdit(ngsqc_fqedit* e, int rc)
{
	if (rc == NGSQC_OK) return;
	const std::string m = ngsqc_fqedit_last_error(e);
	if (rc == NGSQC_E_FORMAT) NB_THROW(FileParseException, m);
	if (rc == NGSQC_E_IO) NB_THROW(FileAccessException, m);
	if (rc == NGSQC_E_ARG) NB_THROW(ArgumentException, m);
	NB_THROW(ProgrammingException, m);
}

inline ngsqc_fqedit_stats runFastqEdit(const FastqEditRun& r, const char* tool)
{
	constexpr size_t PIECE = (size_t)16 << 20;   // text bytes per side and feed
	const bool two = r.params.op == NGSQC_FQEDIT_UMI;
	if (r.compression_level < 0 || r.compression_level > 9)   // (the stream of out1 is made first in every tool)
		NB_THROW(ArgumentException, "Invalid gzip compression level '" + std::to_string(r.compression_level) + "' given for FASTQ file '" + r.out1 + "'!");
	ngsqc_fqedit* e = nullptr;
	{ const int rc = ngsqc_fqedit_create(0, &r.params, &e); if (rc != NGSQC_OK) checkFastqEdit(nullptr, rc); }
	std::unique_ptr<ngsqc_fqedit, void (*)(ngsqc_fqedit*)> guard(e, ngsqc_fqedit_destroy);
	if (r.params.op == NGSQC_FQEDIT_EXTRACT)
	{
		std::string blob; std::vector<int32_t> len;
		for (const std::string& id : r.ids) { blob += id; len.push_back((int32_t)id.size()); }
		checkFastqEdit(e, ngsqc_fqedit_ids(e, blob.data(), len.data(), r.id_lengths.data(), (int64_t)len.size()));
	}
	checkFastqEdit(e, ngsqc_fqedit_outputs(e, r.out1.c_str(), two ? r.out2.c_str() : nullptr, r.compression_level));
	stamp("device");
	double inflate_s = 0; int64_t text_bytes = 0;
	{
		FastqTextReader r1(r.in1);
		std::unique_ptr<FastqTextReader> r2(two ? new FastqTextReader(r.in2) : nullptr);
		std::vector<uint8_t> b1(PIECE), b2(two ? PIECE : 1);
		for (;;)
		{
			const double t0 = now_s();
			const size_t n1 = r1.read(b1.data(), b1.size()), n2 = two ? r2->read(b2.data(), b2.size()) : 0;
			inflate_s += now_s() - t0;
			if (n1 == 0 && n2 == 0) break;
			checkFastqEdit(e, ngsqc_fqedit_feed(e, b1.data(), (int64_t)n1, two ? b2.data() : nullptr, (int64_t)n2, 0));
			text_bytes += (int64_t)(n1 + n2);
		}
		checkFastqEdit(e, ngsqc_fqedit_feed(e, nullptr, 0, nullptr, 0, 1));
	}
	ngsqc_fqedit_stats st{};
	checkFastqEdit(e, ngsqc_fqedit_result(e, &st));
	stamp("inflate, copy, kernels and outputs");
	if (getenv("NGSQC_TIMING"))
		fprintf(stderr, "[ngsqc] %s: %lld entries, %lld text bytes in pieces of %zu per side; host inflate %.1f ms (1 thread), H2D %.1f ms, line index %.1f ms, plan kernel %.1f ms, "
		                "format kernels %.1f ms, deflate and copy-out %.1f ms, host waited %.1f ms for the device\n",
		        tool, (long long)st.entries, (long long)text_bytes, PIECE, inflate_s * 1e3, st.h2d_ms, st.index_ms, st.plan_ms, st.format_ms, st.deflate_ms, st.wait_ms);
	return st;
}

} // namespace ngsbits
