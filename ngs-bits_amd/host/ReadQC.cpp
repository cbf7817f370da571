// ReadQC - drop-in for src/ReadQC/main.cpp on the MI355X path: same flags, defaults, help text, messages and outputs. The loop of main() (:57-96:
// FastqFileStream::readEntry with validation, StatisticsReads::update(entry, direction)) runs on the GPU (ngsqc_fastq_feed: csrc/fastqin.hip); the files are
// inflated here, on the host, by one thread, one file after the other in the reference's order (in1[i] wholly before in2[i]: the first error is the
// reference's). -out1 / -out2 are deflated on the GPU (ngsqc_bgzf_compress_level) into BGZF files (valid gzip) whose decompressed text is the reference's.
#include "Statistics.hpp"
#include "FastqReader.hpp"
using namespace ngsbits;

namespace {
constexpr size_t PIECE = (size_t)32 << 20;   // text bytes per ngsqc_fastq_feed

// FastqOutfileStream (src/cppNGS/FastqFileStream.cpp:160-205) for entries that arrive as text: every entry as its four lines, each followed by "\n" - so "\r"
// in front of a newline goes, an unfinished last line is finished, the empty lines at the end of an input file go and an incomplete last entry is filled up.
class FastqGzWriter
{
public:
	FastqGzWriter(const std::string& path, int level) : path_(path), level_(level)
	{
		f_ = fopen(path.c_str(), "wb");
		if (!f_) NB_THROW(FileAccessException, "Could not open file '" + path + "' for writing!");
		if (level < 0 || level > 9) NB_THROW(ArgumentException, "Invalid gzip compression level '" + std::to_string(level) + "' given for FASTQ file '" + path + "'!");
	}
	~FastqGzWriter() { if (f_) fclose(f_); }
	void write(const uint8_t* t, size_t n)
	{
		for (size_t i = 0; i < n; ++i)
		{
			if (t[i] != '\n') { line_.push_back((char)t[i]); continue; }
			end_line();
		}
		if (text_.size() >= WINDOW) flush(false);
	}
	void end_file()
	{
		if (!line_.empty()) end_line();
		held_ = 0;
		while (lines_ % 4) { text_ += '\n'; ++lines_; }
	}
	void close()
	{
		flush(true);
		static const uint8_t eof[28] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43, 0x02, 0, 0x1b, 0, 0x03, 0, 0, 0, 0, 0, 0, 0, 0, 0};   // the BGZF end-of-file member (SAM spec 4.1.2)
		put(eof, sizeof(eof));
		if (fclose(f_) != 0) { f_ = nullptr; NB_THROW(FileAccessException, "Could not write to file '" + path_ + "'!"); }
		f_ = nullptr;
	}
private:
	static constexpr size_t MEMBER = 0xff00, WINDOW = 1024 * MEMBER;
	void end_line()
	{
		if (!line_.empty() && line_.back() == '\r') line_.pop_back();
		if (line_.empty()) { ++held_; return; }
		text_.append(held_, '\n'); lines_ += held_; held_ = 0;
		text_ += line_; text_ += '\n'; ++lines_; line_.clear();
	}
	void put(const uint8_t* p, size_t n) { if (n && fwrite(p, 1, n, f_) != n) NB_THROW(FileAccessException, "Could not write to file '" + path_ + "'!"); }
	void flush(bool all)   // whole members, so that the file does not depend on where the windows end
	{
		const size_t n = all ? text_.size() : text_.size() / MEMBER * MEMBER;
		if (!n) return;
		out_.resize((n + MEMBER - 1) / MEMBER * 65536);
		size_t got = 0;
		const int rc = ngsqc_bgzf_compress_level(text_.data(), n, 0, level_, out_.data(), out_.size(), &got);
		if (rc != NGSQC_OK) NB_THROW(ProgrammingException, "ngsqc_bgzf_compress_level failed for file '" + path_ + "' (" + std::to_string(rc) + ")");
		put(out_.data(), got);
		text_.erase(0, n);
	}
	std::string path_, line_, text_; int level_; FILE* f_ = nullptr; size_t held_ = 0, lines_ = 0; std::vector<uint8_t> out_;
};
} // namespace

class ConcreteTool : public ToolBase
{
public:
	ConcreteTool(int argc, char** argv) : ToolBase(argc, argv) {}
	void setup() override
	{
		setDescription("Calculates QC metrics on unprocessed NGS reads.");
		addInfileList("in1", "Forward input gzipped FASTQ file(s).", false);
		addInfileList("in2", "Reverse input gzipped FASTQ file(s) for paired-end mode (same number of cycles/reads as 'in1').", true);
		// optional
		addOutfile("out", "Output qcML file. If unset, writes to STDOUT.", true);
		addFlag("txt", "Writes TXT format instead of qcML.");
		addOutfile("out1", "If set, writes merged forward FASTQs to this file (gzipped).", true);
		addOutfile("out2", "If set, writes merged reverse FASTQs to this file (gzipped)", true);
		addInt("compression_level", "Output FASTQ compression level from 1 (fastest) to 9 (best compression).", true, 1);
		addFlag("long_read", "Support long reads (> 1kb).");
		// --changelog (src/ReadQC/main.cpp)
		changeLog(2023, 4, 18, "Added support for LongRead");
		changeLog(2021, 2, 3, "Added option to write out merged input FASTQs (out1/out2).");
		changeLog(2016, 8, 19, "Added support for multiple input files.");
	}
	// one input file into the accumulator (and the merged output); returns the entries with a header: FastqFileStream::index()
	int64_t feedFile(ngsqc_fastq* acc, const std::string& path, int direction, FastqGzWriter* out, std::vector<uint8_t>& buf)
	{
		FastqTextReader reader(path);
		auto check = [&](int rc) {
			if (rc == NGSQC_E_FORMAT) NB_THROW(FileParseException, ngsqc_fastq_last_error(acc));
			if (rc != NGSQC_OK) NB_THROW(ProgrammingException, ngsqc_fastq_last_error(acc)); };
		for (;;)
		{
			const double t0 = now_s();
			const size_t n = reader.read(buf.data(), buf.size());
			inflate_s_ += now_s() - t0;
			if (n == 0) break;
			check(ngsqc_fastq_feed(acc, buf.data(), (int64_t)n, direction, 0));
			if (out) out->write(buf.data(), n);
			text_bytes_ += (int64_t)n;
		}
		check(ngsqc_fastq_feed(acc, nullptr, 0, direction, 1));
		if (out) out->end_file();
		ngsqc_fastq_report rep{};
		check(ngsqc_fastq_result(acc, nullptr, &rep));
		return rep.entries;
	}
	void main() override
	{
		const std::vector<std::string> in1 = getInfileList("in1"), in2 = getInfileList("in2");
		if (!in2.empty() && in1.size() != in2.size()) NB_THROW(CommandLineParsingException, "Input file lists 'in1' and 'in2' differ in counts!");
		const int compression_level = getInt("compression_level");
		std::unique_ptr<FastqGzWriter> out1, out2;
		if (getOutfile("out1") != "") out1.reset(new FastqGzWriter(getOutfile("out1"), compression_level));
		if (getOutfile("out2") != "") out2.reset(new FastqGzWriter(getOutfile("out2"), compression_level));
		const bool long_read = getFlag("long_read");
		StatisticsReads stats(long_read);   // (the constructor's argument is single_end: -long_read is what switches the N50 line on, main.cpp:56)
		stamp("arguments");
		ngsqc_fastq* acc = nullptr;
		if (ngsqc_fastq_create(0, long_read ? 1 : 0, &acc) != NGSQC_OK) NB_THROW(ProgrammingException, ngsqc_fastq_last_error(nullptr));
		std::unique_ptr<ngsqc_fastq, void (*)(ngsqc_fastq*)> guard(acc, ngsqc_fastq_destroy);
		stamp("device");
		std::vector<std::string> infiles; std::vector<uint8_t> buf(PIECE);
		for (size_t i = 0; i < in1.size(); ++i)
		{
			const int64_t n1 = feedFile(acc, in1[i], 0, out1.get(), buf);
			infiles.push_back(in1[i]);
			if (i < in2.size())
			{
				const int64_t n2 = feedFile(acc, in2[i], 1, out2.get(), buf);
				if (n1 != n2) NB_THROW(ArgumentException, "Differing number of reads in file '" + in1[i] + "' and '" + in2[i] + "'!");
				infiles.push_back(in2[i]);
			}
		}
		stats.update(acc);
		stamp("inflate, copy and kernels");
		if (getenv("NGSQC_TIMING"))
		{
			ngsqc_fastq_report rep{}; ngsqc_fastq_result(acc, nullptr, &rep);
			fprintf(stderr, "[ngsqc] ReadQC: %lld text bytes in pieces of %zu; host inflate %.1f ms (1 thread), H2D %.1f ms, kernels %.1f ms, host waited %.1f ms for the device\n",
			        (long long)text_bytes_, PIECE, inflate_s_ * 1e3, rep.h2d_ms, rep.kernels_ms, rep.wait_ms);
		}
		const QCCollection metrics = stats.getResult();
		const std::string out = getOutfile("out");
		if (getFlag("txt"))
		{
			std::vector<std::string> output; metrics.appendToStringList(output);
			std::string text; for (auto& l : output) text += l + "\n";
			if (out.empty()) fwrite(text.data(), 1, text.size(), stdout);
			else { FILE* f = fopen(out.c_str(), "wb"); if (!f) NB_THROW(FileAccessException, "Could not open file for writing: '" + out + "'!"); fwrite(text.data(), 1, text.size(), f); fclose(f); }
		}
		else metrics.storeToQCML(out, infiles, "", "ReadQC", version());
		if (out1) out1->close();
		if (out2) out2->close();
		stamp("outputs");
	}
private:
	double inflate_s_ = 0; int64_t text_bytes_ = 0;
};
int main(int argc, char** argv) { ConcreteTool tool(argc, argv); return tool.execute(); }
