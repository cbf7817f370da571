// SeqPurge - drop-in for src/SeqPurge/main.cpp on the MI355X path: same flags, defaults, help text, messages and outputs. AnalysisWorker::run and the routing of
// OutputWorker::run are on the GPU (ngsqc_purge_feed: csrc/purge.hip), which also formats and deflates the output files; the input files are inflated here, on
// the host, each in1[i] / in2[i] pair in step so that neither side runs far ahead of the other. The summary (Auxilary.h:166-221, :238-269) is written here from
// the library's counters. -qc: the same text goes into a raw-read accumulator (ngsqc_fastq_feed), in1[i] while the pair is read and in2[i] from a second
// reading of that file (one accumulator holds one open file), and the qcML lists in1 and then in2 as its source files (ThreadCoordinator.cpp:138-141).
// -threads, -block_size, -block_prefetch, -progress and -debug are accepted and change nothing.
#include "Statistics.hpp"
#include "FastqReader.hpp"
#include <ctime>
using namespace ngsbits;

namespace {
constexpr size_t PIECE = (size_t)16 << 20;   // text bytes per side and ngsqc_purge_feed

std::string dateTime()
{
	char b[64]; const time_t t = time(nullptr); struct tm tmv; localtime_r(&t, &tmv);
	strftime(b, sizeof(b), "%Y-%m-%dT%H:%M:%S", &tmv);
	return b;
}
std::string rjust4(long long v) { char b[32]; snprintf(b, sizeof(b), "%4lld", v); return b; }
// the consensus of the first 40 adapter bases (Auxilary.h:181-193)
std::string consensus(const int64_t* pile)
{
	std::string s;
	for (int i = 0; i < 40; ++i)
	{
		const int64_t a = pile[5 * i], c = pile[5 * i + 1], g = pile[5 * i + 2], t = pile[5 * i + 3];
		const int64_t depth = a + c + g + t;
		if (depth < 20) break;
		const int64_t mx = std::max(std::max(a, c), std::max(g, t));
		if ((double)mx / depth <= 0.5) s += 'N';
		else if (a == mx) s += 'A';
		else if (c == mx) s += 'C';
		else if (g == mx) s += 'G';
		else if (t == mx) s += 'T';
	}
	return s;
}
// rows first .. the last non-zero index; a histogram that is all zero has none (the reference walks below index 0 there)
void histogram(std::string& out, const int64_t* h, int first)
{
	int max = 999;
	while (max >= 0 && h[max] == 0) --max;
	for (int i = first; i <= max; ++i) out += rjust4(i) + ": " + std::to_string(h[i]) + "\n";
}
std::string percent(double x, int64_t n) { return number(100.0 * x / (double)n, 2); }
} // namespace

class ConcreteTool : public ToolBase
{
public:
	ConcreteTool(int argc, char** argv) : ToolBase(argc, argv) {}
	void setup() override
	{
		setDescription("Removes adapter sequences from paired-end sequencing data.");
		addInfileList("in1", "Forward input gzipped FASTQ file(s).", false);
		addInfileList("in2", "Reverse input gzipped FASTQ file(s).", false);
		addOutfile("out1", "Forward output gzipped FASTQ file.", false);
		addOutfile("out2", "Reverse output gzipped FASTQ file.", false);
		// optional
		addString("a1", "Forward adapter sequence (at least 15 bases).", true, "AGATCGGAAGAGCACACGTCTGAACTCCAGTCA");
		addString("a2", "Reverse adapter sequence (at least 15 bases).", true, "AGATCGGAAGAGCGTCGTGTAGGGAAAGAGTGT");
		addFloat("match_perc", "Minimum percentage of matching bases for sequence/adapter matches.", true, 80.0);
		addFloat("mep", "Maximum error probability of insert and adapter matches.", true, 0.000001);
		addInt("qcut", "Quality trimming cutoff for trimming from the end of reads using a sliding window approach. Set to 0 to disable.", true, 15);
		addInt("qwin", "Quality trimming window size.", true, 5);
		addInt("qoff", "Quality trimming FASTQ score offset.", true, 33);
		addInt("ncut", "Number of subsequent Ns to trimmed using a sliding window approach from the front of reads. Set to 0 to disable.", true, 7);
		addInt("min_len", "Minimum read length after adapter trimming. Shorter reads are discarded.", true, 30);
		addInt("threads", "The number of threads used for trimming (up to three additional threads are used for reading and writing).", true, 1);
		addOutfile("out3", "Name prefix of singleton read output files (if only one read of a pair is discarded).", true);
		addOutfile("summary", "Write summary/progress to this file instead of STDOUT.", true);
		addOutfile("qc", "If set, a read QC file in qcML format is created (just like ReadQC).", true);
		addInt("block_size", "Number of FASTQ entries processed in one block.", true, 10000);
		addInt("block_prefetch", "Number of blocks that may be pre-fetched into memory.", true, 32);
		addFlag("ec", "Enable error-correction of adapter-trimmed reads (only those with insert match).");
		addFlag("debug", "Enables debug output (use only with one thread).");
		addInt("progress", "Enables progress output at the given interval in milliseconds (disabled by default).", true, -1);
		addInt("compression_level", "Output FASTQ compression level from 1 (fastest) to 9 (best compression).", true, 1);
		// --changelog (src/SeqPurge/main.cpp)
		changeLog(2022, 7, 15, "Improved scaling with more than 4 threads and CPU usage.");
		changeLog(2019, 3, 26, "Added 'compression_level' parameter.");
		changeLog(2019, 2, 11, "Added writer thread to make SeqPurge scale better when using many threads.");
		changeLog(2017, 6, 15, "Changed default value of 'min_len' parameter from 15 to 30.");
		changeLog(2016, 8, 10, "Fixed bug in binomial calculation (issue #1).");
		changeLog(2016, 4, 15, "Removed large part of the overtrimming described in the paper (~75% of reads overtrimmed, ~50% of bases overtrimmed).");
		changeLog(2016, 4, 6, "Added error correction (optional).");
		changeLog(2016, 3, 16, "Version used in the SeqPurge paper: http://bmcbioinformatics.biomedcentral.com/articles/10.1186/s12859-016-1069-7");
	}
	void checkPurge(ngsqc_purge* p, int rc)
	{
		if (rc == NGSQC_OK) return;
		const std::string m = ngsqc_purge_last_error(p);
		if (rc == NGSQC_E_FORMAT) { if (m.compare(0, 5, "File ") == 0) NB_THROW(FileParseException, m); NB_THROW(ArgumentException, m); }
		if (rc == NGSQC_E_IO) NB_THROW(FileAccessException, m);
		if (rc == NGSQC_E_ARG) NB_THROW(CommandLineParsingException, m);
		NB_THROW(ProgrammingException, m);
	}
	void checkFastq(ngsqc_fastq* acc, int rc)
	{
		if (rc == NGSQC_E_FORMAT) NB_THROW(FileParseException, ngsqc_fastq_last_error(acc));
		if (rc != NGSQC_OK) NB_THROW(ProgrammingException, ngsqc_fastq_last_error(acc));
	}
	void main() override
	{
		const double t_start = now_s();
		const std::vector<std::string> in1 = getInfileList("in1"), in2 = getInfileList("in2");
		if (in1.size() != in2.size()) NB_THROW(CommandLineParsingException, "Input file lists 'in1' and 'in2' differ in counts!");
		const std::string a1 = trimmed(getString("a1")), a2 = trimmed(getString("a2"));
		if (a1.size() < 15) NB_THROW(CommandLineParsingException, "Forward adapter " + a1 + " too short!");
		if (a2.size() < 15) NB_THROW(CommandLineParsingException, "Reverse adapter " + a2 + " too short!");
		ngsqc_purge_params pp{};
		pp.a1 = a1.c_str(); pp.a2 = a2.c_str(); pp.match_perc = getFloat("match_perc"); pp.mep = getFloat("mep"); pp.min_len = getInt("min_len");
		pp.qcut = getInt("qcut"); pp.qwin = getInt("qwin"); pp.qoff = getInt("qoff"); pp.ncut = getInt("ncut"); pp.ec = getFlag("ec") ? 1 : 0;
		const std::string out3 = getOutfile("out3"), summary = getOutfile("summary"), qc = getOutfile("qc");
		FILE* sum = stdout;
		if (!summary.empty()) { sum = fopen(summary.c_str(), "wb"); if (!sum) NB_THROW(FileAccessException, "Could not open file for writing: '" + summary + "'!"); }
		stamp("arguments");
		ngsqc_purge* p = nullptr;
		{ const int rc = ngsqc_purge_create(0, &pp, &p); if (rc != NGSQC_OK) checkPurge(nullptr, rc); }
		std::unique_ptr<ngsqc_purge, void (*)(ngsqc_purge*)> guard(p, ngsqc_purge_destroy);
		const std::string o3a = out3 + "_R1.fastq.gz", o3b = out3 + "_R2.fastq.gz";
		checkPurge(p, ngsqc_purge_outputs(p, getOutfile("out1").c_str(), getOutfile("out2").c_str(), out3.empty() ? nullptr : o3a.c_str(), out3.empty() ? nullptr : o3b.c_str(), getInt("compression_level")));
		ngsqc_fastq* acc = nullptr;
		if (!qc.empty() && ngsqc_fastq_create(0, 0, &acc) != NGSQC_OK) NB_THROW(ProgrammingException, ngsqc_fastq_last_error(nullptr));
		std::unique_ptr<ngsqc_fastq, void (*)(ngsqc_fastq*)> qguard(acc, ngsqc_fastq_destroy);
		stamp("device");
		std::vector<uint8_t> b1(PIECE), b2(PIECE);
		double inflate_s = 0; int64_t text_bytes = 0;
		for (size_t i = 0; i < in1.size(); ++i)
		{
			checkPurge(p, ngsqc_purge_file_names(p, in1[i].c_str(), in2[i].c_str()));
			FastqTextReader r1(in1[i]), r2(in2[i]);
			for (;;)
			{
				const double t0 = now_s();
				const size_t n1 = r1.read(b1.data(), b1.size()), n2 = r2.read(b2.data(), b2.size());
				inflate_s += now_s() - t0;
				if (n1 == 0 && n2 == 0) break;
				checkPurge(p, ngsqc_purge_feed(p, b1.data(), (int64_t)n1, b2.data(), (int64_t)n2, 0));
				if (acc && n1) checkFastq(acc, ngsqc_fastq_feed(acc, b1.data(), (int64_t)n1, 0, 0));
				text_bytes += (int64_t)(n1 + n2);
			}
			checkPurge(p, ngsqc_purge_feed(p, nullptr, 0, nullptr, 0, 1));
			if (acc)
			{
				checkFastq(acc, ngsqc_fastq_feed(acc, nullptr, 0, 0, 1));
				FastqTextReader again(in2[i]);
				for (;;)
				{
					const double t0 = now_s();
					const size_t n = again.read(b2.data(), b2.size());
					inflate_s += now_s() - t0;
					if (n == 0) break;
					checkFastq(acc, ngsqc_fastq_feed(acc, b2.data(), (int64_t)n, 1, 0));
				}
				checkFastq(acc, ngsqc_fastq_feed(acc, nullptr, 0, 1, 1));
			}
		}
		std::unique_ptr<ngsqc_purge_stats> st(new ngsqc_purge_stats);
		checkPurge(p, ngsqc_purge_result(p, st.get()));
		stamp("inflate, copy, kernels and outputs");
		if (getenv("NGSQC_TIMING"))
			fprintf(stderr, "[ngsqc] SeqPurge: %lld pairs, %lld text bytes in pieces of %zu per side; host inflate %.1f ms (1 thread), H2D %.1f ms, line index %.1f ms, plan kernel %.1f ms, "
			                "format kernels %.1f ms, deflate and copy-out %.1f ms, host waited %.1f ms for the device\n",
			        (long long)st->pairs, (long long)text_bytes, PIECE, inflate_s * 1e3, st->h2d_ms, st->index_ms, st->plan_ms, st->format_ms, st->deflate_ms, st->wait_ms);
		// ---- the summary (ThreadCoordinator.cpp:133-150)
		std::string s = dateTime() + " writing statistics summary\n";
		const int64_t n = st->read_num;
		const int64_t trimmed_reads = st->reads_trimmed_insert + st->reads_trimmed_adapter;
		s += "Reads (forward + reverse): " + std::to_string(n) + "\n\n";
		s += "Reads trimmed by insert match: " + std::to_string(st->reads_trimmed_insert) + "\n";
		s += "Reads trimmed by adapter match: " + std::to_string(st->reads_trimmed_adapter) + "\n";
		s += "Reads trimmed by quality: " + std::to_string(st->reads_trimmed_q) + "\n";
		s += "Reads trimmed by N stretches: " + std::to_string(st->reads_trimmed_n) + "\n";
		s += "Trimmed reads: " + std::to_string(trimmed_reads) + " of " + std::to_string(n) + " (" + percent((double)trimmed_reads, n) + "%)\n";
		s += "Removed reads: " + std::to_string(st->reads_removed) + " of " + std::to_string(n) + " (" + percent((double)st->reads_removed, n) + "%)\n";
		s += "Removed bases: " + percent(st->bases_perc_trim_sum, n) + "%\n\n";
		s += "Forward adapter sequence (given)    : " + a1 + "\n";
		s += "Forward adapter sequence (consensus): " + consensus(st->acons) + "\n";
		s += "Reverse adapter sequence (given)    : " + a2 + "\n";
		s += "Reverse adapter sequence (consensus): " + consensus(st->acons + 200) + "\n\n";
		s += "Read length distribution after trimming:\n";
		histogram(s, st->bases_remaining, 0);
		if (acc)
		{
			StatisticsReads stats(false);
			stats.update(acc);
			std::vector<std::string> sources = in1; sources.insert(sources.end(), in2.begin(), in2.end());
			stats.getResult().storeToQCML(qc, sources, "", "SeqPurge", version());
		}
		if (pp.ec)
		{
			if (getInt("progress") > 0) s += dateTime() + " writing error corrections summary\n";
			s += "\nRead error per cycle (read 1):\n"; histogram(s, st->ec_mismatch_r1, 1);
			s += "\nRead error per cycle (read 2):\n"; histogram(s, st->ec_mismatch_r2, 1);
			s += "\nRead error count distribution:\n"; histogram(s, st->ec_errors_per_read, 1);
		}
		char el[64]; snprintf(el, sizeof(el), "%.3fs", now_s() - t_start);
		s += dateTime() + " overall runtime: " + el + "\n";
		fwrite(s.data(), 1, s.size(), sum);
		if (sum != stdout) fclose(sum);
		stamp("summary");
	}
};
int main(int argc, char** argv) { ConcreteTool tool(argc, argv); return tool.execute(); }
