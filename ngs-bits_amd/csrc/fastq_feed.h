// The input side of the accumulators that take FASTQ text in pieces cut anywhere and write FASTQ again (ngsqc_purge in purge.hip, ngsqc_fqedit in fqedit.hip;
// their output side is fastq_outputs.h): FastqFeed - the text of one, two or three sides, its carry, the line index on the device (launch_fastq_line_index of
// fastqin.hip) and the entries of a feed. The plan kernels, the statistics and what a surplus on one side means stay with the caller; nothing here asks who
// calls. ngsqc_fastq (fastqin.hip) keeps its own pipeline of two pinned slots and takes fastq_text.h, fq_fetch_entry and fastq_guard only - which is why this
// header needs handle.h alone: join.h's kernels and rocPRIM in fastqin.hip's code object made the first line index of a process 6 to 8 ms slower.
#pragma once
#include "handle.h"
#include "fastq_text.h"

namespace ngsqc { namespace lib {
namespace {
// the four lines of entry r of a text of n_lines lines: its offsets from the device's index, the bytes from the host's copy of the text (waits for the stream)
void fq_fetch_entry(const uint8_t* text, const uint32_t* d_lines, uint64_t n_lines, uint64_t r, hipStream_t stream, std::string ln[4])
{
	std::vector<uint32_t> lo(fq_entry_offsets(r, n_lines));
	HIPCHK(hipMemcpyAsync(lo.data(), d_lines + 4 * r, lo.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, stream)); HIPCHK(hipStreamSynchronize(stream));
	fq_entry_lines(text, lo, ln);
}

// an entry point of an accumulator: exceptions -> return code + message (in the accumulator, or in the thread's own string while there is none)
template <typename H, typename F> int fastq_guard(H* h, std::string& fallback, F&& body)
{
	std::string& err = h ? h->err : fallback;
	try { return body(); }
	catch (FormatError& e) { err = e.what(); return NGSQC_E_FORMAT; }
	catch (ArgError& e) { err = e.what(); return NGSQC_E_ARG; }
	catch (IoError& e) { err = e.what(); return NGSQC_E_IO; }
	catch (std::exception& e) { err = e.what(); return NGSQC_E_DEVICE; }
}

struct FastqFeed
{
	int sides = 1, device = 0; hipStream_t stream = nullptr;
	hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
	struct Side
	{
		std::vector<uint8_t> text;   // the carry, then what was fed
		size_t n_idx = 0; int64_t blocks = 0; unsigned long long L = 0, E = 0;   // of the last feed: bytes indexed, their blocks, their lines, the entries they make
		DevBuf<uint8_t> d_text, d_tmp; DevBuf<uint32_t> d_cnt, d_lines; DevBuf<int64_t> d_base;
	} side[3];

	void open(int dev, int n_sides)
	{
		int n_dev = 0;
		if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) throw std::runtime_error("no HIP device available (libngsqc_hip has no CPU fallback)");
		if (dev < 0 || dev >= n_dev) throw ArgError("no such device");
		if (n_sides < 1 || n_sides > 3) throw ArgError("a FASTQ feed has one to three sides");
		device = dev; sides = n_sides;
		HIPCHK(hipSetDevice(device));
		HIPCHK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
		for (auto& e : ev) HIPCHK(hipEventCreate(&e));
	}
	~FastqFeed()
	{
		(void)hipSetDevice(device);
		if (stream) { (void)hipStreamSynchronize(stream); (void)hipStreamDestroy(stream); }
		for (auto& e : ev) if (e) (void)hipEventDestroy(e);
	}
	// The pieces go behind the carries; every side is uploaded and indexed. Returns the entries complete on every side (entry r is lines 4r .. 4r + 3 of
	// side k in side[k].d_text / d_lines, side[k].L lines), or -1 when no line ends in these pieces: nothing new can be complete, nothing was indexed and
	// there is no carry to cut. who: the entry point, for the message. tx, nn: one per side. Behind the last piece the file has ended: the carries are empty,
	// the line phase starts again, and a further feed begins the next file.
	int64_t feed(const char* who, const uint8_t* const* tx, const int64_t* nn, bool last, double& h2d_ms, double& index_ms, double& wait_ms)
	{
		bool any_newline = false;
		for (int k = 0; k < sides; ++k)
		{
			if (side[k].text.size() + (size_t)nn[k] + 1 >= ((size_t)1 << 31)) throw ArgError(std::string(who) + ": a piece and the carry in front of it must stay below 2 GiB");
			if (nn[k]) { any_newline |= memchr(tx[k], '\n', (size_t)nn[k]) != nullptr; side[k].text.insert(side[k].text.end(), tx[k], tx[k] + nn[k]); }
		}
		if (!last && !any_newline) return -1;
		HIPCHK(hipEventRecord(ev[0], stream));
		for (int k = 0; k < sides; ++k)
		{
			Side& s = side[k];
			if (last && !s.text.empty() && s.text.back() != '\n') s.text.push_back('\n');   // a file need not end with a newline
			s.n_idx = fq_strip_empty_lines(s.text.data(), s.text.size());                   // empty lines at the end wait in the carry; behind the last piece they are dropped
			if (last) s.text.resize(s.n_idx);
			s.blocks = (int64_t)((s.n_idx + FQ_BLOCK - 1) / FQ_BLOCK);
			s.d_text.ensure_slack((size_t)std::max<int64_t>(s.blocks, 1) * FQ_BLOCK); s.d_cnt.ensure_slack((size_t)s.blocks + 1); s.d_base.ensure_slack((size_t)s.blocks + 2);
			s.d_tmp.ensure_slack(scan_tmp_bytes(s.blocks) + 64); s.d_lines.ensure_slack(s.n_idx + 2);
			if (s.n_idx) HIPCHK(hipMemcpyAsync(s.d_text.p, s.text.data(), s.n_idx, hipMemcpyHostToDevice, stream));
		}
		HIPCHK(hipEventRecord(ev[1], stream));
		for (int k = 0; k < sides; ++k) { Side& s = side[k]; launch_fastq_line_index(s.d_text.p, s.n_idx, s.d_cnt.p, s.d_base.p, s.d_tmp.p, s.d_lines.p, stream); }
		HIPCHK(hipEventRecord(ev[2], stream));
		int64_t tot[3] = {0, 0, 0};
		for (int k = 0; k < sides; ++k) HIPCHK(hipMemcpyAsync(&tot[k], side[k].d_base.p + side[k].blocks, 8, hipMemcpyDeviceToHost, stream));
		const double w0 = wall_ms();
		HIPCHK(hipStreamSynchronize(stream));
		wait_ms += wall_ms() - w0;
		for (int k = 0; k < sides; ++k) { side[k].L = (unsigned long long)tot[k]; side[k].E = last ? (side[k].L + 3) / 4 : side[k].L / 4; }
		float ms = 0;
		HIPCHK(hipEventElapsedTime(&ms, ev[0], ev[1])); h2d_ms += ms;
		HIPCHK(hipEventElapsedTime(&ms, ev[1], ev[2])); index_ms += ms;
		unsigned long long n = side[0].E;
		for (int k = 1; k < sides; ++k) n = std::min(n, side[k].E);
		return (int64_t)n;
	}
	// The carry behind the n entries the feed gave: what lies behind line 4n - 1 stays as the side's text, nothing behind the last piece. Bit k of the result: side k
	// holds at least one more line. Behind the last piece that is text the caller has to decide about: the empty lines at the end are stripped, so the last line of
	// the index is not empty, and a line at or behind 4n means at least one more, maybe incomplete, entry. It is what reading lines[4n] back and comparing it
	// with n_idx would say, without the wait: the stripped text is empty or ends with '\n', so lines[L] = n_idx, while for 4n < L line 4n starts in front of its
	// own '\n', which lies in front of n_idx. (4n > L: the last entry is incomplete and took its missing lines as empty; nothing is left.)
	int cut_carry(int64_t n, bool last)
	{
		int rest = 0;
		for (int k = 0; k < sides; ++k)
		{
			Side& s = side[k];
			if (4ull * (unsigned long long)n < s.L) rest |= 1 << k;
			if (last) { s.text.clear(); continue; }
			uint32_t from = 0;   // (not last: n <= L / 4, so lines[4n] is in the index; lines[L] is the byte behind the last '\n')
			HIPCHK(hipMemcpyAsync(&from, s.d_lines.p + 4 * n, sizeof(uint32_t), hipMemcpyDeviceToHost, stream)); HIPCHK(hipStreamSynchronize(stream));
			s.text.erase(s.text.begin(), s.text.begin() + (ptrdiff_t)std::min<size_t>(from, s.text.size()));
		}
		return rest;
	}
	// the four lines of entry r of side k of the last feed, for the reference's messages
	void entry_lines(int k, uint64_t r, std::string ln[4]) { fq_fetch_entry(side[k].text.data(), side[k].d_lines.p, side[k].L, r, stream, ln); }
};
} // namespace
}} // namespace ngsqc::lib
