// The output side of the accumulators that read through FastqFeed (fastq_feed.h; ngsqc_purge in purge.hip, ngsqc_fqedit in fqedit.hip): FastqOutputs - up to
// four BGZF streams (join.h's BgzfStream) that the caller's format kernel fills window by window. The sizes and format kernels stay with the caller.
#pragma once
#include "join.h"

namespace ngsqc { namespace lib {
namespace {
// The streams live on the feed's device and stream: an accumulator declares its FastqFeed in front of its FastqOutputs, so that the outputs go first.
struct FastqOutputs
{
	const char* tool = ""; int slots = 0, device = 0; hipStream_t stream = nullptr;
	std::unique_ptr<BgzfStream> s[4]; std::string path[4]; bool opened = false, finished = false;
	DevBuf<uint64_t> d_sz[4], d_off[4]; DevBuf<uint8_t> d_scan_tmp;   // per slot: the bytes every entry gives the stream (the caller's sizes kernel) and where they go
	std::unique_ptr<Timer> placing;

	void init(const char* tool_name, int n_slots, int dev, hipStream_t st) { tool = tool_name; slots = n_slots; device = dev; stream = st; placing.reset(new Timer(stream)); }
	~FastqOutputs()
	{
		(void)hipSetDevice(device);
		if (stream) (void)hipStreamSynchronize(stream);   // (a format kernel may still fill a window)
	}
	// slot k without a path stays absent
	void open(const char* const paths[4], int64_t window_bytes, int level)
	{
		for (int k = 0; k < slots; ++k)
		{
			if (!paths[k]) continue;
			path[k] = paths[k];
			s[k].reset(new BgzfStream(tool, window_bytes, level));
			s[k]->sink.open(paths[k], std::string("Could not open file '") + paths[k] + "' for writing!");
		}
		opened = true;
	}
	// room for the sizes and positions of n entries in every slot; "sizes and positions" is timed from here: the caller's sizes kernel comes next, then write
	void begin(int64_t n)
	{
		for (int k = 0; k < slots; ++k) { grow(d_sz[k], (size_t)n + 1, "the FASTQ entries", tool); grow(d_off[k], (size_t)n + 1, "the FASTQ entries", tool); }
		grow(d_scan_tmp, scan_tmp_bytes((size_t)n, stream) + 16, "the FASTQ entries", tool);
		placing->start();
	}
	// n > 0 entries of d_sz[k] bytes behind what stream k holds: fill(k, window, ws) launches the caller's format kernel for the part of stream k that lies in
	// the window (d_off[k]: the stream positions, ws: that of the window's first byte). format_ms: the sizes and the positions, and the format kernels window
	// by window; deflate_ms: the encoder and the copy-out.
	template <typename F> void write(int64_t n, double& format_ms, double& deflate_ms, F fill)
	{
		for (int k = 0; k < slots; ++k) if (s[k]) s[k]->place(d_scan_tmp, d_sz[k].p, d_off[k].p, n, stream);
		placing->mark();
		HIPCHK(hipStreamSynchronize(stream));
		format_ms += placing->elapsed();
		StageClock clock(true, stream);
		double z0 = 0, z1 = 0;
		for (int k = 0; k < slots; ++k)
		{
			if (!s[k]) continue;
			z0 += s[k]->ms_deflate + s[k]->ms_copy;
			s[k]->emit(s[k]->placed_end(n), stream, device, [&](const Win& win, int64_t ws) { clock.mark(); fill(k, win, ws); clock.mark(); });
			HIPCHK(hipStreamSynchronize(stream));
			z1 += s[k]->ms_deflate + s[k]->ms_copy;
		}
		deflate_ms += z1 - z0;
		format_ms += clock.total();
	}
	void finish()
	{
		if (finished) return;
		finished = true;
		HIPCHK(hipSetDevice(device));
		for (int k = 0; k < 4; ++k)
		{
			if (!s[k]) continue;
			s[k]->finish(stream, device);
			if (!s[k]->sink.err.empty()) throw IoError("Could not write to file '" + path[k] + "'!");
		}
	}
};
} // namespace
}} // namespace ngsqc::lib
