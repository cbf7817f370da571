// The mate join by read name and the windowed BGZF writer, shared by the tools that pair records and / or write compressed output (NameJoin: BamFilter pairs.hip,
// BamToFastq fastq.hip, BamDownsample downsample.hip, BamRemoveVariants rmvar.hip, BamClipOverlap clip.hip; BgzfStream: those and BamExtract extract.hip,
// BamCleanHaloplex haloplex.hip). One pass over the tiles; per tile (NameJoin):
//   1. the tool's keys kernel gives every tile record a 64-bit hash of its name (join_visit.h: the bytes in front of the first NUL; KEY_NONE: the record takes
//      no part), its source pointer and a 32-bit info word whose bit 31 says the record is kept ("passes"); val[e] = e for every entry.
//   2. sort: the open entries carried over from earlier tiles ("held", in (hash, ordinal) order) followed by the tile's records, radix-sorted by hash (rocPRIM,
//      stable: within a hash the order stays the file order).
//   3. resolve: one thread per run of equal hashes. When every name of the run is the same, the run pairs (0,1), (2,3), ... and an odd last entry stays open;
//      otherwise (a hash collision) the run is paired name by name in file order. close_of[closer] = opener entry << 1 | kept (both pass); counts[0] / [1]:
//      pairs kept / not kept.
//   4. held: the entries still open are compacted; their bytes are copied out of the tile buffer (the whole record if it passes, the name alone if not).
// BgzfStream cuts one output stream into windows of whole 0xff00-byte pieces: the tool fills a window, its whole pieces go through the encoder (deflate.hip)
// and a host thread writes the members while the next window is filled; the partial piece moves to the front. Around emit it holds what every writer does
// the same way: put_host (a header in members of its own), place / placed_end (the stream positions of a tile's items and where they end) and close (finish,
// and the error of a failed BAM write); the BAM writers (recwrite.h's open_bam) use all of them, BamToFastq place.
// scan_u64 / scan_tmp_bytes: the one checked rocPRIM exclusive sum of the join, of place and of the tools' own scans.
#pragma once
#include "handle.h"
#include "join_visit.h"
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

namespace ngsqc {
namespace {
__global__ __launch_bounds__(256) void join_resolve_kernel(const uint64_t* __restrict__ ks, const uint32_t* __restrict__ vs, int64_t N, int64_t H, const uint64_t* __restrict__ src,
                                                           const uint32_t* __restrict__ info, ResolveOut o)
{
	const int64_t stride = (int64_t)gridDim.x * blockDim.x;
	for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < N; j += stride)
	{
		const uint64_t k = ks[j];
		if (k == KEY_NONE || (j > 0 && ks[j - 1] == k)) continue;
		join_resolve_run(ks, vs, N, H, src, info, o, j);   // (join_visit.h)
	}
}

// the bytes a held entry keeps (join_visit.h held_entry_bytes)
__global__ __launch_bounds__(256) void held_bytes_kernel(const uint8_t* __restrict__ held, const uint32_t* __restrict__ vs, int64_t N, const uint64_t* __restrict__ src, const uint32_t* __restrict__ info, uint64_t* __restrict__ nb)
{
	const int64_t stride = (int64_t)gridDim.x * blockDim.x;
	for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < N; j += stride)
	{
		if (!held[j]) { nb[j] = 0; continue; }
		const uint8_t* s = (const uint8_t*)(uintptr_t)src[vs[j]];
		nb[j] = held_entry_bytes(s, (info[vs[j]] >> 31) != 0);
	}
}

__global__ __launch_bounds__(256) void held_store_kernel(const uint8_t* __restrict__ held, const uint64_t* __restrict__ hpos, const uint64_t* __restrict__ nb, const uint64_t* __restrict__ boff,
                                                         const uint32_t* __restrict__ vs, const uint64_t* __restrict__ ks, int64_t N, const uint64_t* __restrict__ src, const uint32_t* __restrict__ info,
                                                         uint8_t* __restrict__ pool, uint64_t* __restrict__ hk, uint64_t* __restrict__ hs, uint32_t* __restrict__ hi)
{
	const int lane = threadIdx.x & 63;
	const int64_t nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
	for (int64_t j = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; j < N; j += nw)
	{
		if (!held[j]) continue;
		const uint8_t* s = (const uint8_t*)(uintptr_t)src[vs[j]];
		uint8_t* d = pool + boff[j];
		for (uint64_t i = lane; i < nb[j]; i += 64) d[i] = s[i];
		if (lane == 0) { const uint64_t h = hpos[j]; hk[h] = ks[j]; hs[h] = (uint64_t)(uintptr_t)d; hi[h] = info[vs[j]]; }
	}
}

unsigned grid_for(int64_t n, int per = 256) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + per - 1) / per, 65536)); }

// compressed members to the file: two pinned buffers, a host thread writes one while the next is filled
struct FileSink
{
	FILE* f = nullptr; std::thread th; std::mutex mu; std::condition_variable cv;
	PinBuf<uint8_t> pb[2]; size_t len[2] = {0, 0}; bool full[2] = {false, false}; bool stop = false; std::string err; int next = 0;
	double write_ms = 0;
	void open(const char* path, const std::string& fail_msg)
	{
		f = fopen(path, "wb");
		if (!f) throw IoError(fail_msg);
		th = std::thread([this] { run(); });
	}
	void run()
	{
		int cur = 0;
		std::unique_lock<std::mutex> lk(mu);
		for (;;)
		{
			cv.wait(lk, [&] { return full[cur] || stop; });
			if (!full[cur]) return;
			lk.unlock();
			const double t0 = wall_ms();
			const bool ok = fwrite(pb[cur].p, 1, len[cur], f) == len[cur];
			lk.lock();
			write_ms += wall_ms() - t0;
			if (!ok && err.empty()) err = "write error";
			full[cur] = false; cur ^= 1; cv.notify_all();
		}
	}
	uint8_t* slot(size_t n)   // waits until the next buffer is free
	{
		std::unique_lock<std::mutex> lk(mu);
		cv.wait(lk, [&] { return !full[next]; });
		lk.unlock();
		pb[next].ensure(std::max<size_t>(n, 1));
		return pb[next].p;
	}
	void commit(size_t n) { { std::lock_guard<std::mutex> g(mu); len[next] = n; full[next] = true; } cv.notify_all(); next ^= 1; }
	void put_device(const uint8_t* d, size_t n, hipStream_t s)
	{
		if (!n) return;
		uint8_t* p = slot(n);
		HIPCHK(hipMemcpyAsync(p, d, n, hipMemcpyDeviceToHost, s)); HIPCHK(hipStreamSynchronize(s));
		commit(n);
	}
	void put_host(const uint8_t* h, size_t n) { if (!n) return; uint8_t* p = slot(n); memcpy(p, h, n); commit(n); }
	void finish()
	{
		{ std::lock_guard<std::mutex> g(mu); stop = true; } cv.notify_all();
		if (th.joinable()) th.join();
		if (f) { if (fclose(f) != 0 && err.empty()) err = "close error"; f = nullptr; }
	}
	~FileSink() { finish(); }
};

const uint8_t BGZF_EOF[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};

// device buffers of the join and the held set grow with the tile and with the names still open: planned against hipMemGetInfo before they are allocated
template <typename T> void grow(DevBuf<T>& b, size_t n, const char* what, const char* tool)
{
	if (b.n >= n) return;
	const size_t want = (n + n / 4 + 1024) * sizeof(T);
	size_t fr = 0, tot = 0;
	if (hipMemGetInfo(&fr, &tot) == hipSuccess && want > fr + b.n * sizeof(T))
	{
		reaper().drain();   // (memory on its way back to the driver)
		if (hipMemGetInfo(&fr, &tot) == hipSuccess && want > fr + b.n * sizeof(T))
			throw std::runtime_error(std::string(tool) + ": " + what + " does not fit in device memory (" + std::to_string(want >> 20) + " MiB needed, " + std::to_string(fr >> 20) + " MiB free)");
	}
	try { b.alloc(n + n / 4 + 1024); }
	catch (std::exception& e) { throw std::runtime_error(std::string(tool) + ": " + what + " does not fit in device memory (" + std::to_string((n * sizeof(T)) >> 20) + " MiB asked for; " + e.what() + ")"); }
}

// the checked exclusive sum into uint64 positions (rocPRIM), and the temporary bytes it asks for: tmp holds at least scan_tmp_bytes<In>(n, s) bytes
template <typename In = uint64_t> size_t scan_tmp_bytes(size_t n, hipStream_t s)
{
	size_t sb = 0;
	(void)rocprim::exclusive_scan(nullptr, sb, (const In*)nullptr, (uint64_t*)nullptr, (uint64_t)0, n, rocprim::plus<uint64_t>(), s);
	return sb;
}
template <typename In> void scan_u64(DevBuf<uint8_t>& tmp, const In* in, uint64_t* out, uint64_t init, size_t n, hipStream_t s)
{
	size_t sb = tmp.n;
	if (rocprim::exclusive_scan(tmp.p, sb, in, out, init, n, rocprim::plus<uint64_t>(), s) != hipSuccess) throw std::runtime_error("rocprim::exclusive_scan failed");
}

// A window of an output stream: the bytes [lo, hi) of obuf are written, a record at position pos (relative to obuf[0]; negative: it began in an earlier window)
// writes only what falls inside - so a record that straddles two windows is written in two launches, the same bytes each time.
struct Win { uint8_t* base; int64_t lo, hi; };
__device__ __forceinline__ void put(const Win& w, int64_t& pos, uint8_t v) { if (pos >= w.lo && pos < w.hi) w.base[pos] = v; ++pos; }

struct NameJoin
{
	const char* tool;
	DevBuf<uint64_t> key, skey, src, nb, boff, hpos, hk, hs; DevBuf<uint32_t> val, sval, info, hi; DevBuf<int64_t> close_of; DevBuf<uint8_t> held, st, tmp, pool[2];
	DevBuf<unsigned long long> counts;
	int cur_pool = 0; int64_t H = 0; uint64_t newH = 0;
	explicit NameJoin(const char* t, hipStream_t s) : tool(t) { counts.alloc(4); HIPCHK(hipMemsetAsync(counts.p, 0, 4 * sizeof(unsigned long long), s)); }
	// the entry arrays for H + n entries, the held entries in front; tmp also serves the tool's scans of up to H + n uint64 values
	void begin_tile(int64_t n, hipStream_t s)
	{
		const size_t N = (size_t)(H + n);
		const char* w = "the pair join";
		grow(key, N + 1, w, tool); grow(skey, N + 1, w, tool); grow(val, N + 1, w, tool); grow(sval, N + 1, w, tool); grow(src, N + 1, w, tool); grow(info, N + 1, w, tool);
		grow(held, N + 1, w, tool); grow(st, N + 1, w, tool); grow(close_of, (size_t)n + 1, w, tool); grow(nb, N + 1, w, tool); grow(boff, N + 1, w, tool); grow(hpos, N + 1, w, tool);
		if (H)
		{
			HIPCHK(hipMemcpyAsync(key.p, hk.p, (size_t)H * 8, hipMemcpyDeviceToDevice, s)); HIPCHK(hipMemcpyAsync(src.p, hs.p, (size_t)H * 8, hipMemcpyDeviceToDevice, s));
			HIPCHK(hipMemcpyAsync(info.p, hi.p, (size_t)H * 4, hipMemcpyDeviceToDevice, s));
		}
		if (!N) return;
		// (every temporary size first: a buffer must not be replaced while a queued kernel still uses it)
		size_t tb = 0;
		(void)rocprim::radix_sort_pairs(nullptr, tb, key.p, skey.p, val.p, sval.p, N, 0, 64, s);
		grow(tmp, std::max(tb, std::max(scan_tmp_bytes(N, s), scan_tmp_bytes<uint8_t>(N, s))) + 16, w, tool);
	}
	// after the tool's keys kernel: sort by hash and pair
	void sort_resolve(int64_t n, hipStream_t s)
	{
		const int64_t N = H + n;
		size_t tb = tmp.n;
		if (rocprim::radix_sort_pairs(tmp.p, tb, key.p, skey.p, val.p, sval.p, (size_t)N, 0, 64, s) != hipSuccess) throw std::runtime_error("rocprim::radix_sort_pairs failed");
		if (n) HIPCHK(hipMemsetAsync(close_of.p, 0xff, (size_t)n * sizeof(int64_t), s));
		HIPCHK(hipMemsetAsync(held.p, 0, (size_t)N, s));
		hipLaunchKernelGGL(join_resolve_kernel, dim3(grid_for(N)), dim3(256), 0, s, skey.p, sval.p, N, H, src.p, info.p, ResolveOut{close_of.p, held.p, st.p, counts.p}); KCHECK();
	}
	// the open entries: their bytes leave the tile buffer into the other pool (the tile buffer is overwritten by K1 later); waits for the stream once
	void keep_open(int64_t n, hipStream_t s)
	{
		const int64_t N = H + n;
		hipLaunchKernelGGL(held_bytes_kernel, dim3(grid_for(N)), dim3(256), 0, s, held.p, sval.p, N, src.p, info.p, nb.p); KCHECK();
		uint64_t hcnt[4] = {0, 0, 0, 0};
		scan_u64(tmp, nb.p, boff.p, 0, (size_t)N, s);
		scan_u64(tmp, held.p, hpos.p, 0, (size_t)N, s);
		HIPCHK(hipMemcpyAsync(&hcnt[0], boff.p + N - 1, 8, hipMemcpyDeviceToHost, s)); HIPCHK(hipMemcpyAsync(&hcnt[1], nb.p + N - 1, 8, hipMemcpyDeviceToHost, s));
		HIPCHK(hipMemcpyAsync(&hcnt[2], hpos.p + N - 1, 8, hipMemcpyDeviceToHost, s));
		uint8_t last_held = 0; HIPCHK(hipMemcpyAsync(&last_held, held.p + N - 1, 1, hipMemcpyDeviceToHost, s));
		HIPCHK(hipStreamSynchronize(s));
		hcnt[3] = last_held;
		const uint64_t pool_bytes = hcnt[0] + hcnt[1]; newH = hcnt[2] + hcnt[3];
		DevBuf<uint8_t>& np = pool[cur_pool ^ 1];
		const char* w = "the open read names (held set)";
		grow(np, (size_t)pool_bytes + 64, w, tool);
		// (the held arrays are rewritten: their old contents were copied into the entry arrays in begin_tile)
		grow(hk, (size_t)newH + 1, w, tool); grow(hs, (size_t)newH + 1, w, tool); grow(hi, (size_t)newH + 1, w, tool);
		hipLaunchKernelGGL(held_store_kernel, dim3(grid_for(N, 4)), dim3(256), 0, s, held.p, hpos.p, nb.p, boff.p, sval.p, skey.p, N, src.p, info.p, np.p, hk.p, hs.p, hi.p); KCHECK();
	}
	// after the stream has passed the last use of the tile's bytes and of the old pool
	void end_tile() { cur_pool ^= 1; H = (int64_t)newH; }
	void read_counts(unsigned long long* c, hipStream_t s) { HIPCHK(hipMemcpyAsync(c, counts.p, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s)); HIPCHK(hipStreamSynchronize(s)); }
};

// HIP-event intervals of NGSQC_TIMING, read once at the end of the call
struct StageClock
{
	bool on; hipStream_t s; std::vector<hipEvent_t> ev;
	StageClock(bool o, hipStream_t st) : on(o), s(st) {}
	void mark() { if (!on) return; hipEvent_t e; HIPCHK(hipEventCreate(&e)); HIPCHK(hipEventRecord(e, s)); ev.push_back(e); }   // (called in pairs: begin, end)
	double total()
	{
		double ms = 0;
		for (size_t i = 0; i + 1 < ev.size(); i += 2) { float v = 0; if (hipEventSynchronize(ev[i + 1]) == hipSuccess && hipEventElapsedTime(&v, ev[i], ev[i + 1]) == hipSuccess) ms += v; }
		return ms;
	}
	~StageClock() { for (hipEvent_t e : ev) (void)hipEventDestroy(e); }
};

// one output stream in windows of W bytes (NGSQC_WRITE_WINDOW_PIECES: pieces of 0xff00 bytes per window, a test hook; default about 1 GiB): its device and pinned
// memory does not depend on the size of the file or of a tile
inline int64_t write_window_bytes(int64_t pieces) { return pieces * BGZF_PIECE; }

struct BgzfStream
{
	const char* tool; int64_t W; int level; FileSink sink; BgzfDeflater z;   // (the encoder's slots grow with the largest window deflated, at most W)
	DevBuf<uint8_t> obuf, zbuf;
	int64_t carry = 0, ws = 0;   // ws: stream position of obuf[0]; obuf[0, carry) holds the partial piece in front of what comes next
	double ms_deflate = 0, ms_copy = 0;
	uint64_t tot[2] = {0, 0};   // place(): the last placed record's position and size, on the host behind the caller's next wait for the stream
	BgzfStream(const char* t, int64_t w, int lv) : tool(t), W(w), level(lv) {}
	void deflate_out(int64_t bytes, hipStream_t s, int device)   // the first `bytes` of obuf (whole pieces, or the tail at the end) to the file
	{
		if (bytes <= 0) return;
		const double t0 = wall_ms();
		grow(zbuf, bgzf_max_bytes(bytes), "the compressed output window", tool);   // (bytes <= W: bounded)
		const size_t zn = z.run(obuf.p, bytes, zbuf.p, s, device, level);
		const double t1 = wall_ms(); ms_deflate += t1 - t0;
		sink.put_device(zbuf.p, zn, s);   // (waits while both pinned buffers are still being written)
		ms_copy += wall_ms() - t1;
	}
	// obuf grows with what a window needs, up to W, keeping the partial piece in front (a small file never allocates a whole window)
	void ensure_obuf(int64_t need, hipStream_t s)
	{
		if ((int64_t)obuf.n >= need) return;
		DevBuf<uint8_t> nbf; grow(nbf, (size_t)std::min<int64_t>(W, need + need / 4), "the output window", tool);
		if (nbf.n > (size_t)W) { nbf.release(); nbf.alloc((size_t)W); }
		if (carry) HIPCHK(hipMemcpyAsync(nbf.p, obuf.p, (size_t)carry, hipMemcpyDeviceToDevice, s));
		HIPCHK(hipStreamSynchronize(s));
		std::swap(obuf.p, nbf.p); std::swap(obuf.n, nbf.n);
	}
	// the stream up to position out_end, in windows: fill(Win, ws) writes [have, w_end) of a window, whole pieces go to the encoder, the partial piece to the front
	template <typename F> void emit(int64_t out_end, hipStream_t s, int device, F fill)
	{
		for (;;)
		{
			const int64_t w_end = std::min<int64_t>(out_end, ws + W), have = ws + carry;
			if (w_end > have)
			{
				ensure_obuf(w_end - ws, s);
				fill(Win{obuf.p, have - ws, w_end - ws}, ws);
			}
			const int64_t fill_n = w_end - ws, whole = fill_n / BGZF_PIECE * BGZF_PIECE;
			if (whole)
			{
				deflate_out(whole, s, device);
				carry = fill_n - whole;
				if (carry) HIPCHK(hipMemcpyAsync(obuf.p, obuf.p + whole, (size_t)carry, hipMemcpyDeviceToDevice, s));   // (carry < one piece <= whole: no overlap)
				ws += whole;
			}
			else carry = fill_n;
			if (w_end >= out_end) break;
		}
	}
	// host bytes in front of the stream, in members of their own (a BAM header): pieces cut from the buffer's own start, at most W bytes per step, as windows
	// are whole pieces; the stream positions start behind them at 0
	void put_host(const uint8_t* p, size_t n, hipStream_t s, int device)
	{
		for (size_t o = 0; o < n; o += (size_t)W)
		{
			const size_t k = std::min(n - o, (size_t)W);
			ensure_obuf((int64_t)k, s);
			HIPCHK(hipMemcpyAsync(obuf.p, p + o, k, hipMemcpyHostToDevice, s));
			deflate_out((int64_t)k, s, device);
		}
	}
	// the stream positions off[0, n) of n > 0 items of sz[] bytes, behind the carried partial piece; the totals are queued for placed_end
	void place(DevBuf<uint8_t>& tmp, const uint64_t* sz, uint64_t* off, int64_t n, hipStream_t s)
	{
		scan_u64(tmp, sz, off, (uint64_t)(ws + carry), (size_t)n, s);
		HIPCHK(hipMemcpyAsync(&tot[0], off + n - 1, 8, hipMemcpyDeviceToHost, s)); HIPCHK(hipMemcpyAsync(&tot[1], sz + n - 1, 8, hipMemcpyDeviceToHost, s));
	}
	// the stream position behind what place() placed (after the caller's wait for the stream); n == 0: nothing was placed
	int64_t placed_end(int64_t n) const { return n ? (int64_t)(tot[0] + tot[1]) : ws + carry; }
	void finish(hipStream_t s, int device) { deflate_out(carry, s, device); carry = 0; sink.put_host(BGZF_EOF, sizeof(BGZF_EOF)); sink.finish(); }
	void close(hipStream_t s, int device, const char* path)   // finish, for a BAM: a failed write is the caller's error
	{
		finish(s, device);
		if (!sink.err.empty()) throw IoError(std::string("Could not write BAM file ") + path + ": " + sink.err);
	}
};
} // namespace
} // namespace ngsqc
