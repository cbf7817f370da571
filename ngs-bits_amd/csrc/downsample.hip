// BamDownsample on the device (src/BamDownsample/main.cpp:31-101): the keep / drop decisions of a sequential rand() stream, the mate join by read name, the
// record gather and the BGZF writer (ngsqc_downsample), and the decision stream on its own (ngsqc_downsample_keep).
//
// One pass over the tiles (stream_tiles); the join and the writer are join.h's (NameJoin, BgzfStream), the record bytes recwrite.h's. Per tile:
//   1. keys: secondary / supplementary records and single-end records get the sentinel key (a single-end record never enters the join; one byte marks it as
//      deciding); a paired record gets its name hash (NGSQC_NAME_HASH_BITS truncates it). info = output size with the pass bit always set: the join closes every
//      pair and a held opener keeps its whole record.
//   2. join: NameJoin::sort_resolve, unchanged.
//   3. ordinals: a record decides when it is single-end or closes a pair. The k-th deciding record of the FILE uses the k-th value of the stream - the only
//      sequential dependency: an exclusive scan of the deciding flag plus the 64-bit count of the decisions of earlier tiles.
//   4. keep bytes: the decisions of the tile's ordinal range from the chunked generator (KeepGen below).
//   5. sizes, scan, gather: a kept single-end record contributes its own size at its own position, a kept closer the opener and then the closer; the counts
//      are atomic adds. With want_names the kept names go through a size scan and a gather of their own into a device buffer that is copied out per tile.
//   6. held, deflate: as in pairs.hip.
//
// The generator is glibc's srand() / rand() (stdlib/random_r.c, TYPE_3): 31 words seeded by the Lehmer step 16807 x mod (2^31 - 1), then the additive recurrence
// o[i] = o[i-31] + o[i-3] mod 2^32 with the first 310 values thrown away; rand() returns o[i] >> 1. The recurrence is linear over Z/2^32, so the state e steps
// ahead is a fixed linear map of the state: with c = x^e mod (x^31 - x^28 - 1), o[n + e] = sum_j c[j] o[n + j]. The host keeps one state per chunk boundary and
// moves from one boundary to the next with the jump for CHUNK steps (31 x 31 multiply-adds: about a quarter of one per decision); on the device one lane
// walks one chunk with the 31-word ring in registers.
#include "recwrite.h"
#include "keep_stream.h"

namespace ngsqc {

namespace {
// CHUNK: the ordinals one lane walks. The time of the keep kernel is the time of ONE lane (about five instructions per value, every lane runs at once: a tile of
// 16 M decisions is 4 k lanes on 256 CUs), so it grows with CHUNK; the host's work per decision and the size of the state table fall with it. 3968 = 32 * 124
// keeps the kernel near 0.1 ms and the host below 0.3 multiply-adds per decision; 124 = 4 * 31 steps are four turns of the ring (static register indices) and
// 31 whole dwords of keep bytes (aligned stores).
constexpr int64_t CHUNK = NGSQC_DOWNSAMPLE_CHUNK;
constexpr int RING = 31, TAP = 28, TURN = 4 * RING;
static_assert(CHUNK % TURN == 0, "a chunk is whole turns of the unrolled ring");

struct RandState { uint32_t w[RING]; };   // o[n .. n + 30]: the next value is w[0] + w[28]
struct Jump { uint32_t c[RING]; };        // x^e mod (x^31 - x^28 - 1) over Z/2^32

RandState seed_state(uint32_t seed)   // srandom_r: seed 0 is seed 1; the words as int32, division towards zero
{
	uint32_t o[344];
	int32_t word = seed ? (int32_t)seed : 1;
	o[0] = (uint32_t)word;
	for (int i = 1; i < RING; ++i)
	{
		const int32_t hi = word / 127773, lo = word % 127773;
		word = 16807 * lo - 2836 * hi;
		if (word < 0) word += 2147483647;
		o[i] = (uint32_t)word;
	}
	for (int i = 31; i < 34; ++i) o[i] = o[i - 31];
	for (int i = 34; i < 344; ++i) o[i] = o[i - 31] + o[i - 3];
	RandState s;
	for (int i = 0; i < RING; ++i) s.w[i] = o[313 + i];
	return s;
}

Jump jump_mul(const Jump& a, const Jump& b)
{
	uint32_t t[2 * RING - 1] = {0};
	for (int i = 0; i < RING; ++i) for (int j = 0; j < RING; ++j) t[i + j] += a.c[i] * b.c[j];
	for (int d = 2 * RING - 2; d >= RING; --d) { t[d - 3] += t[d]; t[d - RING] += t[d]; }   // x^d = x^(d-3) + x^(d-31)
	Jump r;
	for (int i = 0; i < RING; ++i) r.c[i] = t[i];
	return r;
}

Jump jump_pow(uint64_t e)
{
	Jump r{}, x{};
	r.c[0] = 1; x.c[1] = 1;
	for (; e; e >>= 1) { if (e & 1) r = jump_mul(r, x); x = jump_mul(x, x); }
	return r;
}

RandState jump_apply(const Jump& j, const RandState& s)
{
	uint32_t ext[2 * RING - 1];
	for (int i = 0; i < RING; ++i) ext[i] = s.w[i];
	for (int i = RING; i < 2 * RING - 1; ++i) ext[i] = ext[i - RING] + ext[i - 3];
	RandState r;
	for (int k = 0; k < RING; ++k) { uint32_t v = 0; for (int i = 0; i < RING; ++i) v += j.c[i] * ext[i + k]; r.w[k] = v; }
	return r;
}

// The smallest T with: r < T exactly when Helper::randomNumber(0, 100) < percentage for the rand() value r. cppCORE is not part of the reference tree at hand, so
// randomNumber(min, max) is taken as min + (double)rand() / RAND_MAX * (max - min); the expected log of the reference's own test (BamDownsample_out1_Linux.txt:
// 30 kept pairs of 160 at 20 % behind srand(1)) is what pins the formula. It is monotonic in r: a bisection, once, on the host; the kernel compares integers.
uint32_t keep_threshold(double percentage)
{
	uint64_t lo = 0, hi = 1ull << 31;   // kept for every r < lo, not kept for every r >= hi
	while (lo < hi)
	{
		const uint64_t m = (lo + hi) >> 1;
		if (0.0 + (double)m / 2147483647.0 * 100.0 < percentage) lo = m + 1; else hi = m;
	}
	return (uint32_t)lo;
}

// states: word-major [31][n_chunks] (the lanes of a wave read neighbouring words); keep: CHUNK bytes per chunk, 1 = kept
__global__ __launch_bounds__(64) void ds_keep_kernel(const uint32_t* __restrict__ states, int64_t n_chunks, uint32_t T, uint32_t* __restrict__ keep)
{
	const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (c >= n_chunks) return;
	uint32_t r[RING];
#pragma unroll
	for (int j = 0; j < RING; ++j) r[j] = states[(int64_t)j * n_chunks + c];
	uint32_t* out = keep + c * (CHUNK / 4);
	for (int it = 0; it < (int)(CHUNK / TURN); ++it)
	{
#pragma unroll
		for (int q = 0; q < RING; ++q)   // (unrolled: every ring index below is a constant, the ring stays in registers)
		{
			uint32_t pack = 0;
#pragma unroll
			for (int b = 0; b < 4; ++b)
			{
				const int t = (4 * q + b) % RING;
				r[t] += r[(t + TAP) % RING];
				pack |= ((r[t] >> 1) < T ? 1u : 0u) << (8 * b);
			}
			out[it * RING + q] = pack;
		}
	}
}

// the decisions of a run of ordinal ranges that never goes backwards: the state of the chunk the last range ended in is kept, the next range starts from it
struct KeepGen
{
	const char* tool; uint32_t T; Jump step; RandState st; int64_t chunk;   // st: the state at ordinal chunk * CHUNK
	PinBuf<uint32_t> hst; DevBuf<uint32_t> dst, keep;
	KeepGen(const char* t, uint32_t seed, double percentage, int64_t first) : tool(t), T(keep_threshold(percentage)), step(jump_pow((uint64_t)CHUNK)), chunk(first / CHUNK)
	{
		st = seed_state(seed);
		if (chunk) st = jump_apply(jump_pow((uint64_t)chunk * (uint64_t)CHUNK), st);
	}
	// keep bytes of the ordinals [k0, k0 + m), m > 0: returns the ordinal of keep.p[0] (a chunk boundary <= k0). The caller has waited for the stream since the last run.
	int64_t run(int64_t k0, int64_t m, hipStream_t s)
	{
		const int64_t c0 = k0 / CHUNK, nc = (k0 + m - 1) / CHUNK - c0 + 1;
		for (; chunk < c0; ++chunk) st = jump_apply(step, st);
		hst.ensure((size_t)(RING * nc));
		grow(dst, (size_t)(RING * nc), "the generator states", tool); grow(keep, (size_t)(nc * (CHUNK / 4)), "the keep bytes", tool);
		for (int64_t i = 0; i < nc; ++i)
		{
			if (i) { st = jump_apply(step, st); ++chunk; }
			for (int j = 0; j < RING; ++j) hst.p[(int64_t)j * nc + i] = st.w[j];
		}
		HIPCHK(hipMemcpyAsync(dst.p, hst.p, (size_t)(RING * nc) * 4, hipMemcpyHostToDevice, s));
		hipLaunchKernelGGL(ds_keep_kernel, dim3((unsigned)((nc + 63) / 64)), dim3(64), 0, s, dst.p, nc, T, keep.p); KCHECK();
		return c0 * CHUNK;
	}
};

enum { C_SE, C_SE_PASS, C_PE_PASS, N_DS_COUNTS };

// entries: [0, H) held, [H, H + n) the tile's records. info = output size | 1 << 31; se[i]: the record is single-end (it decides on its own)
__global__ __launch_bounds__(256) void ds_keys_kernel(const uint8_t* __restrict__ infl, const int64_t* __restrict__ recoff, int64_t n, int64_t H, uint64_t mask,
                                                      uint64_t* __restrict__ key, uint32_t* __restrict__ val, uint64_t* __restrict__ src, uint32_t* __restrict__ info, uint8_t* __restrict__ se)
{
	const int64_t stride = (int64_t)gridDim.x * blockDim.x;
	for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < H + n; e += stride)
	{
		val[e] = (uint32_t)e;
		if (e < H) continue;
		const int64_t i = e - H;
		const RecView r = load_rec(infl, recoff[i]);
		src[e] = (uint64_t)(uintptr_t)(infl + recoff[i]);
		if (r.flag & 0x900) { key[e] = KEY_NONE; info[e] = 0; se[i] = 0; continue; }
		info[e] = out_size(r) | 0x80000000u;
		se[i] = (r.flag & 1) ? 0 : 1;
		key[e] = (r.flag & 1) ? rec_name_hash(r) & mask : KEY_NONE;
	}
}

__global__ __launch_bounds__(256) void ds_decides_kernel(const int64_t* __restrict__ close_of, const uint8_t* __restrict__ se, int64_t n, uint64_t* __restrict__ dec)
{
	const int64_t stride = (int64_t)gridDim.x * blockDim.x;
	for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) dec[i] = se[i] || close_of[i] >= 0 ? 1 : 0;
}

// ord: the tile's exclusive scan of dec; kofs: (ordinal of the tile's first decision) - (ordinal of keep[0]). sz: the bytes a kept deciding record adds to the
// output; nsz (want_names): the bytes of its "SE\tname\n" / "PE\tname\n" line
__global__ __launch_bounds__(256) void ds_sizes_kernel(const int64_t* __restrict__ close_of, const uint8_t* __restrict__ se, const uint64_t* __restrict__ dec, const uint64_t* __restrict__ ord,
                                                       const uint8_t* __restrict__ keep, int64_t kofs, const uint32_t* __restrict__ info, const uint64_t* __restrict__ src, int64_t n, int64_t H,
                                                       uint64_t* __restrict__ sz, uint64_t* __restrict__ nsz, unsigned long long* __restrict__ counts)
{
	const int64_t stride = (int64_t)gridDim.x * blockDim.x;
	for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
	{
		const bool kept = dec[i] && keep[kofs + (int64_t)ord[i]];
		uint64_t v = 0;
		if (se[i]) { atomicAdd(&counts[C_SE], 1ull); if (kept) { atomicAdd(&counts[C_SE_PASS], 1ull); v = info[H + i] & 0x7fffffffu; } }
		else if (kept) { atomicAdd(&counts[C_PE_PASS], 1ull); v = (uint64_t)(info[close_of[i] >> 1] & 0x7fffffffu) + (info[H + i] & 0x7fffffffu); }
		sz[i] = v;
		if (nsz) nsz[i] = kept ? 4ull + (uint64_t)rec_name_len((const uint8_t*)(uintptr_t)src[H + i]) : 0;
	}
}

// off: absolute stream position of what every kept deciding record adds; ws: the stream position of obuf[0]
__global__ __launch_bounds__(256) void ds_gather_kernel(const int64_t* __restrict__ close_of, const uint8_t* __restrict__ se, const uint64_t* __restrict__ sz, const uint64_t* __restrict__ off,
                                                        int64_t n, int64_t H, const uint64_t* __restrict__ src, const uint32_t* __restrict__ info, int64_t ws, Win w)
{
	const int lane = threadIdx.x & 63;
	const int64_t nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
	for (int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; i < n; i += nw)
	{
		if (!sz[i]) continue;
		int64_t pos = (int64_t)off[i] - ws;
		if (pos >= w.hi || pos + (int64_t)sz[i] <= w.lo) continue;
		if (!se[i])
		{
			const uint32_t oe = (uint32_t)(close_of[i] >> 1);
			write_record((const uint8_t*)(uintptr_t)src[oe], w, pos, lane);
			pos += info[oe] & 0x7fffffffu;
		}
		write_record((const uint8_t*)(uintptr_t)src[H + i], w, pos, lane);
	}
}

__global__ __launch_bounds__(256) void ds_names_kernel(const uint8_t* __restrict__ se, const uint64_t* __restrict__ nsz, const uint64_t* __restrict__ noff, int64_t n, int64_t H,
                                                       const uint64_t* __restrict__ src, uint8_t* __restrict__ out)
{
	const int64_t stride = (int64_t)gridDim.x * blockDim.x;
	for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
	{
		if (!nsz[i]) continue;
		const uint8_t* s = (const uint8_t*)(uintptr_t)src[H + i];
		uint8_t* d = out + noff[i];
		const uint64_t ln = nsz[i] - 4;
		d[0] = se[i] ? 'S' : 'P'; d[1] = 'E'; d[2] = '\t';
		for (uint64_t k = 0; k < ln; ++k) d[3 + k] = s[36 + k];
		d[3 + ln] = '\n';
	}
}

bool percentage_ok(double p) { return p > 0 && p < 100; }
} // namespace

namespace lib {
// keep_stream.h: the generator for ngsqc_fqedit (FastqDownsample)
struct KeepStream { KeepGen gen; KeepStream(const char* t, uint32_t seed, double p) : gen(t, seed, p, 0) {} };
KeepStream* keep_stream_open(const char* tool, uint32_t seed, double percentage)
{
	if (!percentage_ok(percentage)) { char b[64]; snprintf(b, sizeof(b), "%g", percentage); throw ArgError(std::string("Invalid percentage ") + b + "!"); }
	return new KeepStream(tool, seed, percentage);
}
const uint8_t* keep_stream_run(KeepStream* k, int64_t k0, int64_t m, hipStream_t s) { const int64_t base = k->gen.run(k0, m, s); return (const uint8_t*)k->gen.keep.p + (k0 - base); }
void keep_stream_close(KeepStream* k) { delete k; }

void downsample(ngsqc_handle* h, const ngsqc_downsample_params* dp, const char* out_path, ngsqc_downsample_counts* cnt, char** kept_names)
{
	if (kept_names) *kept_names = nullptr;
	if (!dp || !out_path || !cnt) throw ArgError("null argument");
	const bool names = dp->want_names != 0;
	if (names && !kept_names) throw ArgError("null argument");
	if (!percentage_ok(dp->percentage)) { char b[64]; snprintf(b, sizeof(b), "%g", dp->percentage); throw ArgError(std::string("Invalid percentage ") + b + "!"); }
	const char* T = "BamDownsample";
	require_whole_file(h, T);
	const uint64_t mask = name_hash_mask(h->sw.name_hash_bits);
	const bool timing = h->sw.timing;
	hipStream_t s = h->stream;
	const int64_t W = write_window_bytes(h->sw.write_window_pieces);
	BgzfStream out(T, W, -1);
	NameJoin j(T, s);
	KeepGen gen(T, dp->seed, dp->percentage, 0);
	DevBuf<uint64_t> dec, ord, sz, off, nsz, noff; DevBuf<uint8_t> se, nbuf;
	DevBuf<unsigned long long> counts; counts.alloc(N_DS_COUNTS); HIPCHK(hipMemsetAsync(counts.p, 0, N_DS_COUNTS * sizeof(unsigned long long), s));
	std::string name_lines;
	int64_t K = 0;   // decisions of the tiles so far: the stream ordinal of the tile's first decision
	double ms_join = 0, ms_keep = 0, t_w = wall_ms();
	open_bam(out, out_path, h, s);
	EagerRecoff eager(h);
	stream_tiles(h, [&](const TileCtx& c) {
		const double t0 = wall_ms();
		const int64_t n = c.n_rec, H = j.H, N = H + n;
		const int64_t* rec = n ? ensure_recoff(h) : nullptr;
		j.begin_tile(n, s);
		const char* w = "the decisions";
		grow(dec, (size_t)n + 1, w, T); grow(ord, (size_t)n + 1, w, T); grow(sz, (size_t)n + 1, w, T); grow(off, (size_t)n + 1, w, T); grow(se, (size_t)n + 1, w, T);
		if (names) { grow(nsz, (size_t)n + 1, w, T); grow(noff, (size_t)n + 1, w, T); }
		if (N == 0) return true;
		hipLaunchKernelGGL(ds_keys_kernel, dim3(grid_for(N)), dim3(256), 0, s, c.infl, rec, n, H, mask, j.key.p, j.val.p, j.src.p, j.info.p, se.p); KCHECK();
		j.sort_resolve(n, s);
		uint64_t ntot[2] = {0, 0};
		if (n)
		{
			// the stream ordinals of the tile's deciding records, and their decisions
			uint64_t m2[2] = {0, 0};
			hipLaunchKernelGGL(ds_decides_kernel, dim3(grid_for(n)), dim3(256), 0, s, j.close_of.p, se.p, n, dec.p); KCHECK();
			scan_u64(j.tmp, dec.p, ord.p, 0, (size_t)n, s);
			HIPCHK(hipMemcpyAsync(&m2[0], ord.p + n - 1, 8, hipMemcpyDeviceToHost, s)); HIPCHK(hipMemcpyAsync(&m2[1], dec.p + n - 1, 8, hipMemcpyDeviceToHost, s));
			HIPCHK(hipStreamSynchronize(s));
			const int64_t m = (int64_t)(m2[0] + m2[1]);
			const double tk = wall_ms();
			const int64_t base = m ? gen.run(K, m, s) : K;
			ms_keep += wall_ms() - tk;
			hipLaunchKernelGGL(ds_sizes_kernel, dim3(grid_for(n)), dim3(256), 0, s, j.close_of.p, se.p, dec.p, ord.p, (const uint8_t*)gen.keep.p, K - base, j.info.p, j.src.p, n, H,
			                   sz.p, names ? nsz.p : nullptr, counts.p); KCHECK();
			K += m;
			// the output of the tile's kept records, behind the carried partial piece
			out.place(j.tmp, sz.p, off.p, n, s);
			if (names)
			{
				scan_u64(j.tmp, nsz.p, noff.p, 0, (size_t)n, s);
				HIPCHK(hipMemcpyAsync(&ntot[0], noff.p + n - 1, 8, hipMemcpyDeviceToHost, s)); HIPCHK(hipMemcpyAsync(&ntot[1], nsz.p + n - 1, 8, hipMemcpyDeviceToHost, s));
			}
		}
		j.keep_open(n, s);   // (waits for the stream: the placed end and ntot are on the host)
		const size_t nb = (size_t)(ntot[0] + ntot[1]), nl0 = name_lines.size();
		if (nb)
		{
			grow(nbuf, nb, "the kept names", T);
			hipLaunchKernelGGL(ds_names_kernel, dim3(grid_for(n)), dim3(256), 0, s, se.p, nsz.p, noff.p, n, H, j.src.p, nbuf.p); KCHECK();
			name_lines.resize(nl0 + nb);
			HIPCHK(hipMemcpyAsync(&name_lines[nl0], nbuf.p, nb, hipMemcpyDeviceToHost, s));
		}
		// the tile's records in windows of the stream
		const double dz0 = out.ms_deflate + out.ms_copy;
		out.emit(out.placed_end(n), s, h->device, [&](const Win& win, int64_t ws) {
			if (n) { hipLaunchKernelGGL(ds_gather_kernel, dim3(grid_for(n, 4)), dim3(256), 0, s, j.close_of.p, se.p, sz.p, off.p, n, H, j.src.p, j.info.p, ws, win); KCHECK(); }
		});
		HIPCHK(hipStreamSynchronize(s));   // (the old pool and the tile's bytes are no longer read)
		j.end_tile();
		ms_join += wall_ms() - t0 - (out.ms_deflate + out.ms_copy - dz0);
		return true;
	});
	unsigned long long jc[4] = {0, 0, 0, 0}, dc[N_DS_COUNTS] = {0, 0, 0};
	j.read_counts(jc, s);
	HIPCHK(hipMemcpyAsync(dc, counts.p, sizeof(dc), hipMemcpyDeviceToHost, s)); HIPCHK(hipStreamSynchronize(s));
	out.close(s, h->device, out_path);
	cnt->se = (int64_t)dc[C_SE]; cnt->se_written = (int64_t)dc[C_SE_PASS]; cnt->pe = (int64_t)(jc[0] + jc[1]); cnt->pe_written = (int64_t)dc[C_PE_PASS]; cnt->pe_unmatched = j.H;
	if (names)
	{
		char* p = (char*)malloc(name_lines.size() + 1);
		if (!p) throw std::runtime_error("out of host memory for the kept names");
		memcpy(p, name_lines.data(), name_lines.size()); p[name_lines.size()] = 0;
		*kept_names = p;
	}
	if (timing)
		fprintf(stderr, "[ngsqc] downsample: %.1f ms in all: join and gather %.1f ms (of which generator states and keep kernel launch %.1f ms, %lld decisions), deflate %.1f ms, "
		                "copy to pinned memory %.1f ms, file writes %.1f ms (host thread), %lld open names at the end, windows of %lld bytes\n",
		        wall_ms() - t_w, ms_join, ms_keep, (long long)K, out.ms_deflate, out.ms_copy, out.sink.write_ms, (long long)j.H, (long long)W);
}
} // namespace lib
} // namespace ngsqc

int ngsqc_downsample(ngsqc_handle* h, const ngsqc_downsample_params* p, const char* out_bam_path, ngsqc_downsample_counts* c, char** kept_names)
{
	return guarded(h, [&] { ngsqc::lib::downsample(h, p, out_bam_path, c, kept_names); });
}

int ngsqc_downsample_keep(uint32_t seed, double percentage, int64_t first, int64_t n, int device, uint8_t* out)
{
	if (!percentage_ok(percentage) || first < 0 || n < 0 || first > INT64_MAX - n || (n && !out) || device < 0 || device >= 64) return NGSQC_E_ARG;
	if (n == 0) return NGSQC_OK;
	try
	{
		HIPCHK(hipSetDevice(device));
		// one stream per device for the process, as in ngsqc_bgzf_compress
		static std::mutex mu; static hipStream_t streams[64] = {nullptr};
		std::lock_guard<std::mutex> g(mu);
		if (!streams[device]) HIPCHK(hipStreamCreateWithFlags(&streams[device], hipStreamNonBlocking));
		hipStream_t s = streams[device];
		constexpr int64_t WIN_CHUNKS = 4096;   // chunks per launch: the device memory stays bounded whatever n is
		KeepGen gen("ngsqc_downsample_keep", seed, percentage, first);
		for (int64_t o = 0; o < n; )
		{
			const int64_t k0 = first + o, k = std::min(n - o, (k0 / CHUNK + WIN_CHUNKS) * CHUNK - k0);   // (up to a chunk boundary)
			const int64_t base = gen.run(k0, k, s);
			HIPCHK(hipMemcpyAsync(out + o, (const uint8_t*)gen.keep.p + (k0 - base), (size_t)k, hipMemcpyDeviceToHost, s));
			HIPCHK(hipStreamSynchronize(s));
			o += k;
		}
		return NGSQC_OK;
	}
	catch (std::exception& e) { fprintf(stderr, "ngsqc_downsample_keep: %s\n", e.what()); return NGSQC_E_DEVICE; }
}
