// FASTQ text in device memory -> the raw-read statistics of ReadQC (src/ReadQC/main.cpp:57-96: FastqFileStream::readEntry + StatisticsReads::update(const
// FastqEntry&)), in the accumulators of reads.hip (ReadsAcc, the [RQ_CYC][7] cycle table) so that everything downstream of ngsqc_read_stats is unchanged.
//   line index  fq_count_kernel: '\n' per FQ_BLOCK bytes (a 16-byte load per lane, a 16-bit match mask, popcount, wave sum) -> scan of the block counts
//               (launch_scan_counts) -> fq_lines_kernel: the start offset of every line. The four lines of entry r are lines 4r .. 4r + 3: the phase comes from
//               the newline count alone (a quality line may begin with '@' or '+').
//   entries     fq_entry_kernel: ONE WAVE PER ENTRY, lanes striding over the cycles as reads_kernel does; validation (fastq_visit.h) leaves the first failing
//               (entry, kind) in one word by atomicMin.
// The accumulator (ngsqc_fastq) takes the text in pieces cut anywhere, keeps the incomplete tail as a carry in front of the next piece, and copies through two
// pinned slots: the kernels of a piece run while the caller inflates the next one (a piece is finished when the next feed, or the result, asks for it). Where
// the text ends, the lines of an entry on the host and the reference's messages are fastq_text.h's, shared with the accumulators of fastq_feed.h.
#include "handle.h"
#include "fastq_visit.h"
#include <map>

namespace ngsqc {
namespace {
__device__ __forceinline__ uint32_t fq_wave_sum(uint32_t x)
{
	#pragma unroll
	for (int o = 32; o > 0; o >>= 1) x += (uint32_t)__shfl_xor((int)x, o);
	return x;
}
// the newline mask of the lane's 16 bytes (text is padded to a multiple of FQ_BLOCK: the load is inside the buffer, bytes at or behind n are masked off)
__device__ __forceinline__ uint32_t fq_lane_mask(const uint8_t* __restrict__ text, uint64_t n, uint64_t pos)
{
	const uint4 w = *(const uint4*)(text + pos);
	return fq_mask_in_range(fq_newline_mask16(w.x, w.y, w.z, w.w), pos, n);
}
enum { FM_ERR, FM_MAX, FM_HEADERS, FM_LONG, FM_TOTAL };        // d_misc
enum { FR_LINES, FR_ENTRIES, FR_CARRY, FR_TOTAL };             // d_res
} // namespace

__global__ __launch_bounds__(256) void fq_count_kernel(const uint8_t* __restrict__ text, uint64_t n, uint32_t* __restrict__ cnt)
{
	__shared__ uint32_t s_w[4];
	const uint64_t pos = (uint64_t)blockIdx.x * FQ_BLOCK + threadIdx.x * 16u;
	const uint32_t c = fq_wave_sum((uint32_t)__popc(fq_lane_mask(text, n, pos)));
	if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = c;
	__syncthreads();
	if (threadIdx.x == 0) cnt[blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

// lines[0] = 0; the k-th '\n' of the text (k from 0) at offset p gives lines[k + 1] = p + 1. base: exclusive scan of the block counts.
__global__ __launch_bounds__(256) void fq_lines_kernel(const uint8_t* __restrict__ text, uint64_t n, const int64_t* __restrict__ base, uint32_t* __restrict__ lines)
{
	__shared__ uint32_t s_w[4];
	const uint64_t pos = (uint64_t)blockIdx.x * FQ_BLOCK + threadIdx.x * 16u;
	uint32_t m = fq_lane_mask(text, n, pos);
	const uint32_t c = (uint32_t)__popc(m);
	uint32_t incl = c;
	#pragma unroll
	for (int o = 1; o < 64; o <<= 1) { const uint32_t t = (uint32_t)__shfl_up((int)incl, o); if ((int)(threadIdx.x & 63) >= o) incl += t; }
	if ((threadIdx.x & 63) == 63) s_w[threadIdx.x >> 6] = incl;
	__syncthreads();
	uint64_t rank = (uint64_t)base[blockIdx.x] + incl - c;
	for (uint32_t w = 0; w < (threadIdx.x >> 6); ++w) rank += s_w[w];
	while (m) { const uint32_t k = (uint32_t)__builtin_ctz(m); m &= m - 1; lines[rank + 1] = (uint32_t)(pos + k + 1); ++rank; }
	if (blockIdx.x == 0 && threadIdx.x == 0) lines[0] = 0;
}

// what the host needs of a piece: its lines, its entries and where the carry starts (the first byte of line 4 * entries; behind the last piece: nothing is left)
__global__ void fq_result_kernel(const int64_t* __restrict__ total, const uint32_t* __restrict__ lines, uint64_t n, int last, unsigned long long* __restrict__ res)
{
	const uint64_t L = (uint64_t)*total, E = last ? (L + 3) / 4 : L / 4;
	res[FR_LINES] = L; res[FR_ENTRIES] = E; res[FR_CARRY] = 4 * E <= L ? lines[4 * E] : n;
}

// The line index of n bytes of text (d_text padded to a multiple of FQ_BLOCK): d_lines[0 .. L] and the line count L in d_base[blocks], blocks = ceil(n / FQ_BLOCK).
// d_cnt: blocks + 1, d_base: blocks + 2, d_tmp: scan_tmp_bytes(blocks) + 64, d_lines: n + 2. Shared with purge.hip.
void launch_fastq_line_index(const uint8_t* d_text, size_t n, uint32_t* d_cnt, int64_t* d_base, void* d_tmp, uint32_t* d_lines, hipStream_t stream)
{
	const int64_t blocks = (int64_t)((n + FQ_BLOCK - 1) / FQ_BLOCK);
	if (blocks) { hipLaunchKernelGGL(fq_count_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, d_text, (uint64_t)n, d_cnt); KCHECK(); }
	launch_scan_counts(d_cnt, blocks, d_base, d_tmp, stream);
	if (blocks) { hipLaunchKernelGGL(fq_lines_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, d_text, (uint64_t)n, d_base, d_lines); KCHECK(); }
	else HIPCHK(hipMemsetAsync(d_lines, 0, sizeof(uint32_t), stream));
}

struct FqKernelArgs
{
	const uint8_t* text; const uint32_t* lines; const int64_t* total;
	int last, reverse, long_read; unsigned long long entry_base;
	unsigned long long* acc; unsigned long long* len_hist; unsigned long long* cyc; unsigned long long* misc; unsigned long long* long_list; unsigned long long long_cap;
};

// acc layout (u64): see ReadsAcc in common.h. Statistics of an entry that fails validation are still added (inside every table's bounds): the accumulator is
// void from the first error on.
__global__ __launch_bounds__(256) void fq_entry_kernel(const FqKernelArgs a)
{
	__shared__ uint32_t s_bq[100], s_rq[100], s_qd[120];
	for (int i = threadIdx.x; i < 100; i += 256) { s_bq[i] = 0; s_rq[i] = 0; }
	for (int i = threadIdx.x; i < 120; i += 256) s_qd[i] = 0;
	__syncthreads();
	const uint32_t lane = threadIdx.x & 63;
	const unsigned long long wave = ((unsigned long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((unsigned long long)gridDim.x * blockDim.x) >> 6;
	const uint64_t L = (uint64_t)*a.total, E = a.last ? (L + 3) / 4 : L / 4;
	const uint8_t* __restrict__ text = a.text;
	uint32_t cB[RQ_PASSES][5], qs[RQ_PASSES];
	#pragma unroll
	for (int k = 0; k < RQ_PASSES; ++k) { qs[k] = 0; for (int c = 0; c < 5; ++c) cB[k][c] = 0; }
	unsigned long long tB[5] = {0, 0, 0, 0, 0};                                        // bases behind the per-cycle window (per lane)
	unsigned long long n_reads = 0, n_bases = 0, n_headers = 0, max_len = 0;           // wave-uniform
	long long run_len = -1; unsigned long long run_cnt = 0;
	for (unsigned long long r = wave; r < E; r += n_waves)
	{
		const FqEntry e = fq_entry(text, a.lines, L, r);
		const uint32_t kind = fq_entry_kind(text, e);
		if (kind) { if (lane == 0) atomicMin(&a.misc[FM_ERR], fq_error_word(a.entry_base + r, kind)); continue; }
		const bool header_empty = e.header.len == 0;
		if (!header_empty) ++n_headers;
		const uint32_t cycles = e.bases.len;
		++n_reads; n_bases += cycles; max_len = cycles > max_len ? cycles : max_len;
		if (cycles >= FQ_LEN_DENSE)
		{
			if (lane == 0) { const unsigned long long at = atomicAdd(&a.misc[FM_LONG], 1ull); if (at < a.long_cap) a.long_list[at] = cycles; }
		}
		else if ((long long)cycles == run_len) ++run_cnt;
		else
		{
			if (run_cnt && lane == 0) atomicAdd(&a.len_hist[run_len], run_cnt);
			run_len = cycles; run_cnt = 1;
		}
		const uint8_t* __restrict__ b = text + e.bases.start; const uint8_t* __restrict__ q = text + e.quals.start;
		uint32_t qsum = 0; bool bb = false, bq = false;
		#pragma unroll
		for (int k = 0; k < RQ_PASSES; ++k)
		{
			const uint32_t i = k * 64 + lane;
			if (i < cycles)
			{
				const FqChar c = fq_char(b[i], q[i], a.long_read);
				cB[k][0] += c.cls == 0; cB[k][1] += c.cls == 1; cB[k][2] += c.cls == 2; cB[k][3] += c.cls == 3; cB[k][4] += c.cls == 4;
				bb |= c.cls == 5; bq |= !c.ok;
				qsum += c.q; qs[k] += c.q;
				atomicAdd(&s_bq[c.q], 1u);
			}
		}
		for (uint32_t i = RQ_CYC + lane; i < cycles; i += 64)
		{
			const FqChar c = fq_char(b[i], q[i], a.long_read);
			tB[0] += c.cls == 0; tB[1] += c.cls == 1; tB[2] += c.cls == 2; tB[3] += c.cls == 3; tB[4] += c.cls == 4;
			bb |= c.cls == 5; bq |= !c.ok;
			qsum += c.q;
			atomicAdd(&s_bq[c.q], 1u);
		}
		// a lane adds at most 2^25 qualities below 94 (a piece holds fewer than 2^31 bytes): 32 bits hold its sum, the wave's needs 64
		unsigned long long wsum = qsum;
		#pragma unroll
		for (int o = 32; o > 0; o >>= 1) wsum += __shfl_xor(wsum, o);
		const uint32_t ckind = fq_char_kind(header_empty, __builtin_amdgcn_ballot_w64(bb) != 0, __builtin_amdgcn_ballot_w64(bq) != 0);
		if (lane == 0)
		{
			if (ckind) atomicMin(&a.misc[FM_ERR], fq_error_word(a.entry_base + r, ckind));
			if (cycles > 0)
			{
				int rq, qd; fq_mean_bins(wsum, cycles, rq, qd);
				if (rq >= 0) atomicAdd(&s_rq[rq], 1u);
				atomicAdd(&s_qd[(a.reverse ? 60 : 0) + qd], 1u);
			}
		}
	}
	if (run_cnt && lane == 0) atomicAdd(&a.len_hist[run_len], run_cnt);
	// ---- flush ----
	#pragma unroll
	for (int k = 0; k < RQ_PASSES; ++k)
	{
		unsigned long long* c = a.cyc + 7ull * (k * 64 + lane);
		#pragma unroll
		for (int j = 0; j < 5; ++j) { if (cB[k][j]) atomicAdd(c + j, (unsigned long long)cB[k][j]); tB[j] += cB[k][j]; }
		if (qs[k]) atomicAdd(c + (a.reverse ? 6 : 5), (unsigned long long)qs[k]);
	}
	#pragma unroll
	for (int o = 32; o > 0; o >>= 1) { for (int j = 0; j < 5; ++j) tB[j] += __shfl_xor(tB[j], o); }
	if (lane == 0)
	{
		if (n_reads) atomicAdd(&a.acc[a.reverse ? RA_REV : RA_FWD], n_reads);
		if (n_bases) atomicAdd(&a.acc[RA_BASES], n_bases);
		for (int j = 0; j < 5; ++j) if (tB[j]) atomicAdd(&a.acc[RA_A + j], tB[j]);
		if (n_headers) atomicAdd(&a.misc[FM_HEADERS], n_headers);
		if (max_len) atomicMax(&a.misc[FM_MAX], max_len);
	}
	__syncthreads();
	for (int i = threadIdx.x; i < 100; i += 256) { if (s_bq[i]) atomicAdd(&a.acc[RA_BQ0 + i], (unsigned long long)s_bq[i]); if (s_rq[i]) atomicAdd(&a.acc[RA_RQ0 + i], (unsigned long long)s_rq[i]); }
	for (int i = threadIdx.x; i < 120; i += 256) if (s_qd[i]) atomicAdd(&a.acc[RA_QD0 + i], (unsigned long long)s_qd[i]);
}

} // namespace ngsqc

// ---------------------------------------------------------------- the accumulator behind the C ABI
#include "fastq_feed.h"
using namespace ngsqc::lib;

struct ngsqc_fastq
{
	int device = 0, long_read = 0; hipStream_t stream = nullptr; std::string err; bool failed = false;
	// text: slot[cur][cstart, len) is the carry; while a piece is pending its kernels read d_text and cstart is not known yet
	PinBuf<uint8_t> slot[2]; size_t len = 0, cstart = 0; int cur = 0;
	DevBuf<uint8_t> d_text, d_tmp; DevBuf<uint32_t> d_cnt, d_lines; DevBuf<int64_t> d_base;
	DevBuf<unsigned long long> d_acc, d_len, d_cyc, d_misc, d_long, d_res; PinBuf<unsigned long long> p_res;
	bool pending = false, pend_last = false;
	hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
	// the current file
	bool file_open = false; int64_t file_ordinal = -1; unsigned long long entry_base = 0, headers_base = 0, headers_total = 0;
	std::map<int64_t, int64_t> long_lengths; int64_t max_cycles = 0;
	ngsqc_fastq_report rep{};
	std::vector<int64_t> res_len, res_cyc;

	~ngsqc_fastq()
	{
		(void)hipSetDevice(device);
		if (stream) { (void)hipStreamSynchronize(stream); (void)hipStreamDestroy(stream); }
		for (auto& e : ev) if (e) (void)hipEventDestroy(e);
	}
	void init(int dev, int lr)
	{
		int n_dev = 0;
		if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) throw std::runtime_error("no HIP device available (libngsqc_hip has no CPU fallback)");
		if (dev < 0 || dev >= n_dev) throw ArgError("no such device");
		device = dev; long_read = lr ? 1 : 0; rep.err_file = rep.err_entry = -1;
		HIPCHK(hipSetDevice(device));
		HIPCHK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
		for (auto& e : ev) HIPCHK(hipEventCreate(&e));
		d_acc.alloc(RA_TOTAL); d_len.alloc(FQ_LEN_DENSE); d_cyc.alloc((size_t)RQ_CYC * 7); d_misc.alloc(FM_TOTAL); d_res.alloc(FR_TOTAL); p_res.ensure(FR_TOTAL + FM_TOTAL);
		HIPCHK(hipMemsetAsync(d_acc.p, 0, RA_TOTAL * 8, stream)); HIPCHK(hipMemsetAsync(d_len.p, 0, (size_t)FQ_LEN_DENSE * 8, stream));
		HIPCHK(hipMemsetAsync(d_cyc.p, 0, (size_t)RQ_CYC * 7 * 8, stream)); HIPCHK(hipMemsetAsync(d_misc.p, 0, FM_TOTAL * 8, stream));
		HIPCHK(hipMemsetAsync(d_misc.p + FM_ERR, 0xff, 8, stream));
		HIPCHK(hipStreamSynchronize(stream));
	}
	void grow_slot(int s, size_t need, size_t keep_from, size_t keep_to)   // slot s holds at least need bytes; its bytes [keep_from, keep_to) survive
	{
		if (slot[s].n >= need) return;
		PinBuf<uint8_t> nw; nw.ensure(need + need / 2 + 4096);
		if (keep_to > keep_from) memcpy(nw.p + keep_from, slot[s].p + keep_from, keep_to - keep_from);
		std::swap(nw.p, slot[s].p); std::swap(nw.n, slot[s].n);
	}
	// the reference's message for the entry the device named (FastqFileStream.cpp:3-44; kind 6 is ours); the text of the piece is still in its slot
	void build_error(unsigned long long word, uint64_t n_lines)
	{
		const uint64_t entry = word >> 8, r = entry - entry_base; const int kind = (int)(word & 255);
		std::string ln[4]; fq_fetch_entry(slot[cur].p, d_lines.p, n_lines, r, stream, ln);
		if (kind != FQ_ERR_EMPTY_HEADER) err = fq_validate_message(kind, ln, long_read);
		else err = "Invalid Fastq file entry: Entry " + std::to_string(entry) + " has an empty header line and bases or qualities that cannot be counted (" + std::to_string(ln[1].size()) + " bases, " + std::to_string(ln[3].size()) + " qualities).";
		failed = true;
		rep.err_file = file_ordinal; rep.err_entry = (int64_t)entry; rep.err_kind = kind;
	}
	// waits for the piece in flight and takes its results
	void finish()
	{
		if (!pending) return;
		const double t0 = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
		HIPCHK(hipStreamSynchronize(stream));
		rep.wait_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count() - t0;
		float ms = 0; HIPCHK(hipEventElapsedTime(&ms, ev[0], ev[1])); rep.h2d_ms += ms; HIPCHK(hipEventElapsedTime(&ms, ev[1], ev[2])); rep.kernels_ms += ms;
		pending = false;
		const unsigned long long* r = p_res.p; const unsigned long long* m = p_res.p + FR_TOTAL;
		const unsigned long long n_long = std::min<unsigned long long>(m[FM_LONG], d_long.n);
		if (n_long)
		{
			std::vector<unsigned long long> ll((size_t)n_long);
			HIPCHK(hipMemcpyAsync(ll.data(), d_long.p, ll.size() * 8, hipMemcpyDeviceToHost, stream)); HIPCHK(hipStreamSynchronize(stream));
			for (auto l : ll) ++long_lengths[(int64_t)l];
		}
		max_cycles = std::max<int64_t>(max_cycles, (int64_t)m[FM_MAX]);
		headers_total = m[FM_HEADERS];
		if (m[FM_ERR] != FQ_NO_ERROR) { build_error(m[FM_ERR], r[FR_LINES]); return; }
		entry_base += r[FR_ENTRIES];
		rep.entries = (int64_t)(headers_total - headers_base);
		cstart = (size_t)r[FR_CARRY]; if (cstart > len) cstart = len;
		if (pend_last) { cstart = len = 0; file_open = false; }
	}
	void launch(size_t n, bool last, int direction)   // slot[cur][0, n) is the text to index
	{
		const int64_t blocks = (int64_t)((n + FQ_BLOCK - 1) / FQ_BLOCK);
		d_text.ensure_slack((size_t)std::max<int64_t>(blocks, 1) * FQ_BLOCK); d_cnt.ensure_slack((size_t)blocks + 1); d_base.ensure_slack((size_t)blocks + 2);
		d_tmp.ensure_slack(scan_tmp_bytes(blocks) + 64); d_lines.ensure_slack(n + 2); d_long.ensure_slack(n / FQ_LEN_DENSE + 1);
		HIPCHK(hipEventRecord(ev[0], stream));
		if (n) HIPCHK(hipMemcpyAsync(d_text.p, slot[cur].p, n, hipMemcpyHostToDevice, stream));
		HIPCHK(hipEventRecord(ev[1], stream));
		HIPCHK(hipMemsetAsync(d_misc.p + FM_LONG, 0, 8, stream));
		launch_fastq_line_index(d_text.p, n, d_cnt.p, d_base.p, d_tmp.p, d_lines.p, stream);
		hipLaunchKernelGGL(fq_result_kernel, dim3(1), dim3(1), 0, stream, d_base.p + blocks, d_lines.p, (uint64_t)n, last ? 1 : 0, d_res.p); KCHECK();
		if (n)
		{
			FqKernelArgs a{d_text.p, d_lines.p, d_base.p + blocks, last ? 1 : 0, direction ? 1 : 0, long_read, entry_base, d_acc.p, d_len.p, d_cyc.p, d_misc.p, d_long.p, (unsigned long long)d_long.n};
			// an entry holds at least four bytes; 2048 workgroups: the 32-bit LDS bins of a workgroup stay far below 2^32 for a piece of less than 2^31 bytes
			const int64_t wgs = std::min<int64_t>((int64_t)(n / 16) + 1, 256 * 8);
			hipLaunchKernelGGL(fq_entry_kernel, dim3((unsigned)wgs), dim3(256), 0, stream, a); KCHECK();
		}
		HIPCHK(hipEventRecord(ev[2], stream));
		HIPCHK(hipMemcpyAsync(p_res.p, d_res.p, FR_TOTAL * 8, hipMemcpyDeviceToHost, stream));
		HIPCHK(hipMemcpyAsync(p_res.p + FR_TOTAL, d_misc.p, FM_TOTAL * 8, hipMemcpyDeviceToHost, stream));
		pending = true; pend_last = last;
	}
	int feed(const uint8_t* text, int64_t n, int direction, int last)
	{
		if (n < 0 || (n && !text)) throw ArgError("ngsqc_fastq_feed: invalid text");
		HIPCHK(hipSetDevice(device));
		finish();
		if (failed) return NGSQC_E_FORMAT;
		if (!file_open) { file_open = true; ++file_ordinal; entry_base = 0; headers_base = headers_total; rep.entries = 0; rep.files = file_ordinal + 1; }
		const size_t carry = len - cstart;
		if (carry + (size_t)n + 1 >= ((size_t)1 << 31)) throw ArgError("ngsqc_fastq_feed: a piece and the carry in front of it must stay below 2 GiB");
		if (!last && (n == 0 || !memchr(text, '\n', (size_t)n)))
		{
			// no line ends in this piece: nothing new can be complete. It joins the carry where that lies (no kernel reads the slot now).
			grow_slot(cur, len + (size_t)n, cstart, len);
			if (n) memcpy(slot[cur].p + len, text, (size_t)n);
			len += (size_t)n;
			return NGSQC_OK;
		}
		const int other = cur ^ 1;
		grow_slot(other, carry + (size_t)n + 1, 0, 0);
		if (carry) memcpy(slot[other].p, slot[cur].p + cstart, carry);
		if (n) memcpy(slot[other].p + carry, text, (size_t)n);
		cur = other; cstart = 0; len = carry + (size_t)n;
		uint8_t* t = slot[cur].p;
		size_t n_idx;
		if (last)
		{
			if (len && t[len - 1] != '\n') t[len++] = '\n';   // a file need not end with a newline
			len = n_idx = fq_strip_empty_lines(t, len);        // lines at the end of a file that are all empty are ignored
		}
		else n_idx = fq_strip_empty_lines(t, len);           // ... and they may still turn out to be that: they wait in the carry
		launch(n_idx, last != 0, direction);
		if (last) { finish(); if (failed) return NGSQC_E_FORMAT; }
		return NGSQC_OK;
	}
	void result(ngsqc_read_stats* st, ngsqc_fastq_report* out)
	{
		HIPCHK(hipSetDevice(device));
		finish();
		std::vector<unsigned long long> acc(RA_TOTAL), cyc((size_t)RQ_CYC * 7);
		const size_t dense = (size_t)std::min<int64_t>(max_cycles + 1, FQ_LEN_DENSE);
		std::vector<unsigned long long> lens(dense);
		HIPCHK(hipMemcpyAsync(acc.data(), d_acc.p, acc.size() * 8, hipMemcpyDeviceToHost, stream));
		HIPCHK(hipMemcpyAsync(cyc.data(), d_cyc.p, cyc.size() * 8, hipMemcpyDeviceToHost, stream));
		HIPCHK(hipMemcpyAsync(lens.data(), d_len.p, lens.size() * 8, hipMemcpyDeviceToHost, stream));
		HIPCHK(hipStreamSynchronize(stream));
		if (st)
		{
			memset(st, 0, sizeof(*st));
			st->c_forward = (int64_t)acc[RA_FWD]; st->c_reverse = (int64_t)acc[RA_REV]; st->bases_sequenced = (int64_t)acc[RA_BASES];
			for (int i = 0; i < 5; ++i) st->bases[i] = (int64_t)acc[RA_A + i];
			for (int i = 0; i < 100; ++i) { st->base_qualities[i] = (int64_t)acc[RA_BQ0 + i]; st->read_qualities[i] = (int64_t)acc[RA_RQ0 + i]; }
			for (int i = 0; i < 60; ++i) { st->qscore_dist_r1[i] = (int64_t)acc[RA_QD0 + i]; st->qscore_dist_r2[i] = (int64_t)acc[RA_QD0 + 60 + i]; }
			st->max_cycles = max_cycles;
		}
		res_len.assign((size_t)max_cycles + 1, 0);
		for (size_t i = 0; i < dense; ++i) res_len[i] = (int64_t)lens[i];
		for (auto& kv : long_lengths) res_len[(size_t)kv.first] += kv.second;
		res_cyc.assign(cyc.begin(), cyc.end());
		if (out) *out = rep;
	}
};

namespace { thread_local std::string g_fastq_error; }

extern "C" {
int ngsqc_fastq_create(int32_t device, int32_t long_read, ngsqc_fastq** out)
{
	if (!out) return NGSQC_E_ARG;
	*out = nullptr;
	return fastq_guard((ngsqc_fastq*)nullptr, g_fastq_error, [&] { std::unique_ptr<ngsqc_fastq> f(new ngsqc_fastq); f->init(device, long_read); *out = f.release(); return NGSQC_OK; });
}
void ngsqc_fastq_destroy(ngsqc_fastq* f) { delete f; }
const char* ngsqc_fastq_last_error(const ngsqc_fastq* f) { return f ? f->err.c_str() : g_fastq_error.c_str(); }
int ngsqc_fastq_feed(ngsqc_fastq* f, const uint8_t* text, int64_t n, int32_t direction, int32_t last)
{
	if (!f) return NGSQC_E_ARG;
	return fastq_guard(f, g_fastq_error, [&] { return f->feed(text, n, direction, last); });
}
int ngsqc_fastq_result(ngsqc_fastq* f, ngsqc_read_stats* st, ngsqc_fastq_report* rep)
{
	if (!f) return NGSQC_E_ARG;
	return fastq_guard(f, g_fastq_error, [&] { f->result(st, rep); return f->failed ? NGSQC_E_FORMAT : NGSQC_OK; });
}
int ngsqc_fastq_length_hist(ngsqc_fastq* f, int64_t* out, int64_t cap)
{
	if (!f) return NGSQC_E_ARG;
	return fastq_guard(f, g_fastq_error, [&] {
		if (f->res_len.empty()) throw ArgError("no read statistics: call ngsqc_fastq_result first");
		if (!out || cap < (int64_t)f->res_len.size()) throw ArgError("read-length buffer too small");
		std::copy(f->res_len.begin(), f->res_len.end(), out);
		return NGSQC_OK; });
}
int ngsqc_fastq_cycle_stats(ngsqc_fastq* f, int64_t* out, int64_t n_cycles)
{
	if (!f) return NGSQC_E_ARG;
	return fastq_guard(f, g_fastq_error, [&] {
		if (f->res_cyc.empty()) throw ArgError("no read statistics: call ngsqc_fastq_result first");
		if (!out || n_cycles < 0) throw ArgError("invalid cycle buffer");
		const int64_t n = std::min<int64_t>(n_cycles, RQ_CYC);
		std::copy(f->res_cyc.begin(), f->res_cyc.begin() + 7 * n, out);
		return NGSQC_OK; });
}
}
