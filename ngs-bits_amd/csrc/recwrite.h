// The BAM-output path of the tools that stream a BAM and write one (BamFilter: pairs.hip, BamDownsample: downsample.hip, BamExtract: extract.hip,
// BamRemoveVariants: rmvar.hip, BamClipOverlap: clip.hip, BamCleanHaloplex: haloplex.hip), on top of join.h's BgzfStream:
//   - the bytes BamWriter::writeAlignment writes for a record (src/cppNGS/BamWriter.cpp over htslib's bam_write1): the size a record takes in the output
//     (out_size) and the wave-wide copy into a window (write_record), with bits OR-ed into the copy's flag word where a tool asks for it;
//   - bam_header_bytes / open_bam: the output's sink and the input's header in front of it (all six);
//   - gather_kernel: the records that leave as they came, a wave each. Its source is FromTile (BamExtract, BamCleanHaloplex) or FromPtrs (BamClipOverlap's open
//     names), its flag mask NoMask or the tool's own (BamCleanHaloplex). The gathers of pairs carry tool logic and stay with their tools;
//   - for_each_tile_bytes: the entry points that hand out one byte per record and write nothing (ngsqc_match_names, _variant_verdicts, _haloplex_verdicts);
//   - fetch_rec_head: the start of a failing record for the reference's error message (BamRemoveVariants, BamClipOverlap).
// Compiled for gfx950 (-Rpass-analysis=kernel-resource-usage), no scratch and no LDS: gather_kernel<true, FromTile, NoMask> 42 VGPRs, 97 SGPRs, 8 waves per
// SIMD; <false, FromTile, HxMask> (haloplex.hip) 44 VGPRs, 102 SGPRs, 7 waves per SIMD; <false, FromPtrs, NoMask> 40 VGPRs, 92 SGPRs, 8 waves per SIMD. The mask
// is a type, not an argument that is usually 0: the two branches of write_record's copy loop in one kernel cost the maskless gather a wave of occupancy.
#pragma once
#include "join.h"

namespace ngsqc {
namespace {
// bin of htslib's hts_reg2bin(beg, end, 14, 5)
__device__ __forceinline__ uint32_t reg2bin(int64_t beg, int64_t end)
{
	--end;
	if (beg >> 14 == end >> 14) return (uint32_t)(((1 << 15) - 1) / 7 + (beg >> 14));
	if (beg >> 17 == end >> 17) return (uint32_t)(((1 << 12) - 1) / 7 + (beg >> 17));
	if (beg >> 20 == end >> 20) return (uint32_t)(((1 << 9) - 1) / 7 + (beg >> 20));
	if (beg >> 23 == end >> 23) return (uint32_t)(((1 << 6) - 1) / 7 + (beg >> 23));
	if (beg >> 26 == end >> 26) return (uint32_t)(((1 << 3) - 1) / 7 + (beg >> 26));
	return 0;
}

// A record whose CIGAR comes from its CG tag (rec_apply_cg) is written as htslib's bam_write1 writes what bam_read1 made of it: up to 65535 operations inline and
// without the tag, more as the placeholder "l_seq S, ref_len N" with CG:B,I appended behind the other tags; bin from the real span in both cases.
struct CgInfo { const uint8_t* ops; uint32_t n; const uint8_t* tag; };   // ops: the tag's array; tag: the tag's first byte (its length is 8 + 4 n)
__device__ __forceinline__ bool cg_of(const RecView& r, CgInfo& g)
{
	RecView e = r; rec_apply_cg(e);
	if (e.cigar == r.cigar) return false;
	g.ops = e.cigar; g.n = e.n_cigar; g.tag = e.cigar - 8;
	return true;
}
// e: r behind rec_apply_cg (a caller that needs the effective CIGAR anyway scans the tags once)
__device__ __forceinline__ uint32_t out_size(const RecView& r, const RecView& e)
{
	if (e.cigar == r.cigar) return r.bs + 4;
	return e.n_cigar <= 65535 ? r.bs + 4 - 4 * r.n_cigar_raw - 8 : r.bs + 4 - 4 * r.n_cigar_raw + 8;
}
__device__ __forceinline__ uint32_t out_size(const RecView& r)
{
	RecView e = r; rec_apply_cg(e);
	return out_size(r, e);
}

// one record into the output window at pos (wave-wide). flag_or: bits OR-ed into the flag word of the copy (bytes 18-19 of the record, block_size included); each
// of the two bytes is stored by whoever stores that byte of the copy, and only where it lies inside the window: a record that straddles two windows gets its
// low flag byte in one launch and its high one in the other. 0 (the default): the copy is the source's bytes
__device__ void write_record(const uint8_t* __restrict__ s, const Win& w, int64_t pos, int lane, uint32_t flag_or = 0)
{
	const RecView r = load_rec(s, 0);
	CgInfo g;
	if (!cg_of(r, g))
	{
		const int64_t n = (int64_t)r.bs + 4, a = max<int64_t>(0, w.lo - pos), b = min<int64_t>(n, w.hi - pos);
		if (!flag_or) { for (int64_t i = a + lane; i < b; i += 64) w.base[pos + i] = s[i]; return; }
		for (int64_t i = a + lane; i < b; i += 64) w.base[pos + i] = (uint8_t)(s[i] | (i == 18 ? flag_or : i == 19 ? flag_or >> 8 : 0u));
		return;
	}
	if (lane) return;   // (rare: long reads only)
	const uint32_t osz = out_size(r);
	uint32_t rlen = 0;
	for (uint32_t i = 0; i < g.n; ++i) { const uint32_t c = ld32(g.ops + 4ull * i), op = c & 15u; if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) rlen += c >> 4; }
	const int64_t end = (int64_t)r.pos + ((r.flag & 4) || rlen == 0 ? 1 : rlen);
	const bool inl = g.n <= 65535;
	const uint32_t bs = osz - 4, bin = reg2bin(r.pos, end), nc = inl ? g.n : 2;
	uint8_t fixed[36];
	for (int i = 0; i < 36; ++i) fixed[i] = s[i];
	for (int i = 0; i < 4; ++i) fixed[i] = (uint8_t)(bs >> (8 * i));
	fixed[14] = (uint8_t)bin; fixed[15] = (uint8_t)(bin >> 8); fixed[16] = (uint8_t)nc; fixed[17] = (uint8_t)(nc >> 8);
	fixed[18] |= (uint8_t)flag_or; fixed[19] |= (uint8_t)(flag_or >> 8);   // (put() keeps each byte to the window)
	int64_t o = pos;
	for (int i = 0; i < 36; ++i) put(w, o, fixed[i]);
	for (uint32_t i = 0; i < r.l_name; ++i) put(w, o, s[36 + i]);
	if (inl) for (uint32_t i = 0; i < 4 * g.n; ++i) put(w, o, g.ops[i]);
	else
	{
		const uint32_t c0 = (uint32_t)r.l_seq << 4 | 4u, c1 = rlen << 4 | 3u;
		for (int i = 0; i < 4; ++i) put(w, o, (uint8_t)(c0 >> (8 * i)));
		for (int i = 0; i < 4; ++i) put(w, o, (uint8_t)(c1 >> (8 * i)));
	}
	const uint8_t* sq = r.cigar + 4ull * r.n_cigar_raw;   // seq, qual, aux
	const uint8_t* tag0 = g.tag; const uint8_t* tag1 = g.tag + 8 + 4ull * g.n; const uint8_t* e = rec_end(r);
	for (const uint8_t* x = sq; x < tag0; ++x) put(w, o, *x);
	for (const uint8_t* x = tag1; x < e; ++x) put(w, o, *x);
	if (!inl) for (const uint8_t* x = tag0; x < tag1; ++x) put(w, o, *x);
}

// the records that leave as they came, one wave per record: src(i) is record i's first byte, mask(i) the bits OR-ed into its flag word. Sparse: some records
// add nothing (sz 0: they belong to another stream) and are skipped before their position is read; where every record is written the test would only hold back
// the load of off[i] (measured: 0.5 % of the kernel). A wave copies about four records, so its prologue counts: the mask comes last, which keeps the pointers in
// one 32-byte load of the kernel arguments. off: absolute stream positions; ws: the stream position of obuf[0]
struct FromTile { const uint8_t* __restrict__ infl; const int64_t* __restrict__ recoff; __device__ const uint8_t* operator()(int64_t i) const { return infl + recoff[i]; } };
struct FromPtrs { const uint64_t* __restrict__ src; __device__ const uint8_t* operator()(int64_t i) const { return (const uint8_t*)(uintptr_t)src[i]; } };
struct NoMask { __device__ uint32_t operator()(int64_t) const { return 0; } };
template <bool Sparse, typename Src, typename Mask>
__global__ __launch_bounds__(256) void gather_kernel(Src src, const uint64_t* __restrict__ sz, const uint64_t* __restrict__ off, int64_t n, int64_t ws, Win w, Mask mask)
{
	const int lane = threadIdx.x & 63;
	const int64_t nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
	for (int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; i < n; i += nw)
	{
		if (Sparse && !sz[i]) continue;
		const int64_t pos = (int64_t)off[i] - ws;
		if (pos >= w.hi || pos + (int64_t)sz[i] <= w.lo) continue;
		write_record(src(i), w, pos, lane, mask(i));
	}
}
template <bool Sparse, typename Src, typename Mask> void launch_gather(Src src, Mask mask, const uint64_t* sz, const uint64_t* off, int64_t n, int64_t ws, const Win& w, hipStream_t s)
{
	hipLaunchKernelGGL((gather_kernel<Sparse, Src, Mask>), dim3(grid_for(n, 4)), dim3(256), 0, s, src, sz, off, n, ws, w, mask); KCHECK();
}

// the header: the input's bytes (magic, l_text, text, n_ref, refs); no @PG line (BamWriter::writeHeader copies the input's)
inline std::vector<uint8_t> bam_header_bytes(const ngsqc_handle* h)
{
	std::vector<uint8_t> hdr;
	auto put32 = [&](uint32_t v) { for (int i = 0; i < 4; ++i) hdr.push_back((uint8_t)(v >> (8 * i))); };
	hdr.insert(hdr.end(), {'B', 'A', 'M', 1}); put32((uint32_t)h->header_text.size()); hdr.insert(hdr.end(), h->header_text.begin(), h->header_text.end());
	put32((uint32_t)h->ref_names.size());
	for (size_t i = 0; i < h->ref_names.size(); ++i) { put32((uint32_t)h->ref_names[i].size() + 1); hdr.insert(hdr.end(), h->ref_names[i].begin(), h->ref_names[i].end()); hdr.push_back(0); put32((uint32_t)h->ref_lens[i]); }
	return hdr;
}

// the output file and, in members of its own, the header
inline void open_bam(BgzfStream& out, const char* path, const ngsqc_handle* h, hipStream_t s)
{
	out.sink.open(path, std::string("Could not open BAM/CRAM file for writing: ") + path);
	const std::vector<uint8_t> hdr = bam_header_bytes(h);
	out.put_host(hdr.data(), hdr.size(), s, h->device);
}

// one byte per record of the file into out[0, cap): run(c, rec, n) queues the tool's kernels for the resident tile and returns the device pointer to its n bytes.
// Returns the number of records
template <typename F> int64_t for_each_tile_bytes(ngsqc_handle* h, uint8_t* out, int64_t cap, const char* too_small_msg, F run)
{
	hipStream_t s = h->stream;
	int64_t done = 0;
	EagerRecoff eager(h);
	stream_tiles(h, [&](const TileCtx& c) {
		const int64_t n = c.n_rec;
		if (n == 0) return true;
		if (done + n > cap) throw ArgError(too_small_msg);
		const uint8_t* d = run(c, ensure_recoff(h), n);
		HIPCHK(hipMemcpyAsync(out + done, d, (size_t)n, hipMemcpyDeviceToHost, s)); HIPCHK(hipStreamSynchronize(s));
		done += n;
		return true;
	});
	return done;
}

// record i of the resident tile for an error message: its offset in the tile, its first bytes and its name. Waits for the stream (twice): what the caller
// queued in front is on the host as well
struct RecHead { int64_t off = 0; uint8_t head[36 + 256] = {0}; std::string name; };
inline RecHead fetch_rec_head(const TileCtx& c, const int64_t* rec, int64_t i, hipStream_t s)
{
	RecHead r;
	HIPCHK(hipMemcpyAsync(&r.off, rec + i, 8, hipMemcpyDeviceToHost, s)); HIPCHK(hipStreamSynchronize(s));
	HIPCHK(hipMemcpyAsync(r.head, c.infl + r.off, (size_t)std::min<int64_t>((int64_t)sizeof(r.head), c.total - r.off), hipMemcpyDeviceToHost, s)); HIPCHK(hipStreamSynchronize(s));
	r.name.assign((const char*)r.head + 36, strnlen((const char*)r.head + 36, r.head[12]));
	return r;
}
} // namespace
} // namespace ngsqc
