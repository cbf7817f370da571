// One to three FASTQ texts in device memory -> the per-entry FASTQ-to-FASTQ tools (src/FastqTrim, src/FastqExtract, src/FastqExtractUMI, src/FastqConvert,
// src/FastqExtractBarcode, src/FastqAddBarcode, src/FastqDownsample, src/FastqConcat): every entry is edited and written again.
//   shape       fe_shape (fqedit_visit.h): the input sides and output streams of an operation and the side every stream reads. The old four have stream k on
//               side k; FastqExtractBarcode writes two streams from one side, FastqAddBarcode two streams from three sides.
//   line index  the kernels of fastqin.hip (launch_fastq_line_index), once per side. Entry r is lines 4r .. 4r + 3 of its side.
//   plan        one record of 8 int32 per entry and stream (fqedit_visit.h): keep, the insertion into the header, the kept ranges of the bases and quality lines,
//               the quality delta. fe_plan_kernel: ONE LANE PER ENTRY where the plan is arithmetic on the line lengths (Trim, Convert, UMI; UMI looks for the first
//               space of the header). fe_extract_kernel validates every cycle and looks the id up in the table: a lane per entry as ex_match_kernel does for
//               short reads, ONE WAVE PER ENTRY with long_read (lanes striding over the cycles, lane 0 hashes the id and probes). FastqDownsample's keep bit of
//               pair ordinal r is a byte of the decision stream of downsample.hip (keep_stream.h), made on the device for the ordinals of the feed.
//   id table    FastqExtract: open-addressed slots {hash, id index} of a power of two and at least twice the ids, linear probing, hashed by join.h's name_hash
//               (NGSQC_NAME_HASH_BITS truncates it); offset, length and payload per id in arrays of their own. The host resolves duplicates before the upload, so
//               insertion is a compare-and-swap per id and nothing else; a hash hit is confirmed by the length and the bytes.
//   format      fe_sizes_kernel (the bytes an entry gives its stream; the counters of the statistics) -> BgzfStream::place -> fe_format_kernel: one wave per
//               entry writes the bytes of the entry that fall inside the stream's window (fe_entry_byte); the windows are deflated on the device.
//   headers     FastqDownsample -test: fe_header_sizes_kernel -> exclusive sum -> fe_header_copy_kernel gather the header lines of the kept pairs into one text.
// The accumulator (ngsqc_fqedit) takes the texts in pieces cut anywhere, as ngsqc_purge does: the entries of a feed are those complete on every side, the rest
// waits as the side's carry. Both do it through FastqFeed (fastq_feed.h) and write through FastqOutputs (fastq_outputs.h); the reference's messages are fastq_text.h's.
#include "join.h"
#include "fqedit_visit.h"
#include "keep_stream.h"
#include <unordered_map>

namespace ngsqc {
namespace {
constexpr uint64_t FE_SLOT_EMPTY = ~0ull;
struct FeSide { const uint8_t* text; const uint32_t* lines; uint64_t L; };
struct FeTable { const ulonglong2* slots; uint64_t slot_mask, hash_mask; const uint8_t* bytes; const uint64_t* id_off; const uint32_t* id_len; const int32_t* payload; };
// streams, src: fe_shape of the operation; keep: the decision byte of entry r of the feed (FastqDownsample)
struct FeArgs { FeSide s[FE_MAX_SIDES]; int sides, streams, src[FE_MAX_STREAMS]; int64_t n; unsigned long long entry_base; FeParams P; int32_t* plan; unsigned long long* err; FeTable t; const uint8_t* keep; };
__device__ __forceinline__ FqEntry fe_entry_of(const FeArgs& a, int side, int64_t r) { return fq_entry(a.s[side].text, a.s[side].lines, a.s[side].L, (uint64_t)r); }

__device__ __forceinline__ int32_t fe_lookup(const FeTable& t, const uint8_t* id, uint32_t len)
{
	if (!t.slots || !len) return FE_ABSENT;   // (the empty id is never listed)
	const uint64_t h = name_hash(id, (int)len) & t.hash_mask;
	for (uint64_t s = h & t.slot_mask;; s = (s + 1) & t.slot_mask)
	{
		const ulonglong2 e = t.slots[s];
		if (e.y == FE_SLOT_EMPTY) return FE_ABSENT;
		if (e.x != h || t.id_len[e.y] != len) continue;
		const uint8_t* p = t.bytes + t.id_off[e.y];
		bool same = true;
		for (uint32_t i = 0; i < len && same; ++i) same = p[i] == id[i];
		if (same) return t.payload[e.y];
	}
}
} // namespace

// slots: all words FE_SLOT_EMPTY; the ids are distinct
__global__ __launch_bounds__(256) void fe_insert_kernel(const uint64_t* __restrict__ id_off, const uint32_t* __restrict__ id_len, int64_t n, const uint8_t* __restrict__ bytes,
                                                        uint64_t hash_mask, uint64_t slot_mask, unsigned long long* slots /* [slot][2] */)
{
	const int64_t stride = (int64_t)gridDim.x * blockDim.x;
	for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
	{
		const uint64_t h = name_hash(bytes + id_off[i], (int)id_len[i]) & hash_mask;
		for (uint64_t s = h & slot_mask;; s = (s + 1) & slot_mask)
			if (atomicCAS(&slots[2 * s + 1], (unsigned long long)FE_SLOT_EMPTY, (unsigned long long)i) == FE_SLOT_EMPTY) { slots[2 * s] = h; break; }   // (the hash word is read behind this kernel only)
	}
}

// Trim, Convert, UMI, and the four tools whose plan is arithmetic on the line lengths, the header's first space or a decision byte: a lane per entry
__global__ __launch_bounds__(256) void fe_plan_kernel(const FeArgs a)
{
	const int64_t stride = (int64_t)gridDim.x * blockDim.x;
	for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < a.n; r += stride)
	{
		const FqEntry e = fq_entry(a.s[0].text, a.s[0].lines, a.s[0].L, (uint64_t)r);
		int32_t* row = a.plan + (int64_t)FE_PLAN * a.streams * r;
		if (a.P.op == FE_OP_TRIM) fe_plan_trim(row, a.P, e.bases.len, e.quals.len);
		else if (a.P.op == FE_OP_CONVERT) fe_plan_convert(row, e.bases.len, e.quals.len);
		else if (a.P.op == FE_OP_COPY) fe_plan_keep(row, 1u, e.bases.len, e.quals.len);
		else if (a.P.op == FE_OP_BARCODE_CUT)
		{
			fe_plan_barcode_main(row, (uint32_t)a.P.cut1, e.bases.len, e.quals.len);
			fe_plan_barcode_index(row + FE_PLAN, (uint32_t)a.P.cut1, e.bases.len, e.quals.len);
		}
		else if (a.P.op == FE_OP_DOWNSAMPLE)
		{
			const FqEntry e2 = fe_entry_of(a, 1, r);
			const uint32_t keep = a.keep[r];
			fe_plan_keep(row, keep, e.bases.len, e.quals.len);
			fe_plan_keep(row + FE_PLAN, keep, e2.bases.len, e2.quals.len);
		}
		else if (a.P.op == FE_OP_BARCODE_ADD)
		{
			const uint32_t len3 = fe_entry_of(a, 2, r).bases.len;
			fe_plan_addbarcode(row, a.s[0].text, e, len3);
			fe_plan_addbarcode(row + FE_PLAN, a.s[1].text, fe_entry_of(a, 1, r), len3);
		}
		else
		{
			const FqEntry e2 = fq_entry(a.s[1].text, a.s[1].lines, a.s[1].L, (uint64_t)r);
			const uint32_t ins = fe_umi_len(fe_umi_of(a.s[0].text, e, a.s[1].text, e2, a.P.cut1, a.P.cut2));
			fe_plan_umi(row, a.s[0].text, e, (uint32_t)a.P.cut1, ins);
			fe_plan_umi(row + FE_PLAN, a.s[1].text, e2, (uint32_t)a.P.cut2, ins);
		}
	}
}

// Extract: NL lanes per entry (1, or the 64 of a wave). The first failing (entry, kind) by atomicMin, as fq_entry_kernel leaves it.
template <int NL> __global__ __launch_bounds__(256) void fe_extract_kernel(const FeArgs a)
{
	const uint32_t lane = NL == 64 ? (threadIdx.x & 63u) : 0u;
	const int64_t unit = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / NL, n_units = ((int64_t)gridDim.x * blockDim.x) / NL;
	const uint8_t* __restrict__ text = a.s[0].text;
	for (int64_t r = unit; r < a.n; r += n_units)   // (with NL = 64 r is the same in every lane of a wave: the ballots below see whole waves)
	{
		const FqEntry e = fq_entry(text, a.s[0].lines, a.s[0].L, (uint64_t)r);
		uint32_t kind = fe_entry_kind(text, e);
		if (!kind && e.header.len)
		{
			const uint8_t* __restrict__ b = text + e.bases.start; const uint8_t* __restrict__ q = text + e.quals.start;
			uint32_t bad = 0;
			for (uint32_t i = lane; i < e.bases.len; i += NL) bad |= fe_cycle_bad(b[i], q[i], a.P.long_read);
			bool bb = bad & 1u, bq = bad & 2u;
			if (NL == 64) { bb = __builtin_amdgcn_ballot_w64(bb) != 0; bq = __builtin_amdgcn_ballot_w64(bq) != 0; }
			kind = fq_char_kind(false, bb, bq);
		}
		if (lane == 0)
		{
			if (kind) atomicMin(a.err, fq_error_word(a.entry_base + (unsigned long long)r, kind));
			uint32_t at, len; fe_id_range(text, e.header, at, len);
			fe_plan_extract(a.plan + (int64_t)FE_PLAN * r, fe_lookup(a.t, text + at, len), a.P.invert, e.bases.len, e.quals.len);
		}
	}
}

// sz[k][r]: the bytes entry r gives stream k (stream k takes side src[k]); counts[k] / counts[2 + k]: entries and bytes of stream k
__global__ __launch_bounds__(256) void fe_sizes_kernel(const FeArgs a, uint64_t* __restrict__ sz0, uint64_t* __restrict__ sz1, unsigned long long* __restrict__ counts)
{
	const int64_t stride = (int64_t)gridDim.x * blockDim.x;
	const int64_t rounds = (a.n + stride - 1) / stride;   // (every lane of a wave makes the same number of rounds: the wave sums see whole waves)
	int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	long long c[2] = {0, 0}, b[2] = {0, 0};
	for (int64_t i = 0; i < rounds; ++i, r += stride)
	{
		if (r >= a.n) continue;
		for (int k = 0; k < a.streams; ++k)
		{
			const int32_t* row = a.plan + FE_PLAN * ((int64_t)a.streams * r + k);
			const uint64_t n = fe_entry_bytes(row, fe_entry_of(a, a.src[k], r));
			(k ? sz1 : sz0)[r] = n;
			c[k] += row[FE_KEEP] ? 1 : 0; b[k] += (long long)n;
		}
	}
	for (int k = 0; k < 2; ++k)
	{
		const long long wc = wave_sum(c[k]), wb = wave_sum(b[k]);
		if ((threadIdx.x & 63) == 0) { if (wc) atomicAdd(&counts[k], (unsigned long long)wc); if (wb) atomicAdd(&counts[2 + k], (unsigned long long)wb); }
	}
}

// one wave per entry of stream k: the bytes of the entry that fall inside the window
__global__ __launch_bounds__(256) void fe_format_kernel(const FeArgs a, int k, const uint64_t* __restrict__ sz, const uint64_t* __restrict__ off, int64_t ws, Win w)
{
	const int lane = threadIdx.x & 63;
	const int64_t nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
	const int side = a.src[k];
	const uint8_t* __restrict__ text = a.s[side].text;
	for (int64_t r = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; r < a.n; r += nw)
	{
		const int64_t size = (int64_t)sz[r];
		if (!size) continue;
		const int64_t pos = (int64_t)off[r] - ws;
		const int64_t lo = max(pos, w.lo), hi = min(pos + size, w.hi);
		if (lo >= hi) continue;
		const FqEntry e = fe_entry_of(a, side, r);
		const int32_t* row = a.plan + FE_PLAN * ((int64_t)a.streams * r + k);
		FeIns u{};
		if (a.P.op == FE_OP_UMI) u = fe_ins_umi(fe_umi_of(a.s[0].text, k == 0 ? e : fe_entry_of(a, 0, r), a.s[1].text, k == 1 ? e : fe_entry_of(a, 1, r), a.P.cut1, a.P.cut2));
		else if (a.P.op == FE_OP_BARCODE_ADD) u = fe_ins_barcode(a.s[2].text, fe_entry_of(a, 2, r));
		for (int64_t x = lo + lane; x < hi; x += 64) w.base[x] = fe_entry_byte(text, e, row, (uint64_t)(x - pos), u);
	}
}

// FastqDownsample -test: hsz[r] = the bytes the header line of side 0 gives the text of kept headers (the line and its "\n"; 0 for a dropped pair) ...
__global__ __launch_bounds__(256) void fe_header_sizes_kernel(const FeArgs a, uint64_t* __restrict__ hsz)
{
	const int64_t stride = (int64_t)gridDim.x * blockDim.x;
	for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < a.n; r += stride)
		hsz[r] = fe_header_bytes(a.plan + FE_PLAN * (int64_t)a.streams * r, fe_entry_of(a, 0, r));
}
// ... and, behind their exclusive sum hoff, the copy: one wave per kept pair. out holds hoff[n - 1] + hsz[n - 1] bytes.
__global__ __launch_bounds__(256) void fe_header_copy_kernel(const FeArgs a, const uint64_t* __restrict__ hsz, const uint64_t* __restrict__ hoff, uint8_t* __restrict__ out)
{
	const int lane = threadIdx.x & 63;
	const int64_t nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
	for (int64_t r = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; r < a.n; r += nw)
	{
		const uint64_t size = hsz[r];
		if (!size) continue;
		const FqEntry e = fe_entry_of(a, 0, r);
		uint8_t* d = out + hoff[r];
		for (uint64_t x = (uint64_t)lane; x < size; x += 64) d[x] = fe_header_byte(a.s[0].text, e, x);
	}
}
} // namespace ngsqc

// ---------------------------------------------------------------- the accumulator behind the C ABI
#include "fastq_feed.h"
#include "fastq_outputs.h"
using namespace ngsqc::lib;

struct ngsqc_fqedit
{
	std::string err; bool failed = false;
	FeParams P{}; int sides = 1, streams = 1; ngsqc::FeShape shape{}; const char* tool = "FastqTrim"; CallSwitches sw;
	FastqFeed in;   // (in front of out: fastq_outputs.h)
	std::unique_ptr<Timer> plan_clock;
	// the id table
	DevBuf<uint8_t> d_id_bytes; DevBuf<uint64_t> d_id_off; DevBuf<uint32_t> d_id_len; DevBuf<int32_t> d_id_payload; DevBuf<ulonglong2> d_slots; uint64_t slot_mask = 0; bool has_ids = false;
	DevBuf<int32_t> d_plan; DevBuf<unsigned long long> d_err, d_counts;
	FastqOutputs out;
	std::vector<int32_t> all_plan;
	ngsqc_fqedit_stats st{};
	int64_t seen[3] = {0, 0, 0};   // entries of every side, those no partner came for included
	// FastqDownsample: the decision stream, and with want_headers the header lines of the kept pairs
	KeepStream* keep = nullptr; bool want_headers = false; DevBuf<uint64_t> d_hsz, d_hoff; DevBuf<uint8_t> d_headers; std::string headers;
	~ngsqc_fqedit() { keep_stream_close(keep); }

	void init(int dev, const ngsqc_fqedit_params* p)
	{
		if (!p) throw ArgError("ngsqc_fqedit_create: no parameters");
		static const char* names[FE_N_OPS] = {"FastqTrim", "FastqExtract", "FastqExtractUMI", "FastqConvert", "FastqExtractBarcode", "FastqAddBarcode", "FastqDownsample", "FastqConcat"};
		if (p->op < 0 || p->op >= FE_N_OPS) throw ArgError("ngsqc_fqedit_create: no such operation: " + std::to_string(p->op));
		if (p->start < 0 || p->end < 0 || p->len < 0 || p->max_len < 0) throw ArgError("start, end, len and max_len must not be negative!");
		if (p->cut1 < 0 || p->cut2 < 0) throw ArgError("cut1 and cut2 must not be negative!");
		P.op = p->op; P.long_read = p->long_read ? 1 : 0; P.start = p->start; P.end = p->end; P.len = p->len; P.max_len = p->max_len; P.cut1 = p->cut1; P.cut2 = p->cut2; P.invert = p->invert ? 1 : 0;
		shape = ngsqc::fe_shape(P.op); sides = shape.sides; streams = shape.streams; tool = names[P.op];
		in.open(dev, sides); st.err_entry = -1;
		plan_clock.reset(new Timer(in.stream)); out.init(tool, streams, in.device, in.stream);
		d_err.alloc(1); d_counts.alloc(4);
		HIPCHK(hipMemsetAsync(d_err.p, 0xff, 8, in.stream)); HIPCHK(hipMemsetAsync(d_counts.p, 0, 4 * 8, in.stream));
		HIPCHK(hipStreamSynchronize(in.stream));
	}
	void ids(const uint8_t* names, const int32_t* name_len, const int32_t* lengths, int64_t n)
	{
		if (P.op != FE_OP_EXTRACT) throw ArgError("ngsqc_fqedit_ids: only FastqExtract takes ids");
		if (has_ids || st.entries) throw ArgError("ngsqc_fqedit_ids: the ids are set once, before the first feed");
		if (n < 0 || (n && (!names || !name_len))) throw ArgError("ngsqc_fqedit_ids: invalid ids");
		HIPCHK(hipSetDevice(in.device));
		// QHash::insert (main.cpp:51): a later duplicate replaces the earlier one
		std::unordered_map<std::string, int32_t> m;
		uint64_t o = 0;
		for (int64_t i = 0; i < n; ++i)
		{
			if (name_len[i] < 0) throw ArgError("negative id length");
			m[std::string((const char*)names + o, (size_t)name_len[i])] = lengths ? lengths[i] : FE_NO_LENGTH;
			o += (uint64_t)name_len[i];
		}
		std::vector<uint8_t> bytes; std::vector<uint64_t> off; std::vector<uint32_t> len; std::vector<int32_t> payload;
		for (auto& kv : m)
		{
			if (kv.second == FE_ABSENT || kv.first.empty()) continue;   // (ids.value(id, -2) cannot tell such an id from one that is not listed; no entry has the empty id in the table: see fe_lookup)
			off.push_back(bytes.size()); len.push_back((uint32_t)kv.first.size()); payload.push_back(kv.second);
			bytes.insert(bytes.end(), kv.first.begin(), kv.first.end());
		}
		has_ids = true;
		const int64_t k = (int64_t)off.size();
		if (!k) return;
		uint64_t cap = 64;
		while (cap < 2 * (uint64_t)k) cap <<= 1;
		slot_mask = cap - 1;
		const char* what = "the table of ids";
		grow(d_id_bytes, bytes.size() + 1, what, tool); grow(d_id_off, (size_t)k, what, tool); grow(d_id_len, (size_t)k, what, tool); grow(d_id_payload, (size_t)k, what, tool); grow(d_slots, (size_t)cap, what, tool);
		if (!bytes.empty()) HIPCHK(hipMemcpyAsync(d_id_bytes.p, bytes.data(), bytes.size(), hipMemcpyHostToDevice, in.stream));
		HIPCHK(hipMemcpyAsync(d_id_off.p, off.data(), (size_t)k * 8, hipMemcpyHostToDevice, in.stream)); HIPCHK(hipMemcpyAsync(d_id_len.p, len.data(), (size_t)k * 4, hipMemcpyHostToDevice, in.stream));
		HIPCHK(hipMemcpyAsync(d_id_payload.p, payload.data(), (size_t)k * 4, hipMemcpyHostToDevice, in.stream));
		HIPCHK(hipMemsetAsync(d_slots.p, 0xff, (size_t)cap * 16, in.stream));
		hipLaunchKernelGGL(ngsqc::fe_insert_kernel, dim3(grid_for(k)), dim3(256), 0, in.stream, d_id_off.p, d_id_len.p, k, d_id_bytes.p, name_hash_mask(sw.name_hash_bits), slot_mask, (unsigned long long*)d_slots.p); KCHECK();
		HIPCHK(hipStreamSynchronize(in.stream));   // (the host vectors go)
	}
	void downsample(uint32_t seed, double percentage, int headers_too)
	{
		if (P.op != FE_OP_DOWNSAMPLE) throw ArgError("ngsqc_fqedit_downsample: only FastqDownsample takes a seed and a percentage");
		if (keep || st.entries || seen[0] || seen[1]) throw ArgError("ngsqc_fqedit_downsample: the seed and the percentage are set once, before the first feed");
		HIPCHK(hipSetDevice(in.device));
		keep = keep_stream_open(tool, seed, percentage); want_headers = headers_too != 0;
	}
	void outputs(const char* o1, const char* o2, int level)
	{
		if (out.opened || st.entries) throw ArgError("ngsqc_fqedit_outputs: the outputs are set once, before the first feed");
		if (!o1) throw ArgError("ngsqc_fqedit_outputs: out1 is needed");
		if ((streams == 2) != (o2 != nullptr)) throw ArgError(streams == 2 ? "ngsqc_fqedit_outputs: out2 is needed" : "ngsqc_fqedit_outputs: this operation has one output");
		if (level < 0 || level > 9) throw ArgError("compression level " + std::to_string(level) + " is not in 0..9");
		const char* paths[4] = {o1, o2, nullptr, nullptr};
		out.open(paths, write_window_bytes(sw.write_window_pieces), level);
	}
	// the reference's message for the entry the device named (FastqFileStream.cpp:3-44), from the host's copy of the text
	void build_error(unsigned long long word)
	{
		const uint64_t entry = word >> 8, r = entry - (uint64_t)st.entries; const int kind = (int)(word & 255);
		std::string ln[4]; in.entry_lines(0, r, ln);
		err = fq_validate_message(kind, ln, P.long_read); failed = true; st.err_entry = (int64_t)entry; st.err_kind = kind;
	}
	FeArgs args(int64_t n) const
	{
		FeArgs a{};
		for (int k = 0; k < sides; ++k) a.s[k] = FeSide{in.side[k].d_text.p, in.side[k].d_lines.p, in.side[k].L};
		a.sides = sides; a.streams = streams; for (int k = 0; k < FE_MAX_STREAMS; ++k) a.src[k] = shape.src[k];
		a.n = n; a.entry_base = (unsigned long long)st.entries; a.P = P; a.plan = d_plan.p; a.err = d_err.p;
		a.t = FeTable{d_slots.p, slot_mask, name_hash_mask(sw.name_hash_bits), d_id_bytes.p, d_id_off.p, d_id_len.p, d_id_payload.p};
		return a;
	}
	// a feed behind the last piece of a file begins the next file (FastqConcat, FastqAddBarcode's lists): positions and ordinals carry on
	int feed(const char* who, const uint8_t* t1, int64_t n1, const uint8_t* t2, int64_t n2, const uint8_t* t3, int64_t n3, int last)
	{
		if (n1 < 0 || n2 < 0 || n3 < 0 || (n1 && !t1) || (n2 && !t2) || (n3 && !t3)) throw ArgError(std::string(who) + ": invalid text");
		if ((sides == 1 && n2) || (sides < 3 && n3)) throw ArgError(std::string(who) + (sides == 1 ? ": this operation has one input" : ": this operation has two inputs"));
		if (out.finished) throw ArgError(std::string(who) + ": the outputs are closed");
		if (P.op == FE_OP_DOWNSAMPLE && !keep) throw ArgError(std::string(who) + ": ngsqc_fqedit_downsample comes before the first feed");
		if (failed) return NGSQC_E_FORMAT;
		HIPCHK(hipSetDevice(in.device));
		const uint8_t* tx[3] = {t1, t2, t3}; const int64_t nn[3] = {n1, n2, n3};
		const int64_t n = in.feed(who, tx, nn, last != 0, st.h2d_ms, st.index_ms, st.wait_ms);
		if (n < 0) return NGSQC_OK;
		for (int k = 0; k < sides; ++k) seen[k] += last ? (int64_t)in.side[k].E : n;
		hipStream_t stream = in.stream;
		if (n)
		{
			d_plan.ensure_slack((size_t)n * FE_PLAN * streams);
			FeArgs a = args(n);
			plan_clock->start();
			if (keep) a.keep = keep_stream_run(keep, st.entries, n, stream);   // (the pair ordinals of this feed; the stream was waited for in in.feed)
			if (P.op != FE_OP_EXTRACT) { hipLaunchKernelGGL(ngsqc::fe_plan_kernel, dim3(grid_for(n)), dim3(256), 0, stream, a); KCHECK(); }
			else if (P.long_read) { hipLaunchKernelGGL(ngsqc::fe_extract_kernel<64>, dim3(grid_for(n, 4)), dim3(256), 0, stream, a); KCHECK(); }
			else { hipLaunchKernelGGL(ngsqc::fe_extract_kernel<1>, dim3(grid_for(n)), dim3(256), 0, stream, a); KCHECK(); }
			plan_clock->mark();
			unsigned long long e_word = FQ_NO_ERROR;
			HIPCHK(hipMemcpyAsync(&e_word, d_err.p, 8, hipMemcpyDeviceToHost, stream));
			if (!out.opened)
			{
				const size_t at = all_plan.size();
				all_plan.resize(at + (size_t)n * FE_PLAN * streams);
				HIPCHK(hipMemcpyAsync(all_plan.data() + at, d_plan.p, (size_t)n * FE_PLAN * streams * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
			}
			const double w1 = wall_ms();
			HIPCHK(hipStreamSynchronize(stream));
			st.wait_ms += wall_ms() - w1;
			st.plan_ms += plan_clock->elapsed();
			if (e_word != FQ_NO_ERROR) { build_error(e_word); return NGSQC_E_FORMAT; }
			write_out(a);
			if (want_headers) kept_headers_of(a);
			st.entries += n;
		}
		// the carry: what lies behind the last entry on either side; behind the last piece the longer side's surplus is left alone (main.cpp:48 of FastqExtractUMI)
		in.cut_carry(n, last != 0);
		return NGSQC_OK;
	}
	void write_out(const FeArgs& a)
	{
		const int64_t n = a.n;
		out.begin(n);
		hipLaunchKernelGGL(ngsqc::fe_sizes_kernel, dim3(grid_for(n)), dim3(256), 0, in.stream, a, out.d_sz[0].p, out.d_sz[1].p, d_counts.p); KCHECK();
		if (!out.opened) return;
		out.write(n, st.format_ms, st.deflate_ms, [&](int k, const Win& win, int64_t ws) {
			hipLaunchKernelGGL(ngsqc::fe_format_kernel, dim3(grid_for(n, 4)), dim3(256), 0, in.stream, a, k, out.d_sz[k].p, out.d_off[k].p, ws, win); KCHECK();
		});
	}
	// sizes -> exclusive positions -> copy, then the text of this feed's kept headers goes behind that of the earlier feeds
	void kept_headers_of(const FeArgs& a)
	{
		const int64_t n = a.n; hipStream_t stream = in.stream;
		grow(d_hsz, (size_t)n + 1, "the kept headers", tool); grow(d_hoff, (size_t)n + 1, "the kept headers", tool);
		hipLaunchKernelGGL(ngsqc::fe_header_sizes_kernel, dim3(grid_for(n)), dim3(256), 0, stream, a, d_hsz.p); KCHECK();
		scan_u64(out.d_scan_tmp, d_hsz.p, d_hoff.p, 0, (size_t)n, stream);   // (write_out's begin made room for n values)
		uint64_t tot[2] = {0, 0};
		HIPCHK(hipMemcpyAsync(&tot[0], d_hoff.p + n - 1, 8, hipMemcpyDeviceToHost, stream)); HIPCHK(hipMemcpyAsync(&tot[1], d_hsz.p + n - 1, 8, hipMemcpyDeviceToHost, stream));
		HIPCHK(hipStreamSynchronize(stream));
		const size_t nb = (size_t)(tot[0] + tot[1]), at = headers.size();
		if (!nb) return;
		grow(d_headers, nb, "the kept headers", tool);
		hipLaunchKernelGGL(ngsqc::fe_header_copy_kernel, dim3(grid_for(n, 4)), dim3(256), 0, stream, a, d_hsz.p, d_hoff.p, d_headers.p); KCHECK();
		headers.resize(at + nb);
		HIPCHK(hipMemcpyAsync(&headers[at], d_headers.p, nb, hipMemcpyDeviceToHost, stream)); HIPCHK(hipStreamSynchronize(stream));
	}
	void result(ngsqc_fqedit_stats* o)
	{
		HIPCHK(hipSetDevice(in.device));
		if (!failed) out.finish();
		unsigned long long c[4] = {0, 0, 0, 0};
		HIPCHK(hipMemcpyAsync(c, d_counts.p, sizeof(c), hipMemcpyDeviceToHost, in.stream)); HIPCHK(hipStreamSynchronize(in.stream));
		for (int k = 0; k < 2; ++k) { st.written[k] = (int64_t)c[k]; st.bytes[k] = (int64_t)c[2 + k]; }
		if (o) *o = st;
	}
};

namespace { thread_local std::string g_fqedit_error; }

extern "C" {
int ngsqc_fqedit_create(int32_t device, const ngsqc_fqedit_params* params, ngsqc_fqedit** out)
{
	if (!out) return NGSQC_E_ARG;
	*out = nullptr;
	return fastq_guard((ngsqc_fqedit*)nullptr, g_fqedit_error, [&] { std::unique_ptr<ngsqc_fqedit> e(new ngsqc_fqedit); e->init(device, params); *out = e.release(); return NGSQC_OK; });
}
void ngsqc_fqedit_destroy(ngsqc_fqedit* e) { delete e; }
const char* ngsqc_fqedit_last_error(const ngsqc_fqedit* e) { return e ? e->err.c_str() : g_fqedit_error.c_str(); }
int ngsqc_fqedit_ids(ngsqc_fqedit* e, const void* names, const int32_t* name_len, const int32_t* lengths, int64_t n)
{
	if (!e) return NGSQC_E_ARG;
	return fastq_guard(e, g_fqedit_error, [&] { e->ids((const uint8_t*)names, name_len, lengths, n); return NGSQC_OK; });
}
int ngsqc_fqedit_outputs(ngsqc_fqedit* e, const char* out1, const char* out2, int32_t compression_level)
{
	if (!e) return NGSQC_E_ARG;
	return fastq_guard(e, g_fqedit_error, [&] { e->outputs(out1, out2, compression_level); return NGSQC_OK; });
}
int ngsqc_fqedit_feed(ngsqc_fqedit* e, const uint8_t* text1, int64_t n1, const uint8_t* text2, int64_t n2, int32_t last)
{
	if (!e) return NGSQC_E_ARG;
	return fastq_guard(e, g_fqedit_error, [&] {
		if (e->sides == 3) throw ArgError("ngsqc_fqedit_feed: FastqAddBarcode has three inputs: ngsqc_fqedit_feed3");
		return e->feed("ngsqc_fqedit_feed", text1, n1, text2, n2, nullptr, 0, last); });
}
int ngsqc_fqedit_feed3(ngsqc_fqedit* e, const uint8_t* text1, int64_t n1, const uint8_t* text2, int64_t n2, const uint8_t* text3, int64_t n3, int32_t last)
{
	if (!e) return NGSQC_E_ARG;
	return fastq_guard(e, g_fqedit_error, [&] { return e->feed("ngsqc_fqedit_feed3", text1, n1, text2, n2, text3, n3, last); });
}
int ngsqc_fqedit_downsample(ngsqc_fqedit* e, uint32_t seed, double percentage, int32_t want_headers)
{
	if (!e) return NGSQC_E_ARG;
	return fastq_guard(e, g_fqedit_error, [&] { e->downsample(seed, percentage, want_headers); return NGSQC_OK; });
}
int ngsqc_fqedit_side_entries(const ngsqc_fqedit* e, int64_t out[3])
{
	if (!e || !out) return NGSQC_E_ARG;
	for (int k = 0; k < 3; ++k) out[k] = e->seen[k];
	return NGSQC_OK;
}
int ngsqc_fqedit_kept_headers(ngsqc_fqedit* e, char** text, int64_t* n)
{
	if (!e) return NGSQC_E_ARG;
	return fastq_guard(e, g_fqedit_error, [&] {
		if (!text || !n) throw ArgError("ngsqc_fqedit_kept_headers: null argument");
		if (!e->want_headers) throw ArgError("ngsqc_fqedit_kept_headers: the headers are kept only when ngsqc_fqedit_downsample asked for them");
		if (!e->out.finished && !e->failed) throw ArgError("ngsqc_fqedit_kept_headers: ngsqc_fqedit_result comes first");
		*text = &e->headers[0]; *n = (int64_t)e->headers.size();
		return NGSQC_OK; });
}
int ngsqc_fqedit_result(ngsqc_fqedit* e, ngsqc_fqedit_stats* st)
{
	if (!e) return NGSQC_E_ARG;
	return fastq_guard(e, g_fqedit_error, [&] { e->result(st); return e->failed ? NGSQC_E_FORMAT : NGSQC_OK; });
}
int ngsqc_fqedit_plan(ngsqc_fqedit* e, int64_t first, int64_t n, int32_t* out)
{
	if (!e) return NGSQC_E_ARG;
	return fastq_guard(e, g_fqedit_error, [&] {
		if (e->out.opened) throw ArgError("ngsqc_fqedit_plan: the plan is kept only when no outputs are set");
		const int64_t w = (int64_t)FE_PLAN * e->streams;
		if (first < 0 || n < 0 || (n && !out) || (uint64_t)(first + n) * (uint64_t)w > e->all_plan.size()) throw ArgError("ngsqc_fqedit_plan: entries out of range");
		std::copy(e->all_plan.begin() + first * w, e->all_plan.begin() + (first + n) * w, out);
		return NGSQC_OK; });
}
}
