// The position table under the site pileup, the pileup candidates that ride the scan's chain walk, and the indel windows: the 1-based positions of a table of
// sites or windows in file order (sorted within a reference, the items of a reference in one run), a [first, last) index range per reference, and per reference
// with items one entry per 64 kb bucket naming the first item at or behind the bucket's start. The device view and its two lookups, and the host builder that
// every table goes through. The builder needs neither HIP nor handle.h: g++ compiles this header through tests/emul/device_on_cpu.h
// (tests/test_cpu_postable.py holds builder and lookups to bisect_left).
#pragma once
#include <cstdint>
#include <vector>

namespace ngsqc {

constexpr int PILEUP_BUCKET_SHIFT = 16;   // 64 kb position buckets per reference: bucket -> first item at or behind the bucket start

struct PosTable
{
	const int32_t* pos;           // [n] 1-based positions
	const int32_t* tid_first;     // [max(n_ref, 1)] items of reference t: [tid_first[t], tid_last[t])
	const int32_t* tid_last;
	const int32_t* bucket;        // buckets of reference t: bucket[tid_bucket0[t] .. tid_bucket0[t + 1]); none for a reference without items
	const int64_t* tid_bucket0;   // [n_ref + 1]
};

// The lookups ask for a reference that has items (tid_first[tid] < tid_last[tid]: its callers look first - a reference without items has no buckets).
// The index range [lo, hi) of the bucket that holds x: the first item at or behind x lies in [lo, hi], and in [lo, last) for any x behind the last bucket
__device__ __forceinline__ void postable_bucket(const PosTable& t, int tid, int last, int64_t x, int& lo, int& hi)
{
	const int64_t b0 = t.tid_bucket0[tid], nbk = t.tid_bucket0[tid + 1] - b0;
	int64_t bi = x > 0 ? x >> PILEUP_BUCKET_SHIFT : 0; if (bi >= nbk) bi = nbk - 1;
	lo = t.bucket[b0 + bi]; hi = bi + 1 < nbk ? t.bucket[b0 + bi + 1] : last;
}
// first item of reference tid with pos >= x, or last: a short scan from the bucket's first item (a sparse table: the sites of the pileup). x is a record's
// 1-based start (x <= 0 looks into the first bucket)
__device__ __forceinline__ int postable_lower_scan(const PosTable& t, int tid, int last, int x)
{
	int i, hi; postable_bucket(t, tid, last, x, i, hi);
	while (i < last && t.pos[i] < x) ++i;
	return i;
}
// the same by binary search inside the bucket (a dense table: the windows of a whole VCF); any x
__device__ __forceinline__ int postable_lower_bsearch(const PosTable& t, int tid, int first, int last, long long x)
{
	if (x <= 1) return first;
	int lo, hi; postable_bucket(t, tid, last, x, lo, hi);
	while (lo < hi) { const int m = (lo + hi) >> 1; if (t.pos[m] < x) lo = m + 1; else hi = m; }
	return lo;
}

// ---- the host builder ----
struct PosTableHost { std::vector<int32_t> pos, tid_first, tid_last, bucket; std::vector<int64_t> tid_bucket0; };
struct PosTableRules { const char* bad_tid; const char* unsorted; const char* split; };   // what the caller's items are told: reference id out of range / order inside a run / a reference that comes back

// (a) the runs: tid_first / tid_last of max(n_ref, 1) entries from items in file order (an Item has .tid). Per item: the reference id; each(i, item) - the
// caller's own checks (it throws what it likes) and whatever it collects of the item; in_order(previous, item) where the item continues a run, else the
// reference must not have had a run before. Err(message) is thrown.
template <class Err, class Item, class Each, class InOrder>
void postable_runs(const Item* items, int64_t n, int n_ref, const PosTableRules& rules, std::vector<int32_t>& tid_first, std::vector<int32_t>& tid_last, Each each, InOrder in_order)
{
	const size_t nt = (size_t)(n_ref > 1 ? n_ref : 1);
	tid_first.assign(nt, 0); tid_last.assign(nt, 0);
	std::vector<uint8_t> seen(nt, 0);
	for (int64_t i = 0; i < n; ++i)
	{
		const Item& r = items[i];
		if (r.tid < 0 || r.tid >= n_ref) throw Err(rules.bad_tid);
		each(i, r);
		if (i > 0 && items[i - 1].tid == r.tid) { if (!in_order(items[i - 1], r)) throw Err(rules.unsorted); }
		else { if (seen[(size_t)r.tid]) throw Err(rules.split); seen[(size_t)r.tid] = 1; tid_first[(size_t)r.tid] = (int32_t)i; }
		tid_last[(size_t)r.tid] = (int32_t)i + 1;
	}
}

// (b) the buckets from positions, runs and reference lengths: they reach one bucket behind the longer of the reference and its last position, so that every
// position of a record (a record may lie behind the end the header gives) finds a bucket; bucket is never empty (it is uploaded)
template <class Len>
void postable_buckets(PosTableHost& t, const Len* ref_lens, int n_ref)
{
	t.tid_bucket0.assign((size_t)n_ref + 1, 0); t.bucket.clear();
	for (int r = 0; r < n_ref; ++r)
	{
		t.tid_bucket0[(size_t)r] = (int64_t)t.bucket.size();
		int32_t i = t.tid_first[(size_t)r]; const int32_t last = t.tid_last[(size_t)r];
		if (i >= last) continue;
		const int64_t far = (int64_t)ref_lens[r] > t.pos[(size_t)last - 1] ? (int64_t)ref_lens[r] : t.pos[(size_t)last - 1];
		const int64_t nb = (far >> PILEUP_BUCKET_SHIFT) + 2;
		for (int64_t b = 0; b < nb; ++b) { const int64_t lo = b << PILEUP_BUCKET_SHIFT; while (i < last && t.pos[(size_t)i] < lo) ++i; t.bucket.push_back(i); }
	}
	t.tid_bucket0[(size_t)n_ref] = (int64_t)t.bucket.size();
	if (t.bucket.empty()) t.bucket.push_back(0);
}

} // namespace ngsqc
