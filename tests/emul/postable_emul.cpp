// The position table of the site pileup, its scan rider and the indel windows (ngs-bits_amd/csrc/postable.h: the host builder, and the two lookups as the GPU
// library compiles them into walk_scan_kernel, pileup_kernel, pileup_long_kernel and the window kernels) on the CPU: tests/test_cpu_postable.py holds them to
// bisect_left. The three rule sets restate what PileupState::begin, IndelState::begin and setup_regions (csrc/jobs.hip) hand to postable_runs - nouns, messages,
// the item's own checks and the order rule - so that the order of the first error is the callers'. Test infrastructure, never linked into the library.
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <vector>
#include "device_on_cpu.h"
#include "../../ngs-bits_amd/csrc/postable.h"

using namespace ngsqc;

extern "C" {

struct PtItem { int32_t tid, start, end, kind, len, has_allele, has_slice; };   // (kind .. has_slice: windows only; kind 0 none, 1 insertion, 2 deletion as include/ngsqc.h)
enum { PT_SITES = 0, PT_WINDOWS = 1, PT_REGIONS = 2 };
struct PtError : std::runtime_error { using std::runtime_error::runtime_error; };

// -> the table (postable_emul_free), or null with the message of the first error in err[256]
void* postable_emul_build(int rules, const PtItem* items, int64_t n, const int64_t* ref_lens, int32_t n_ref, char* err)
{
	static const char* const merged = "Merged and sorted BED file required for coverage details statistics!";
	static const PosTableRules R[3] = {
		{"site with invalid reference id", "sites must be sorted by position within a reference", "sites of one reference must be contiguous"},
		{"window with invalid reference id", "windows must be sorted by start within a reference", "windows of one reference must be contiguous"},
		{"region with invalid reference id", merged, merged}};
	PosTableHost* t = new PosTableHost; t->pos.resize((size_t)n);
	try
	{
		postable_runs<PtError>(items, n, n_ref, R[rules], t->tid_first, t->tid_last,
			[&](int64_t i, const PtItem& x) {
				if (rules == PT_SITES) { if (x.start < 1 || x.end != x.start) throw PtError("a site is a single 1-based position (start == end)"); }
				else if (x.start < 1 || x.end < x.start) throw PtError(rules == PT_WINDOWS ? "invalid window range" : "invalid region range");
				if (rules == PT_WINDOWS)
				{
					if (x.kind < 0 || x.kind > 2 || x.len < 0 || (x.kind != 0 && x.len > 0 && !x.has_allele)) throw PtError("invalid window allele");
					if (x.kind == 2 && x.len > 0 && !x.has_slice) throw PtError("a deletion window needs its reference slice");
				}
				t->pos[(size_t)i] = x.start;
			},
			[&](const PtItem& prev, const PtItem& x) { return rules == PT_REGIONS ? prev.end < x.start : prev.start <= x.start; });
		postable_buckets(*t, ref_lens, n_ref);
	}
	catch (const PtError& e) { delete t; strncpy(err, e.what(), 255); err[255] = 0; return nullptr; }
	err[0] = 0;
	return t;
}
void postable_emul_free(void* table) { delete (PosTableHost*)table; }

// the arrays as they are uploaded: which 0 pos, 1 tid_first, 2 tid_last, 3 bucket (int32), 4 tid_bucket0 (int64). -> the length; copied when out holds it
int64_t postable_emul_array(const void* table, int which, void* out, int64_t cap)
{
	const PosTableHost& t = *(const PosTableHost*)table;
	if (which == 4) { if ((int64_t)t.tid_bucket0.size() <= cap) memcpy(out, t.tid_bucket0.data(), t.tid_bucket0.size() * sizeof(int64_t)); return (int64_t)t.tid_bucket0.size(); }   // (n_ref + 1 entries: never empty)
	const std::vector<int32_t>& v = which == 0 ? t.pos : which == 1 ? t.tid_first : which == 2 ? t.tid_last : t.bucket;
	if (!v.empty() && (int64_t)v.size() <= cap) memcpy(out, v.data(), v.size() * sizeof(int32_t));
	return (int64_t)v.size();
}

// out[k] = the first item of reference tid at or behind xs[k]. form 0: postable_lower_scan (xs must fit int32), 1: postable_lower_bsearch. A reference
// without items is answered as every kernel answers it - they look at [first, last) before they look anything up
void postable_emul_lower(const void* table, int form, int32_t tid, const int64_t* xs, int64_t n, int32_t* out)
{
	const PosTableHost& h = *(const PosTableHost*)table;
	const PosTable t{h.pos.data(), h.tid_first.data(), h.tid_last.data(), h.bucket.data(), h.tid_bucket0.data()};
	const int first = t.tid_first[tid], last = t.tid_last[tid];
	for (int64_t k = 0; k < n; ++k)
		out[k] = first >= last ? first : form == 0 ? postable_lower_scan(t, tid, last, (int)xs[k]) : postable_lower_bsearch(t, tid, first, last, (long long)xs[k]);
}

}
