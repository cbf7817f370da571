// BamToFastq's per-entry text (ngs-bits_amd/csrc/tofastq_visit.h: what the GPU library compiles into fq_keys_kernel and fq_format_kernel) on the CPU:
// tests/test_cpu_tofastq_designed.py runs it over designed records (tests/tofastq_cases.py) against the Python restatement. Test infrastructure, never linked
// into the library.
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>
#define NGSQC_REC_ON_CPU
#include "device_on_cpu.h"
static inline unsigned long long atomicAdd(unsigned long long* p, unsigned long long v) { const unsigned long long o = *p; *p += v; return o; }
namespace ngsqc { using std::max; using std::min; }
#include "tofastq_visit.h"

using namespace ngsqc;

namespace {
constexpr uint8_t POISON = 0xA5;

// the entry as a wave writes its part inside the window [lo, hi) of the buffer at base (64 lanes, one after the other)
void format_wave(const uint8_t* rec, uint32_t size, int32_t extend, int64_t pos, int64_t lo, int64_t hi, uint8_t* base)
{
	const FqSplit sp = fq_split(pos, (int64_t)size, lo, hi);
	if (sp.a >= sp.b) return;
	for (int lane = 0; lane < 64; ++lane) fq_format_lane(fq_entry(rec, size, extend), pos, sp, lane, base);
}

// buf[from, from + n) holds expect[0, n) and every other byte of buf is still POISON: -1, else the first offending offset
int64_t only(const std::vector<uint32_t>& words, size_t bytes, int64_t from, int64_t n, const uint8_t* expect)
{
	const uint8_t* buf = reinterpret_cast<const uint8_t*>(words.data());
	for (int64_t x = 0; x < (int64_t)bytes; ++x)
	{
		const uint8_t want = x >= from && x < from + n ? expect[x - from] : POISON;
		if (buf[x] != want) return x;
	}
	return -1;
}
}

extern "C" {

// per record i at infl + recoff[i]: the info word (size | kept | throws), the region verdict and bam_endpos
void tofastq_info(const uint8_t* infl, const int64_t* recoff, int64_t n, int32_t extend, int32_t reg_tid, int32_t reg_start, int32_t reg_end, uint32_t* info, uint8_t* in_region, int64_t* endpos)
{
	for (int64_t i = 0; i < n; ++i)
	{
		const RecView r = load_rec(infl, recoff[i]);
		info[i] = fq_entry_info(r, extend, name_len(r.core + 32, r.l_name));
		in_region[i] = fq_in_region(r, reg_tid, reg_start, reg_end) ? 1 : 0;
		endpos[i] = rec_endpos(r);
	}
}

// the entry of `size` bytes, byte by byte
void tofastq_entry(const uint8_t* rec, uint32_t size, int32_t extend, uint8_t* out)
{
	const FqEntry e = fq_entry(rec, size, extend);
	for (uint32_t k = 0; k < size; ++k) out[k] = fq_byte(e, (int)k);
}

// The entry through the format kernel's range split, for each of the four alignments of its start and every cut c of its range (an entry longer than `dense`
// bytes: the cuts within `dense` bytes of either end and every 251st between): the window that ends c bytes behind the entry's start, the next window,
// which begins there at 0, and a window that ends c bytes in front of the entry's end. Each launch must write its part of `expect` and leave every other
// byte of the buffer alone.
// Returns -1, or (launch << 60 | alignment << 56 | c << 24 | offending offset).
int64_t tofastq_splits(const uint8_t* rec, uint32_t size, int32_t extend, const uint8_t* expect, int32_t dense)
{
	const size_t bytes = ((size_t)size + 8 + 8 + 3) & ~(size_t)3;
	std::vector<uint32_t> words(bytes / 4);
	uint8_t* buf = reinterpret_cast<uint8_t*>(words.data());
	for (int64_t al = 0; al < 4; ++al)
		for (int64_t c = 0; c <= (int64_t)size; c += (c < dense || c + dense >= (int64_t)size) ? 1 : std::min<int64_t>(251, (int64_t)size - dense - c))
		{
			const int64_t P = 4 + al;
			memset(buf, POISON, bytes);
			format_wave(rec, size, extend, P, 0, P + c, buf);
			int64_t bad = only(words, bytes, P, c, expect);
			if (bad >= 0) return (int64_t)0 << 60 | al << 56 | c << 24 | bad;
			memset(buf, POISON, bytes);
			format_wave(rec, size, extend, -c, 0, (int64_t)bytes, buf);
			bad = only(words, bytes, 0, (int64_t)size - c, expect + c);
			if (bad >= 0) return (int64_t)1 << 60 | al << 56 | c << 24 | bad;
			// a window that begins with the entry and ends c bytes in front of its end
			memset(buf, POISON, bytes);
			format_wave(rec, size, extend, P, P, P + (int64_t)size - c, buf);
			bad = only(words, bytes, P, (int64_t)size - c, expect);
			if (bad >= 0) return (int64_t)2 << 60 | al << 56 | c << 24 | bad;
		}
	return -1;
}
}
