// The bit tricks of baseq_tile_kernel (ngs-bits_amd/csrc/baseq_bits.h: the text the GPU library compiles into the kernel) on the CPU, against the obvious loops and
// exhaustively: tests/test_cpu_readdepth_model.py builds and runs this program. Exit status 0 and a line of counts when everything agrees, 1 and the first
// disagreement otherwise. Test infrastructure, never linked into the library.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include "device_on_cpu.h"
#include "../../ngs-bits_amd/csrc/baseq_bits.h"

using namespace ngsqc;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }   // xorshift64

// the kernel's sixteen steps over 64 qualities and the cut to the first `left` (scan.hip, baseq_tile_kernel)
static unsigned long long below64(const uint8_t* q, uint32_t thr, uint32_t left)
{
	uint32_t w[16]; memcpy(w, q, 64);
	unsigned long long mm = 0;
	for (int k = 0; k < 16; ++k)
	{
		const uint32_t lt = bq_below4(w[k], thr);
		mm |= (unsigned long long)lt << (4 * k);
	}
	return bq_keep_first(mm, left);
}

int main()
{
	long long n4 = 0, n64 = 0, nclip = 0;
	// (1) a dword of qualities: every value of a byte in every lane against every threshold the trick serves, the other three bytes drawn (and at their own edges)
	for (int min_baseq = 1; min_baseq <= 127; ++min_baseq)
	{
		const uint32_t thr = 0x01010101u * (uint32_t)(min_baseq & 127);
		for (int lane = 0; lane < 4; ++lane)
			for (int v = 0; v < 256; ++v)
				for (int rep = 0; rep < 8; ++rep)
				{
					uint8_t b[4];
					const uint64_t r = rnd();
					for (int k = 0; k < 4; ++k) b[k] = (uint8_t)(r >> (8 * k));
					if (rep == 1) for (int k = 0; k < 4; ++k) b[k] = 0;
					if (rep == 2) for (int k = 0; k < 4; ++k) b[k] = 0xff;
					if (rep == 3) for (int k = 0; k < 4; ++k) b[k] = (uint8_t)(min_baseq - 1);
					if (rep == 4) for (int k = 0; k < 4; ++k) b[k] = (uint8_t)min_baseq;
					if (rep == 5) for (int k = 0; k < 4; ++k) b[k] = (uint8_t)(0x80 | (min_baseq - 1));
					b[lane] = (uint8_t)v;
					uint32_t w; memcpy(&w, b, 4);
					uint32_t want = 0;
					for (int k = 0; k < 4; ++k) if ((int)b[k] < min_baseq) want |= 1u << k;
					const uint32_t got = bq_below4(w, thr);
					if (got != want) { printf("bq_below4: min_baseq %d, bytes %u %u %u %u: flags %x, expected %x\n", min_baseq, b[0], b[1], b[2], b[3], got, want); return 1; }
					++n4;
				}
	}
	// (2) 64 qualities, every left (0: nothing kept; the kernel asks for 1 and more), every threshold
	for (int min_baseq = 1; min_baseq <= 127; ++min_baseq)
	{
		const uint32_t thr = 0x01010101u * (uint32_t)(min_baseq & 127);
		for (uint32_t left = 0; left <= 64; ++left)
			for (int rep = 0; rep < 4; ++rep)
			{
				uint8_t q[64];
				for (int k = 0; k < 64; ++k)
				{
					const uint64_t r = rnd();
					q[k] = rep == 0 ? (uint8_t)r : rep == 1 ? (uint8_t)(min_baseq - 1 + (int)(r & 1)) : rep == 2 ? (uint8_t)((r & 1) ? 0xff : 0) : (uint8_t)(r % 42);
				}
				unsigned long long want = 0;
				for (uint32_t k = 0; k < 64 && k < left; ++k) if ((int)q[k] < min_baseq) want |= 1ull << k;
				const unsigned long long got = below64(q, thr, left);
				if (got != want) { printf("64 qualities: min_baseq %d, left %u, pattern %d: %016llx, expected %016llx\n", min_baseq, left, rep, got, want); return 1; }
				++n64;
			}
	}
	// (3) the flags of 256 read positions cut to [a_lo, b_hi): every pair, the words the kernel's loop visits (cw from a_lo >> 6 while 64 cw < b_hi) - each word
	// against the obvious loop, and the words together hold every flagged position of the range once and none outside it
	for (int rep = 0; rep < 3; ++rep)
	{
		unsigned long long low[4];
		for (int c = 0; c < 4; ++c) low[c] = rep == 0 ? ~0ull : rep == 1 ? rnd() : rnd() & rnd() & rnd();
		for (uint32_t a_lo = 0; a_lo <= 256; ++a_lo)
			for (uint32_t b_hi = a_lo; b_hi <= 256; ++b_hi)
			{
				uint8_t seen[256] = {0};
				for (uint32_t cw = a_lo >> 6; cw * 64u < b_hi; ++cw)
				{
					const unsigned long long m = bq_clip_word(low[cw], a_lo, b_hi, cw);
					unsigned long long want = 0;
					for (uint32_t bit = 0; bit < 64; ++bit) { const uint32_t x = 64u * cw + bit; if (x >= a_lo && x < b_hi && ((low[cw] >> bit) & 1ull)) want |= 1ull << bit; }
					if (m != want) { printf("bq_clip_word: [%u, %u) word %u of %016llx: %016llx, expected %016llx\n", a_lo, b_hi, cw, low[cw], m, want); return 1; }
					for (uint32_t bit = 0; bit < 64; ++bit) if ((m >> bit) & 1ull) seen[64u * cw + bit]++;
					++nclip;
				}
				for (uint32_t x = 0; x < 256; ++x)
				{
					const int want = x >= a_lo && x < b_hi && ((low[x >> 6] >> (x & 63u)) & 1ull);
					if (seen[x] != want) { printf("word loop: [%u, %u) position %u visited %d times, expected %d\n", a_lo, b_hi, x, seen[x], want); return 1; }
				}
			}
	}
	printf("ok dwords=%lld blocks=%lld words=%lld\n", n4, n64, nclip);
	return 0;
}
