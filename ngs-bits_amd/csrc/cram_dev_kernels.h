// CRAM on the device, the kernels (cram_dev.hip holds the launch, copy and status code): rANS 4x8 decode of the quality blocks and the copy of every record's
// qualities into the BAM image.
//
// Written against the wave vocabulary of wave.h only, so that the same text runs under the wave emulator of the test suite (tests/emul/cram_emul.cpp,
// tests/test_cram_dev_emul.py: every job against a sequential decoder of the same plan, with guards around the input and the output).
#pragma once
#include "cram_plan.h"

namespace ngsqc { namespace cramdev {

// One WORKGROUP per block, the job's tables in LDS (a search step is an LDS read, not a dependent global load). The four rANS states live in four lanes - every round
// each lane decodes the symbol of its state,
// the lanes count the bytes their renormalisation takes (0, 1 or 2), a prefix over the four lanes gives each its place in the shared byte stream (the order the
// sequential decoder reads them in: state 0 first), and the stream pointer moves on by the sum. Order 1 writes four quarters of the output, one per lane; what is left
// behind the quarters belongs to state 3 alone.
// The symbol of a state by bisection over the cumulative row (6 LDS reads for 64 symbols). (Round 4 went through four versions - one lane per block with the
// tables in global memory, one lane with the tables in LDS, four lanes with a scan from the front: 800 -> 480 -> 150 -> 38 ms for the test twin's largest block,
// profiles/r04_cram_device_quals.txt; only the last one is kept.)
K1_KERNEL(64) void cram_rans_lds_kernel(const uint8_t* __restrict__ in, const CramQualPlan::Job* __restrict__ jobs, int n_jobs, const uint16_t* __restrict__ tabs,
                                        const uint8_t* __restrict__ syms, uint8_t* __restrict__ out, unsigned int* __restrict__ status)
{
	K1_SHARED uint16_t sC[65 * 64]; K1_SHARED uint8_t sSym[64]; K1_SHARED int sK0;
	const int j = (int)wv::block_id(), lane = wv::lane();
	if (j >= n_jobs) return;
	const CramQualPlan::Job jb = jobs[j];
	const int ns = (int)jb.nsym, row = ns + 1, rows = jb.order ? ns : 1;
	if (jb.in_len < 16 || ns < 1 || ns > 64) { if (lane == 0) wv::atomic_or_u32(status, CRAM_ST_JOB); return; }
	for (int x = lane; x < rows * row; x += 64) sC[x] = tabs[jb.tab_off + x];
	if (lane < ns) sSym[lane] = syms[jb.sym_off + lane];
	if (lane == 0) sK0 = syms[jb.sym_off + 64];   // the row of context 0
	wv::wg_barrier();
	if (lane >= 4) return;
	const uint8_t* p = in + jb.in_off; const uint8_t* const end = p + jb.in_len;
	uint8_t* const o = out + jb.out_off; const uint32_t n = jb.n_out;
	bool bad = false;
	auto sym_of = [&](uint32_t x, const uint16_t* C, uint32_t& v) -> int {   // the symbol index of state x in row C; v: the state behind it, before renormalisation
		const uint32_t m = x & 0xfffu; int k = 0;
		// the LAST k with C[k] <= m: behind it C[k + 1] > m, so that symbol has a frequency (symbols without one repeat the value of their successor)
		int hi = ns;
		while (hi - k > 1) { const int mid = (k + hi) >> 1; if ((uint32_t)C[mid] <= m) k = mid; else hi = mid; }
		const uint32_t c0 = C[k], f = (uint32_t)C[k + 1] - c0;
		if (f == 0 || m < c0 || m >= (uint32_t)C[k + 1]) { bad = true; v = x; return 0; }
		v = f * (x >> 12) + m - c0;
		return k;
	};
	{
		uint32_t x = (uint32_t)p[4 * lane] | ((uint32_t)p[4 * lane + 1] << 8) | ((uint32_t)p[4 * lane + 2] << 16) | ((uint32_t)p[4 * lane + 3] << 24);
		p += 16;   // (every lane tracks the shared stream pointer)
		// a state below the renormalisation bound is no rANS state (every coder leaves its states in [2^23, 2^31)); it is refused here, because the rounds below
		// give a state at most three bytes where a sequential decoder reads until the bound is reached: from a state >= 2^23 two always do
		if (x < (1u << 23)) bad = true;
		// one round: the lane's symbol (when it has one), then the renormalisation bytes in the order of the states
		auto round = [&](bool active, const uint16_t* C) -> int {
			uint32_t v = x; int s = 0, cnt = 0;
			if (active) { s = sym_of(x, C, v); uint32_t t = v; while (t < (1u << 23) && cnt < 3) { t <<= 8; ++cnt; } }
			const int c0 = (int)wv::shfl((uint32_t)cnt, 0), c1 = (int)wv::shfl((uint32_t)cnt, 1), c2 = (int)wv::shfl((uint32_t)cnt, 2), c3 = (int)wv::shfl((uint32_t)cnt, 3);
			const int my = lane == 0 ? 0 : lane == 1 ? c0 : lane == 2 ? c0 + c1 : c0 + c1 + c2;
			if (p + c0 + c1 + c2 + c3 > end) bad = true;
			else for (int b = 0; b < cnt; ++b) v = (v << 8) | p[my + b];
			p += c0 + c1 + c2 + c3;
			if (active) x = v;
			return s;
		};
		if (jb.order == 0)
		{
			for (uint32_t i = 0; i < n; i += 4)
			{
				const bool act = i + (uint32_t)lane < n;
				const int s = round(act, sC);
				if (act && !bad) o[i + (uint32_t)lane] = sSym[s];
				if (wv::ballot(bad) != 0) break;
			}
		}
		else
		{
			const uint32_t q = n >> 2; uint32_t idx = (uint32_t)lane * q; int pk = sK0;
			if (pk >= ns) bad = true;
			for (uint32_t i = 0; i < q; ++i)
			{
				const int s = round(!bad, sC + pk * row);
				if (!bad) { o[idx++] = sSym[s]; pk = s; }
				if (wv::ballot(bad) != 0) break;
			}
			if (lane == 3 && !bad)   // what the quarters leave over: state 3 alone, bytes one after the other
				while (idx < n)
				{
					uint32_t v; const int s = sym_of(x, sC + pk * row, v);
					while (v < (1u << 23)) { if (p >= end) { bad = true; break; } v = (v << 8) | *p++; }
					if (bad) break;
					x = v; o[idx++] = sSym[s]; pk = s;
				}
		}
	}
	if (bad) wv::atomic_or_u32(status, CRAM_ST_STREAM);
}

// one lane per record: its qualities into the stored-BGZF image (the payload of member m starts at m * 65311 + 23)
K1_KERNEL(256) void cram_patch_kernel(const CramQualPlan::Patch* __restrict__ P, int64_t n, const uint8_t* __restrict__ qs, uint64_t qs_bytes, uint8_t* __restrict__ image, uint64_t image_bytes,
                                      unsigned int* __restrict__ status)
{
	const int64_t i = wv::block_id() * wv::block_dim() + wv::thread_id();
	if (i >= n) return;
	const CramQualPlan::Patch p = P[i];
	if (p.src + p.len > qs_bytes) { wv::atomic_or_u32(status, CRAM_ST_SRC); return; }
	for (uint32_t b = 0; b < p.len; ++b)
	{
		const uint64_t s = p.dst + b, at = (s / 65280ull) * 65311ull + 23ull + (s % 65280ull);
		if (at >= image_bytes) { wv::atomic_or_u32(status, CRAM_ST_DST); return; }
		image[at] = qs[p.src + b];
	}
}

} } // namespace ngsqc::cramdev
