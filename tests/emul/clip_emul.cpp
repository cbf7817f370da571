// BamClipOverlap's visit of a read pair and the bytes of its two records (ngs-bits_amd/csrc/clip_visit.h: the text the GPU library compiles into its plan and
// gather kernels) on the CPU: tests/test_cpu_bamclipoverlap_emul.py runs it over designed and random pairs against the literal Python restatement. Test
// infrastructure, never linked into the library.
#include <cstddef>
#include <cstdint>
#include <cstring>
#define NGSQC_REC_ON_CPU
#include "device_on_cpu.h"
#include "../../ngs-bits_amd/csrc/clip_visit.h"

using namespace ngsqc;
using namespace ngsqc::clip;

namespace {
struct BufSink
{
	uint8_t* base; long long cap;
	void operator()(long long at, uint8_t v) const { if (at >= 0 && at < cap) base[at] = v; }
	void fence() const {}
};
}

extern "C" {

// 1 when the record enters the name map, 0 when it is written through
int clip_emul_joins(const uint8_t* rec) { RecView r = load_rec(rec, 0); rec_apply_cg(r); return joins(r) ? 1 : 0; }

// The pair (opener, closer: two records in file order). plan: two rows of six (forward read, reverse read: role, bases clipped, pos, n_cigar, tlen, verdict
// bits); info: soft_clip, forward is the opener, overlap; err: code and its two integers. out: the two records as the gather writes them, forward first
// (n_out[0], n_out[1] bytes; 0 / 0 for a removed pair); returns 1 when out holds them, 0 when the pair leaves as it came (not soft-clipped) or has an error.
int clip_emul_pair(const uint8_t* opener, const uint8_t* closer, int mode, int ignore_indels, int parity, int32_t* plan, int32_t* info, int32_t* err, uint8_t* out, long long cap, int64_t* n_out)
{
	PairOut o; uint32_t sf = 0, sr = 0;
	const bool wrote = write_pair(opener, closer, mode, ignore_indels != 0, parity, 0, BufSink{out, cap}, 0, 1, o, sf, sr);
	const MateOut* m[2] = {&o.f, &o.r};
	for (int k = 0; k < 2; ++k)
	{
		int32_t* p = plan + 6 * k;
		p[0] = k ? ROLE_REVERSE : ROLE_FORWARD; p[1] = m[k]->clip; p[2] = m[k]->pos; p[3] = m[k]->n_cigar; p[4] = m[k]->tlen; p[5] = m[k]->bits;
	}
	info[0] = o.soft_clip; info[1] = o.fwd_is_opener; info[2] = o.overlap;
	err[0] = o.err; err[1] = o.ea; err[2] = o.eb;
	n_out[0] = sf; n_out[1] = sr;
	return wrote ? 1 : 0;
}

// softClipAlignment on its own: the new CIGAR words (up to cap), their number in *n, the new pos; returns the error code
int clip_emul_soft_clip(const uint8_t* rec, int start_ref, int end_ref, uint32_t* words, int cap, int* n, int* new_pos)
{
	RecView r = load_rec(rec, 0); rec_apply_cg(r);
	int rlen = 0, ea = 0;
	*n = 0; *new_pos = r.pos;
	return soft_clip(r, start_ref, end_ref, [&](int k, uint32_t w) { if (k < cap) words[k] = w; }, *new_pos, *n, rlen, ea);
}
}
