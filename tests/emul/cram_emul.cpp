// Runs the two CRAM quality kernels (ngs-bits_amd/csrc/cram_dev_kernels.h, the text the GPU library compiles) under the wave emulator on the CPU:
// tests/test_cram_dev_emul.py compares the result with a sequential decoder of the same plan. Test infrastructure - see wave_emul.h.
//
// Every job runs twice, on private copies of its input and output between two inaccessible pages: once with the END of the byte stream and of the output range
// against the page behind them, once with their START against the page in front. The other side of each range carries GUARD bytes that are compared afterwards.
// A read or a write that reaches a page ends the workgroup and is reported; so is a guard byte that changed, and a run whose two placements disagree.
#include "wave_emul.h"
#include "../../ngs-bits_amd/csrc/cram_dev_kernels.h"
#include <signal.h>
#include <sys/mman.h>
#include <unistd.h>
#include <algorithm>

using namespace ngsqc;

namespace {
constexpr size_t GUARD = 256;
constexpr uint8_t FILL = 0xa5;
volatile sig_atomic_t g_fault = 0;

void on_segv(int)
{
	// a lane touched an inaccessible page: the workgroup ends here (the fault is synchronous, the handler runs on the lane's own stack)
	wv::Emu& E = wv::emu(); g_fault = 1;
	for (int l = 0; l < wv::Emu::W; ++l) E.live[l] = false;
	setcontext(&E.main_ctx);
}

// a range of `bytes` accessible bytes between two inaccessible pages
struct Arena
{
	uint8_t* base = nullptr; size_t page = 0, span = 0;
	explicit Arena(size_t bytes)
	{
		page = (size_t)sysconf(_SC_PAGESIZE); span = (bytes + page - 1) / page * page + page;   // (one page more than needed: room for the guard bytes)
		base = (uint8_t*)mmap(nullptr, span + 2 * page, PROT_NONE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
		if (base == MAP_FAILED) { base = nullptr; return; }
		mprotect(base + page, span, PROT_READ | PROT_WRITE);
	}
	~Arena() { if (base) munmap(base, span + 2 * page); }
	uint8_t* lo() const { return base + page; }          // the first accessible byte
	uint8_t* hi() const { return base + page + span; }   // the first inaccessible byte behind
	// n bytes placed at the end (back) or at the start, FILL everywhere else
	uint8_t* place(size_t n, bool back) const { memset(lo(), FILL, span); return back ? hi() - n : lo(); }
	bool guards_intact(const uint8_t* at, size_t n) const
	{
		for (const uint8_t* q = lo(); q < at; ++q) if (*q != FILL) return false;
		for (const uint8_t* q = at + n; q < hi(); ++q) if (*q != FILL) return false;
		return true;
	}
};
} // namespace

extern "C" {

// result bits (besides the kernels' own status word)
enum { EMU_PAGE_FAULT = 1, EMU_GUARD_WRITTEN = 2, EMU_PLACEMENTS_DIFFER = 4, EMU_NO_MEMORY = 8 };

// plan: jobs / tabs / syms / patches / out_bytes as NGSQC_CRAM_PLAN_DUMP writes them; cram: the CRAM file; stream: the BAM STREAM with blank qualities (what the stored
// members of the image carry). Out: qs (out_bytes: the decoded quality bytes), job_status (per job: the kernel's status word for that workgroup alone),
// job_emu (per job: EMU_* bits), the stream patched in place (the kernel addresses the stored-BGZF IMAGE: it is laid out here and taken apart again),
// patch_status / patch_emu for the second kernel. image_slack: bytes the image is cut short by (damaged plans).
int cram_emul_run(const CramQualPlan::Job* jobs, int64_t n_jobs, const uint16_t* tabs, int64_t n_tabs, const uint8_t* syms, int64_t n_syms,
                  const CramQualPlan::Patch* patches, int64_t n_patches, uint64_t out_bytes, const uint8_t* cram, uint64_t cram_bytes,
                  uint8_t* stream, uint64_t stream_bytes, uint8_t* qs, uint32_t* job_status, uint32_t* job_emu, uint32_t* patch_status, uint32_t* patch_emu)
{
	struct sigaction sa, old_segv, old_bus; memset(&sa, 0, sizeof sa); sa.sa_handler = on_segv; sigemptyset(&sa.sa_mask); sa.sa_flags = SA_NODEFER;
	sigaction(SIGSEGV, &sa, &old_segv); sigaction(SIGBUS, &sa, &old_bus);
	int rc = 0;
	if (n_jobs > 0) memset(qs, 0, (size_t)out_bytes);   // (a plan without jobs: the caller's quality bytes go to the second kernel as they are)
	// the tables as the device gets them: exactly n_tabs / n_syms elements, the end against an inaccessible page (a row read behind the plan's tables faults)
	Arena at((size_t)n_tabs * 2 + 2), as((size_t)n_syms + 1);
	if (!at.base || !as.base) rc = EMU_NO_MEMORY;
	uint16_t* d_tabs = nullptr; uint8_t* d_syms = nullptr;
	if (!rc)
	{
		d_tabs = (uint16_t*)at.place((size_t)n_tabs * 2, true); if (n_tabs) memcpy(d_tabs, tabs, (size_t)n_tabs * 2);
		d_syms = as.place((size_t)n_syms, true); if (n_syms) memcpy(d_syms, syms, (size_t)n_syms);
	}
	for (int64_t j = 0; j < n_jobs && !rc; ++j)
	{
		const CramQualPlan::Job& jb = jobs[j]; job_status[j] = 0; job_emu[j] = 0;
		if (jb.in_off > cram_bytes || jb.in_len > cram_bytes - jb.in_off || jb.out_off > out_bytes || jb.n_out > out_bytes - jb.out_off) { job_emu[j] = EMU_NO_MEMORY; continue; }   // (the test hands in plans whose ranges lie inside its buffers)
		Arena ai(jb.in_len + GUARD), ao(jb.n_out + GUARD);
		if (!ai.base || !ao.base) { rc = EMU_NO_MEMORY; break; }
		std::vector<uint8_t> first((size_t)jb.n_out); uint32_t st_first = 0;
		for (int pass = 0; pass < 2; ++pass)
		{
			const bool back = pass == 0;
			uint8_t* in = ai.place(jb.in_len, back); memcpy(in, cram + jb.in_off, jb.in_len);
			uint8_t* out = ao.place(jb.n_out, back); memset(out, 0, jb.n_out);
			CramQualPlan::Job one = jb; one.in_off = 0; one.out_off = 0;
			unsigned int status = 0; g_fault = 0;
			wv::run_block(0, 1, [&] { cramdev::cram_rans_lds_kernel(in, &one, 1, d_tabs, d_syms, out, &status); });
			if (g_fault) job_emu[j] |= EMU_PAGE_FAULT;
			if (!ai.guards_intact(in, jb.in_len) || !ao.guards_intact(out, jb.n_out) || !at.guards_intact((uint8_t*)d_tabs, (size_t)n_tabs * 2) || !as.guards_intact(d_syms, (size_t)n_syms)) job_emu[j] |= EMU_GUARD_WRITTEN;
			if (memcmp(in, cram + jb.in_off, jb.in_len) != 0) job_emu[j] |= EMU_GUARD_WRITTEN;   // (the input is read only)
			if (pass == 0) { memcpy(first.data(), out, jb.n_out); st_first = status; }
			else if (status != st_first || (status == 0 && memcmp(first.data(), out, jb.n_out) != 0)) job_emu[j] |= EMU_PLACEMENTS_DIFFER;
			job_status[j] |= status;
		}
		memcpy(qs + jb.out_off, first.data(), jb.n_out);
	}
	// the second kernel: the image of stored members (payload of member m at m * 65311 + 23), its end and the end of qs against inaccessible pages
	*patch_status = 0; *patch_emu = 0;
	if (!rc && n_patches > 0)
	{
		const uint64_t members = (stream_bytes + 65279) / 65280, image_bytes = members ? (members - 1) * 65311 + 23 + (stream_bytes - (members - 1) * 65280) + 8 : 0;
		Arena im((size_t)image_bytes + GUARD), aq((size_t)out_bytes + GUARD), ap((size_t)n_patches * sizeof(CramQualPlan::Patch));
		if (!im.base || !aq.base || !ap.base) rc = EMU_NO_MEMORY;
		else
		{
			uint8_t* image = im.place((size_t)image_bytes, true); memset(image, 0xee, (size_t)image_bytes);   // (headers and trailers of the members: not the kernel's to touch)
			for (uint64_t s = 0; s < stream_bytes; s += 65280) memcpy(image + (s / 65280) * 65311 + 23, stream + s, (size_t)std::min<uint64_t>(65280, stream_bytes - s));
			uint8_t* d_qs = aq.place((size_t)out_bytes, true); memcpy(d_qs, qs, (size_t)out_bytes);
			CramQualPlan::Patch* d_p = (CramQualPlan::Patch*)ap.place((size_t)n_patches * sizeof(CramQualPlan::Patch), true); memcpy(d_p, patches, (size_t)n_patches * sizeof(CramQualPlan::Patch));
			unsigned int status = 0; g_fault = 0;
			const int64_t grid = (n_patches + wv::Emu::W - 1) / wv::Emu::W;
			for (int64_t b = 0; b < grid && !g_fault; ++b)
				wv::run_block(b, grid, [&] { cramdev::cram_patch_kernel(d_p, n_patches, d_qs, out_bytes, image, image_bytes, &status); });
			if (g_fault) *patch_emu |= EMU_PAGE_FAULT;
			if (!im.guards_intact(image, (size_t)image_bytes) || !aq.guards_intact(d_qs, (size_t)out_bytes) || memcmp(d_qs, qs, (size_t)out_bytes) != 0) *patch_emu |= EMU_GUARD_WRITTEN;
			for (uint64_t m = 0; m < members; ++m)   // the bytes between the payloads
			{
				const uint8_t* h = image + m * 65311; const uint64_t pay = std::min<uint64_t>(65280, stream_bytes - m * 65280);
				for (int k = 0; k < 23; ++k) if (h[k] != 0xee) *patch_emu |= EMU_GUARD_WRITTEN;
				for (int k = 0; k < 8; ++k) if (h[23 + pay + k] != 0xee) *patch_emu |= EMU_GUARD_WRITTEN;
			}
			for (uint64_t s = 0; s < stream_bytes; s += 65280) memcpy(stream + s, image + (s / 65280) * 65311 + 23, (size_t)std::min<uint64_t>(65280, stream_bytes - s));
			*patch_status = status;
		}
	}
	sigaction(SIGSEGV, &old_segv, nullptr); sigaction(SIGBUS, &old_bus, nullptr);
	return rc;
}

}
