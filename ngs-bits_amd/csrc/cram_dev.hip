// CRAM on the device, first codec: the QUALITY arrays. A CRAM slice stores the qualities of its records in one external block (series QS), rANS 4x8 coded
// (CRAMv3 section 13; order 1 in htslib's files) - about half of the bytes of the BAM records the slice decodes to. The host (cram.hip) builds every record with
// its quality bytes left blank and a plan: per block the position of its four rANS states in the CRAM image and its frequency tables in a compact form (the
// symbols that occur - at most 64 - and per context the cumulative frequencies), per record where its qualities go. Here: one lane per block decodes it
// (four interleaved states over one byte stream: sequential by construction; a file has one block per slice, i.e. thousands), then one lane per record copies
// its qualities into the BAM image that K1 reads (stored BGZF members: the payload of member m starts at m * 65311 + 23). The kernels: cram_dev_kernels.h.
#include "common.h"
#include "wave.h"
#include "cram_dev_kernels.h"
#include <cstring>

namespace ngsqc {
namespace {
template <typename T> T* dev_copy(const T* host, size_t n, hipStream_t s)
{
	T* d = nullptr; HIPCHK(hipMalloc((void**)&d, std::max<size_t>(n, 1) * sizeof(T)));
	if (n) HIPCHK(hipMemcpyAsync(d, host, n * sizeof(T), hipMemcpyHostToDevice, s));
	return d;
}
} // namespace

double cram_device_quals(const uint8_t* cram_image, const CramQualPlan& plan, uint8_t* d_image, size_t image_bytes, hipStream_t s)
{
	if (plan.jobs.empty()) return 0.0;
	// the blocks' byte streams, packed one behind the other (the only part of the CRAM file the device sees)
	std::vector<CramQualPlan::Job> jobs = plan.jobs; std::vector<uint8_t> in; size_t total = 0;
	for (const auto& j : jobs) total += j.in_len;
	in.reserve(total);
	for (auto& j : jobs) { const uint64_t at = in.size(); in.insert(in.end(), cram_image + j.in_off, cram_image + j.in_off + j.in_len); j.in_off = at; }
	uint8_t* d_in = dev_copy(in.data(), in.size(), s); CramQualPlan::Job* d_jobs = dev_copy(jobs.data(), jobs.size(), s);
	uint16_t* d_tabs = dev_copy(plan.tabs.data(), plan.tabs.size(), s); uint8_t* d_syms = dev_copy(plan.syms.data(), plan.syms.size(), s);
	CramQualPlan::Patch* d_patch = dev_copy(plan.patches.data(), plan.patches.size(), s);
	uint8_t* d_out = nullptr; HIPCHK(hipMalloc((void**)&d_out, std::max<uint64_t>(plan.out_bytes, 1)));
	unsigned int* d_status = nullptr; HIPCHK(hipMalloc((void**)&d_status, sizeof(unsigned int))); HIPCHK(hipMemsetAsync(d_status, 0, sizeof(unsigned int), s));
	hipEvent_t e0, e1; HIPCHK(hipEventCreate(&e0)); HIPCHK(hipEventCreate(&e1));
	HIPCHK(hipEventRecord(e0, s));
	hipLaunchKernelGGL(cramdev::cram_rans_lds_kernel, dim3((unsigned)jobs.size()), dim3(64), 0, s, d_in, d_jobs, (int)jobs.size(), d_tabs, d_syms, d_out, d_status);
	KCHECK();
	if (!plan.patches.empty())
	{
		hipLaunchKernelGGL(cramdev::cram_patch_kernel, dim3((unsigned)((plan.patches.size() + 255) / 256)), dim3(256), 0, s, d_patch, (int64_t)plan.patches.size(), d_out, (uint64_t)plan.out_bytes, d_image, (uint64_t)image_bytes, d_status); KCHECK();
	}
	HIPCHK(hipEventRecord(e1, s));
	unsigned int st = 0; HIPCHK(hipMemcpyAsync(&st, d_status, sizeof st, hipMemcpyDeviceToHost, s)); HIPCHK(hipStreamSynchronize(s));
	float ms = 0; HIPCHK(hipEventElapsedTime(&ms, e0, e1));
	(void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
	(void)hipFree(d_in); (void)hipFree(d_jobs); (void)hipFree(d_tabs); (void)hipFree(d_syms); (void)hipFree(d_patch); (void)hipFree(d_out); (void)hipFree(d_status);
	if (st) throw std::runtime_error("a quality block of the CRAM file does not decode on the device (rANS status " + std::to_string(st) + ")");
	return (double)ms;
}
} // namespace ngsqc
