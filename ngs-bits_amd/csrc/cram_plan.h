// The plan of the CRAM quality blocks that the device decodes (cram.hip writes it, cram_dev.hip / cram_dev_kernels.h read it): plain data, shared with the
// wave-emulation test harness (tests/emul), therefore free of HIP includes.
#pragma once
#include <cstdint>
#include <vector>

namespace ngsqc {

// The quality arrays of a CRAM (QS series: one rANS 4x8 block per slice, about half of a BAM record's bytes) can stay compressed on the host: the plan names every such
// block (where its four rANS states start in the CRAM image, its frequency tables in a compact form) and, per record, where its qualities go in the BAM stream; the
// device decodes the blocks and writes the qualities into the uploaded image (cram_dev.hip).
struct CramQualPlan
{
	struct Job { uint64_t in_off; uint64_t out_off; uint32_t in_len, n_out, tab_off, sym_off; uint32_t order, nsym; };   // in_off: the states + byte stream in the CRAM image; out_off: into the decoded quality bytes of all jobs
	struct Patch { uint64_t dst, src; uint32_t len, pad; };                                                       // dst: offset in the BAM stream; src: offset in the decoded quality bytes
	std::vector<Job> jobs; std::vector<uint16_t> tabs; std::vector<uint8_t> syms; std::vector<Patch> patches; uint64_t out_bytes = 0;
	// tabs: per job (order 0: one row; order 1: nsym rows, row = index of the previous symbol) of nsym + 1 cumulative frequencies; syms: per job 64 symbols + 256 bytes "byte -> index"
};

// status bits of the two kernels (any bit set: the handle is refused)
enum { CRAM_ST_JOB = 1u,      // a job the kernel does not take: fewer than 16 bytes of states, no symbol or more than 64
       CRAM_ST_STREAM = 2u,   // a block that does not decode: a start state below 2^23, a state outside every symbol's range, a context without a table, a byte stream that ends early
       CRAM_ST_SRC = 4u,      // a record's qualities lie behind the decoded bytes
       CRAM_ST_DST = 8u };    // a record's qualities lie behind the BAM image

} // namespace ngsqc
