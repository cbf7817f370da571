// The decision stream of downsample.hip (glibc's rand() behind srand(seed), one value per ordinal, kept when it lies below the threshold of the percentage) for
// the accumulators of other files: the generator, the host's jump to a chunk's start state and ds_keep_kernel stay in downsample.hip, this is the call that
// fills a device buffer with the keep bytes of a range of ordinals. The ranges of one stream never go backwards.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace ngsqc { namespace lib {
struct KeepStream;
// throws ArgError("Invalid percentage <%g>!") outside (0, 100)
KeepStream* keep_stream_open(const char* tool, uint32_t seed, double percentage);
// the keep bytes (1 = kept) of the ordinals [k0, k0 + m), m > 0, queued on s: -> the device address of the byte of ordinal k0, valid until the next run.
// The caller has waited for s since the last run.
const uint8_t* keep_stream_run(KeepStream* k, int64_t k0, int64_t m, hipStream_t s);
void keep_stream_close(KeepStream* k);
}} // namespace ngsqc::lib
