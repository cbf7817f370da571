// The device keywords of the csrc headers, defined away for g++: the one place that says "this text is being compiled for the CPU".
// Include it after the standard headers (libstdc++ spells attributes with some of these words) and before the csrc header under test.
// The macros csrc itself tests (NGSQC_REC_ON_CPU, NGSQC_K2_GUESS_ON_CPU, __HIPCC__) stay with the source that needs them.
#pragma once
#ifndef __device__
#define __device__
#endif
#ifndef __forceinline__
#define __forceinline__ inline
#endif
#ifndef __noinline__
#define __noinline__
#endif
#ifndef __restrict__
#define __restrict__
#endif
#ifndef __constant__
#define __constant__ static const
#endif
