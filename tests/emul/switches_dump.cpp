// Prints what ngs-bits_amd/csrc/switches.h makes of the environment, one "struct.field=value" line per switch (SW_UNSET prints as "unset"):
// tests/test_cpu_switches.py runs it as a child process under one environment per rule. Test infrastructure, never linked into the library.
#include "../../ngs-bits_amd/csrc/switches.h"
#include <cstdio>

using namespace ngsqc;

static void put(const char* k, long long v) { if (v == SW_UNSET) printf("%s=unset\n", k); else printf("%s=%lld\n", k, v); }
static void put(const char* k, double v) { printf("%s=%g\n", k, v); }
static void put(const char* k, const std::string& v) { printf("%s=%s\n", k, v.c_str()); }
#define PUT(s, f) put(#s "." #f, s.f)
#define PUTI(s, f) put(#s "." #f, (long long)s.f)

int main()
{
	const OpenSwitches open; const CallSwitches call;
	PUTI(open, tile_members); PUTI(open, tile_chunks); PUTI(open, token_slots); PUT(open, token_pool_factor); PUTI(open, carry_max); PUTI(open, comp_slots);
	PUTI(open, h2d_threads); PUTI(open, h2d_piece_mb); PUTI(open, h2d_delay_us); PUTI(open, walk_threads); PUTI(open, stream_image); PUTI(open, stream_image_min_mb);
	PUTI(open, shard_tail_members); PUTI(open, async_h2d); PUTI(open, async_plan); PUTI(open, verify_crc); PUTI(open, p1_park);
	PUTI(open, cram_threads); PUTI(open, cram_device_quals); PUTI(open, cram_ignore_md5); PUTI(open, cram_no_reference); PUT(open, cram_plan_dump); PUT(open, reference);
	PUTI(open, debug); PUTI(open, timing);
	PUTI(call, pipeline); PUTI(call, k1_serial); PUTI(call, no_fused_scan); PUTI(call, no_fused_pileup); PUTI(call, k2_general); PUTI(call, eager_recoff);
	PUTI(call, baseq_ride); PUTI(call, bq_list_cap); PUTI(call, walker_shift); PUTI(call, group_shift); PUTI(call, walk_waves); PUTI(call, long_read_mode);
	PUTI(call, crc_chains); PUTI(call, name_hash_bits); PUTI(call, write_window_pieces); PUTI(call, debug); PUTI(call, timing);
	return 0;
}
