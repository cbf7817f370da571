// Every environment switch of libngsqc_hip.so: this file holds all the getenv calls of csrc/ and nothing else. Host-only C++ (no HIP includes: tests/emul builds it
// with a plain g++). One line per switch: field = rule(name, default, range); kind | when unset | what it does. README.md lists the same names.
// The switches take effect at two moments, so there are two structs; MAKING one reads the environment (the default member initialisers below):
//   OpenSwitches  read once when ngsqc_open* makes the handle, on the caller's thread, before any background thread starts; never written again. The layout thread
//                 and the copier threads read only this one (getenv on their side against a caller's setenv would be a data race).
//   CallSwitches  read when the handle is made and again at the top of every entry point that works on a handle (guarded(), handle.h), on the caller's thread:
//                 what a job, a tile or a launch consults, so that one handle can run two jobs under two settings.
#pragma once
#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstdlib>
#include <string>

namespace ngsqc {

constexpr int SW_UNSET = INT_MIN;   // a switch without a fixed default (its user decides: by the file, by the mode) that is not set

inline bool env_flag_present(const char* name) { return getenv(name) != nullptr; }                                          // on when set to any value, "0" included
inline bool env_on_unless_zero(const char* name) { const char* e = getenv(name); return !(e && atoi(e) == 0); }
inline bool env_nonzero(const char* name, bool unset) { const char* e = getenv(name); return e ? atoi(e) != 0 : unset; }
inline int env_tristate(const char* name) { const char* e = getenv(name); return e ? (atoi(e) != 0 ? 1 : 0) : SW_UNSET; }
inline int64_t env_int_clamped(const char* name, int64_t unset, int64_t lo, int64_t hi) { const char* e = getenv(name); return e ? std::min(hi, std::max(lo, (int64_t)atoll(e))) : unset; }
inline int env_int_raw(const char* name, int unset) { const char* e = getenv(name); return e ? atoi(e) : unset; }
inline double env_double_min(const char* name, double unset, double lo) { const char* e = getenv(name); return e ? std::max(lo, atof(e)) : unset; }
inline int env_one_of(const char* name, int a, int b, int otherwise) { const int v = env_int_raw(name, otherwise); return v == a || v == b ? v : otherwise; }
inline std::string env_string(const char* name) { const char* e = getenv(name); return e ? e : ""; }
inline int walkers_shift(int64_t k) { return k >= 8 ? 3 : k >= 4 ? 2 : k >= 2 ? 1 : 0; }

struct OpenSwitches
{
	// ---- layout of the tile stream (plan_layout_now) ----
	int64_t tile_members        = env_int_clamped("NGSQC_TILE_MEMBERS", 0, 1, INT64_MAX);             // test hook | 0: sized by the device | K1 chunks and tiles of that many BGZF members (one chunk per tile)
	int64_t tile_chunks         = env_int_clamped("NGSQC_TILE_CHUNKS", 0, 1, INT64_MAX);              // product   | 0: 8, 1 for a streamed image | K1 chunks per tile (at most: what the HBM holds)
	int     token_slots         = (int)env_int_clamped("NGSQC_TOKEN_SLOTS", 8, 2, 8);                 // product   | 8 | slots of the token pool ring
	double  token_pool_factor   = env_double_min("NGSQC_TOKEN_POOL_FACTOR", 1.0, 0.01);               // test hook | 1.0 | scales the token pool (a small pool forces the second-chance path)
	int64_t carry_max           = env_int_clamped("NGSQC_CARRY_MAX", 64ll << 20, 0, INT64_MAX);       // product   | 64 MiB | bytes reserved in front of a tile for a record that straddles two tiles
	int     comp_slots          = (int)env_int_clamped("NGSQC_COMP_SLOTS", 0, 2, INT_MAX);            // product   | 0: min(8, chunks) | chunk slots of a streamed image's ring (at most one per chunk)
	// ---- the compressed image on its way to the device ----
	int     h2d_threads         = (int)env_int_clamped("NGSQC_H2D_THREADS", 4, 1, INT_MAX);           // product   | 4 | host threads that copy the pieces of a file opened by path
	int     h2d_piece_mb        = (int)env_int_clamped("NGSQC_H2D_PIECE_MB", 64, 1, INT_MAX);         // product   | 64 | size of such a piece
	int     h2d_delay_us        = (int)env_int_clamped("NGSQC_H2D_DELAY_US", 0, 0, INT_MAX);          // test hook | 0 | sleep before every piece (a slow link: the chunk stream really waits)
	int     walk_threads        = (int)env_int_clamped("NGSQC_WALK_THREADS", 8, 1, 64);               // product   | 8 | host threads that walk the BGZF member table in pieces
	int     stream_image        = env_tristate("NGSQC_STREAM_IMAGE");                                 // product   | by size | 1 / 0: a file opened by path is streamed through a ring of chunk slots / kept resident
	int64_t stream_image_min_mb = env_int_clamped("NGSQC_STREAM_IMAGE_MIN_MB", 4096, 0, INT_MAX);     // product   | 4096 | files of that size and more are streamed
	int64_t shard_tail_members  = env_int_clamped("NGSQC_SHARD_TAIL_MEMBERS", 64, 0, INT64_MAX);      // product   | 64 | members inflated behind a shard or a head request to complete its last record
	bool    async_h2d           = env_on_unless_zero("NGSQC_ASYNC_H2D");                              // product   | on | 0: ngsqc_open copies the image in the foreground
	bool    async_plan          = env_on_unless_zero("NGSQC_ASYNC_PLAN");                             // product   | on | 0: the tile stream's buffers are allocated by the first job, not by a thread of ngsqc_open
	bool    verify_crc          = env_nonzero("NGSQC_VERIFY_CRC", true);                              // product   | on | 0: the CRC32 of the inflated members is not checked
	int     p1_park             = env_int_raw("NGSQC_P1_PARK", 32);                                   // test hook | 32 | lanes that wait for the decoder's slow section before the wave enters it (& 255 at launch)
	// ---- CRAM input ----
	int     cram_threads        = (int)env_int_clamped("NGSQC_CRAM_THREADS", 0, 1, INT_MAX);          // product   | 0: the host's cores, at most 32 | host workers, one slice each
	bool    cram_device_quals   = env_on_unless_zero("NGSQC_CRAM_DEVICE_QUALS");                      // product   | on | 0: the quality arrays are decoded on the host
	bool    cram_ignore_md5     = env_nonzero("NGSQC_CRAM_IGNORE_MD5", false);                        // product   | off | 1: a slice's reference MD5 is not checked
	bool    cram_no_reference   = env_nonzero("NGSQC_CRAM_NO_REFERENCE", false);                      // test hook | off | 1: no genome is read, its bases become N
	std::string cram_plan_dump  = env_string("NGSQC_CRAM_PLAN_DUMP");                                 // test hook | none | ngsqc_cram_to_bam leaves the qualities blank and writes the device decoder's plan to this file
	std::string reference       = env_string("NGSQC_REFERENCE");                                      // product   | none | the genome when ngsqc_set_reference names none
	// ---- what ngsqc_open* itself and the threads it starts print ----
	bool    debug               = env_flag_present("NGSQC_DEBUG");                                    // profiling | off | stamps of open, the copy and the layout
	bool    timing              = env_flag_present("NGSQC_TIMING");                                   // profiling | off | where the time of a CRAM open goes
};

struct CallSwitches
{
	bool    pipeline            = env_on_unless_zero("NGSQC_PIPELINE");                               // profiling | on | 0: K1 of a tile starts when the previous tile is consumed (stage attribution)
	bool    k1_serial           = env_nonzero("NGSQC_K1_SERIAL", false);                              // profiling | off | 1: every K1 kernel in line on one stream (isolated per-kernel counters)
	bool    no_fused_scan       = env_flag_present("NGSQC_NO_FUSED_SCAN");                            // test hook | off | K2 and the scan as two kernels
	bool    no_fused_pileup     = env_flag_present("NGSQC_NO_FUSED_PILEUP");                          // test hook | off | the site pileup reads every record instead of the riding scan's candidates
	bool    k2_general          = env_flag_present("NGSQC_K2_GENERAL");                               // test hook | off | the host-verified chain for every tile
	bool    eager_recoff        = env_flag_present("NGSQC_EAGER_RECOFF");                             // test hook | off | record offsets of every tile expanded, asked for or not
	bool    baseq_ride          = env_on_unless_zero("NGSQC_BASEQ_RIDE");                             // product   | on | 0: a depth scan with min_baseq runs behind K2, a thread per record, instead of riding the walk
	int64_t bq_list_cap         = env_int_clamped("NGSQC_BQ_LIST_CAP", 0, 1, INT64_MAX);              // test hook | 0: the list's own size | bounds the riding walk's list of min_baseq records (a list that overflows)
	int     walker_shift        = walkers_shift(env_int_raw("NGSQC_WALKERS", 1));                     // product   | 0 | log2 of the walkers per BGZF member on K2's fast path (NGSQC_WALKERS = 1 / 2 / 4 / 8)
	int     group_shift         = (int)env_int_clamped("NGSQC_GROUP_SHIFT", SW_UNSET, 0, 8);          // product   | unset: 4 | long-read mode: 2^shift members per walker
	int     walk_waves          = env_int_raw("NGSQC_WALK_WAVES", SW_UNSET);                          // profiling | unset: 5 for the coverage tools' walk, 3 otherwise | waves per SIMD the fused walk is compiled for (5 / 4 / 3)
	int     long_read_mode      = env_tristate("NGSQC_LONG_READ_MODE");                               // test hook | by the file's first records | 1 / 0: always / never the long-read form of K2
	int     crc_chains          = env_one_of("NGSQC_CRC_CHAINS", 1, 2, 4);                            // profiling | 4 | chains per lane of the CRC kernel (1 / 2 / 4)
	int     name_hash_bits      = (int)env_int_clamped("NGSQC_NAME_HASH_BITS", 63, 1, 63);            // test hook | 63 | the mate join's read-name hash cut to that many bits (collisions everywhere)
	int64_t write_window_pieces = env_int_clamped("NGSQC_WRITE_WINDOW_PIECES", 16384, 1, INT64_MAX);  // test hook | 16384, about 1 GiB | the BAM and FASTQ writers' window in pieces of 0xff00 bytes
	bool    debug               = env_flag_present("NGSQC_DEBUG");                                    // profiling | off | stamps of every job and tile
	bool    timing              = env_flag_present("NGSQC_TIMING");                                   // profiling | off | stage times of the writers (BamFilter, BamToFastq)
};

} // namespace ngsqc
