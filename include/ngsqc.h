/*
 * ngsqc.h — C ABI of the MI355X-native BAM mapping-QC / coverage engine (libngsqc_hip.so).
 *
 * Drop-in boundary for ONE hot path of imgag/ngs-bits: the per-read loop behind
 *   Statistics::mapping(bed,...)      src/cppNGS/Statistics.h:40   (Statistics.cpp:343-803)
 *   Statistics::mapping(bam,...)      src/cppNGS/Statistics.h:42   (Statistics.cpp:805-988)
 *   Statistics::mapping_wgs           src/cppNGS/Statistics.h:44   (Statistics.cpp:990-1359)
 *   Statistics::avgCoverage           src/cppNGS/Statistics.h:70   (Statistics.cpp:2698-2804)
 *   Statistics::lowCoverage/highCoverage  Statistics.h:66,68       (Statistics.cpp:2534-2657,2693-2696,2806-2809)
 *   Statistics::yxRatio               Statistics.cpp:2659-2691
 * and the reader underneath them, BamReader::getNextAlignment / setRegion (src/cppNGS/BamReader.h:386-398,
 * BamReader.cpp:734-768), i.e. what the reference gets from htslib's sam_read1 / sam_itr_next / bam_endpos.
 *
 * The reference has no FFI for this path; the seam is the static C++ API above. The host layer
 * (ngs-bits_amd/host, plain C++17) keeps those function names/arguments/errors and calls into this ABI.
 * Everything here is plain C: pointers + sizes, caller-owned output buffers, int return codes
 * (0 = ok, <0 = error; message via ngsqc_last_error). No torch / HIP types cross the boundary.
 *
 * Coordinates: regions are 1-based, closed [start,end] (the in-memory convention of BedLine, BedFile.cpp:157-159).
 * Chromosomes are addressed by BAM reference id (tid); name -> tid mapping is host logic.
 */
#ifndef NGSQC_H
#define NGSQC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ngsqc_handle ngsqc_handle;

/* ---- error codes ---- */
#define NGSQC_OK            0
#define NGSQC_E_IO         -1   /* "Could not open BAM/CRAM file ..."            BamReader.cpp:465-468 */
#define NGSQC_E_FORMAT     -2   /* not BGZF / not BAM / corrupt record           BamReader.h:389-392  */
#define NGSQC_E_ARG        -3   /* invalid argument (ArgumentException cases)    */
#define NGSQC_E_DEVICE     -4   /* HIP runtime error / no device / out of memory */
#define NGSQC_E_UNSUPPORTED -5  /* CRAM 3.1 codecs other than rANS Nx16            */

/* ---- lifecycle (replaces BamReader ctor/dtor, BamReader.cpp:462-523) ---- */
int  ngsqc_open(const char* bam_path, int device, ngsqc_handle** out);
/* Same, from a BAM image already in host memory (bytes are copied to HBM; caller keeps ownership). */
int  ngsqc_open_memory(const void* bam_bytes, size_t n_bytes, int device, ngsqc_handle** out);
void ngsqc_close(ngsqc_handle* h);
/* ngsqc_open copies the compressed image to the device in the background (pieces in file order; the first job starts on the pieces that have
 * arrived - what the reference overlaps with htslib's reader thread, BamReader.cpp:472). This call returns when the whole image is on the device;
 * ngsqc_timings.h2d_ms is final behind it. NGSQC_ASYNC_H2D=0: ngsqc_open itself waits (ngsqc_open_memory always does: the caller owns the buffer). */
int  ngsqc_upload_wait(ngsqc_handle* h);
/* Message of the last failing call on h (or of the last failing ngsqc_open* when h is NULL). */
const char* ngsqc_last_error(const ngsqc_handle* h);

/* ---- header access (BamReader::chromosomes/chromosomeSize, BamReader.cpp:770-800) ---- */
int         ngsqc_n_ref(const ngsqc_handle* h);
const char* ngsqc_ref_name(const ngsqc_handle* h, int tid);
int64_t     ngsqc_ref_len(const ngsqc_handle* h, int tid);
int64_t     ngsqc_n_records(ngsqc_handle* h);     /* forces inflate + record indexing */
int64_t     ngsqc_inflated_size(ngsqc_handle* h); /* bytes of the inflated BGZF stream */
int64_t     ngsqc_n_bgzf_blocks(const ngsqc_handle* h);
int64_t     ngsqc_compressed_size(const ngsqc_handle* h);

/* ---- stage control ----
 * Inflate (K1) and record indexing (K2) run lazily and their result stays in HBM for subsequent scans on the
 * same handle (the reference re-reads the file for every pass). ngsqc_drop_decoded() frees/invalidates that
 * state so that the next scan redoes the whole job from the compressed bytes (what bench.py times). */
int ngsqc_decode(ngsqc_handle* h);
int ngsqc_drop_decoded(ngsqc_handle* h);
/* test hooks: copy device results back (caller buffers) */
int ngsqc_copy_inflated(ngsqc_handle* h, uint8_t* out, int64_t cap);
int ngsqc_copy_record_offsets(ngsqc_handle* h, int64_t* out, int64_t cap);

/* ---- regions ---- */
typedef struct ngsqc_region { int32_t tid; int32_t start; int32_t end; } ngsqc_region; /* 1-based closed */

/* ---- mapping QC scan (Statistics::mapping x2, mapping_wgs) ---- */
#define NGSQC_MODE_ROI    0   /* Statistics.cpp:343  target-region mode                 */
#define NGSQC_MODE_NOROI  1   /* Statistics.cpp:805  -rna / -wgs -build non_human       */
#define NGSQC_MODE_WGS    2   /* Statistics.cpp:990  -wgs, optional OMIM ROI second pass */

/* counter vector indices (int64). Doubles of the reference that only ever hold integers are kept as int64. */
enum {
	NGSQC_C_AL_TOTAL = 0, NGSQC_C_AL_MAPPED, NGSQC_C_AL_ONTARGET, NGSQC_C_AL_NEARTARGET, NGSQC_C_AL_DUP,
	NGSQC_C_AL_PROPER_PAIRED, NGSQC_C_INSERT_SIZE_READ_COUNT, NGSQC_C_BASES_TRIMMED, NGSQC_C_BASES_MAPPED,
	NGSQC_C_BASES_CLIPPED, NGSQC_C_INSERT_SIZE_SUM, NGSQC_C_BASES_USABLE, NGSQC_C_BASES_USABLE_NO_OVERLAP,
	NGSQC_C_BASES_USABLE_RAW, NGSQC_C_BASES_USABLE_ROI, NGSQC_C_BASES_USABLE_DP0, /* ..DP4 = +4 */
	NGSQC_C_DP_DIST0 = 20, /* ..3 */
	NGSQC_C_MAX_LENGTH = 24, NGSQC_C_PAIRED_END, NGSQC_C_ROI_BASES, NGSQC_C_HALF_DEPTH, NGSQC_C_BASES_COVERED_HALF,
	NGSQC_C_READS_X, NGSQC_C_READS_Y, NGSQC_C_YX_VALID,
	NGSQC_C_INSERT_HIST0 = 32, /* 1000 bins: reads per integer insert size 0..999 (binned on host, Statistics.cpp:401) */
	NGSQC_NCOUNTERS = 1032
};

typedef struct ngsqc_mapping_params {
	int32_t mode;                 /* NGSQC_MODE_*                                                        */
	int32_t min_mapq;             /* Statistics.cpp:343 min_mapq                                          */
	int32_t tid_x, tid_y;         /* tids of chrX / chrY or -1 (yxRatio, Statistics.cpp:2662-2666)        */
	const uint8_t* tid_nonspecial;/* [n_ref] 1 if Chromosome::isNonSpecial (Chromosome.h:78-81)           */
	const ngsqc_region* regions;  /* merged + sorted target regions (NULL for NOROI / WGS without ROI)     */
	int64_t n_regions;
	const ngsqc_region* gc_chunks;/* roi.chunk(100) lines, same order (Statistics.cpp:366) or NULL        */
	const int32_t* gc_bin;        /* per chunk: GC bin 0..100 or -1                                       */
	int64_t n_gc_chunks;
} ngsqc_mapping_params;

/* Runs the scan. counters: int64[NGSQC_NCOUNTERS]. gc_reads: double[101] (may be NULL).
 * HALF_DEPTH / BASES_COVERED_HALF are left 0 here (they need avg depth): use ngsqc_depth_stats. */
int ngsqc_scan_mapping(ngsqc_handle* h, const ngsqc_mapping_params* p, int64_t* counters, double* gc_reads);

/* ---- plain depth scan (avgCoverage / lowOrHighCoverage filters) ---- */
typedef struct ngsqc_depth_params {
	int32_t min_mapq;
	int32_t min_baseq;        /* >0: per-base quality mask of BamAlignment::qualities (BamReader.cpp:210-255) */
	int32_t skip_mismapped;   /* WorkerAverageCoverage.cpp:44                                                 */
	int32_t reserved;
	const ngsqc_region* regions; /* merged + sorted */
	int64_t n_regions;
} ngsqc_depth_params;
int ngsqc_scan_depth(ngsqc_handle* h, const ngsqc_depth_params* p);

/* ---- BedReadCount (src/BedReadCount/main.cpp:33-71): number of reads overlapping each line of a merged + sorted BED. A read counts when it is
 * mapped, not secondary / supplementary and has MAPQ >= min_mapq (duplicates count); overlap is [start, bam_endpos] against the closed line. */
int ngsqc_region_read_counts(ngsqc_handle* h, const ngsqc_region* regions, int64_t n_regions, int32_t min_mapq, int64_t* counts);

/* ---- consumers of the per-base depth left in HBM by the last ngsqc_scan_mapping / ngsqc_scan_depth ---- */
/* hist[d] for d in 0..hist_cap (depths > cap are clamped into hist[cap]); covered = #bases with depth >= half_depth */
int ngsqc_depth_stats(ngsqc_handle* h, int32_t hist_cap, int64_t half_depth, int64_t* hist, int64_t* covered);
/* per-base depth, regions concatenated in order (roi_bases int32) */
int ngsqc_depth_copy(ngsqc_handle* h, int32_t* out, int64_t cap);
/* BedCoverage: sum of depth over each (possibly overlapping, unmerged) line; every line must lie inside the scanned regions */
int ngsqc_region_sums(ngsqc_handle* h, const ngsqc_region* lines, int64_t n_lines, int64_t* sums);
/* BedLow/HighCoverage: maximal runs inside each line with depth<cutoff (is_high=0) or depth>=cutoff (is_high=1).
 * saturate254 reproduces the sweep mode's uchar array (WorkerLowOrHighCoverage.cpp:199-203). Output runs are
 * (line index, start, end) triples in line order; returns number of runs via n_runs (call with cap=0 to size). */
typedef struct ngsqc_run { int64_t line; int32_t start; int32_t end; } ngsqc_run;
int ngsqc_lowhigh_runs(ngsqc_handle* h, const ngsqc_region* lines, int64_t n_lines, int32_t cutoff, int32_t is_high,
                       int32_t saturate254, ngsqc_run* runs, int64_t cap, int64_t* n_runs);

/* ---- site pileup: BamReader::getPileup (src/cppNGS/BamReader.cpp:809-885; SNP counts, indel_window = -1,
 * count_fragments = false) for a table of known sites, e.g. the common SNPs of Statistics::contamination
 * (Statistics.cpp:2333-2386). Sites: (tid, pos) with start == end == pos (1-based), sorted by tid then pos, each tid
 * contiguous. counts[8*i + 0..5] = A, C, G, T, N, deletion at site i after the reference's filters (not secondary /
 * supplementary / duplicate / unmapped, proper pair unless include_not_properly_paired, MAPQ >= min_mapq, base quality
 * >= min_baseq; a deleted base passes with quality 255); [6] = bases Pileup::inc throws on (IUPAC codes other than
 * ACGTN), [7] = reads whose CIGAR does not reach the site (the reference throws "Could not find position"). */
int ngsqc_site_pileup(ngsqc_handle* h, const ngsqc_region* sites, int64_t n_sites, int32_t min_mapq, int32_t min_baseq,
                      int32_t include_not_properly_paired, int64_t* counts);

/* ---- indel windows: BamReader::getIndels (src/cppNGS/BamReader.cpp:948-1125, count_fragments = false) for a table of windows, the indel half of
 * BamReader::getVariantDetails (:888-946). A window is [start, end] (1-based, closed) as getIndels receives it (indelRegion widened by one base on each side),
 * sorted by tid then start, each tid contiguous; windows may overlap. Its query allele: kind NGSQC_ALLELE_INS with the len inserted bases in allele,
 * NGSQC_ALLELE_DEL with the len deleted reference bases in allele and the reference slice [start, end + len) in ref_slice (end - start + len bytes, upper
 * case as FastaFileIndex::seq returns it, 0 behind the contig end), or NGSQC_ALLELE_NONE (n_match stays 0). counts[NGSQC_INDEL_NCOUNTERS * i + k]: */
#define NGSQC_ALLELE_NONE 0
#define NGSQC_ALLELE_INS  1
#define NGSQC_ALLELE_DEL  2
typedef struct ngsqc_indel_window {
	int32_t tid, start, end;
	int32_t kind, len;
	const char* allele;      /* len bases */
	const char* ref_slice;   /* NGSQC_ALLELE_DEL: end - start + len bases, else NULL */
} ngsqc_indel_window;
#define NGSQC_W_READS_MAPPED 0   /* reads overlapping the window that pass the filters (duplicate, proper pair unless include_npp, secondary / supplementary, unmapped) */
#define NGSQC_W_READS_MAPQ0  1   /* ... of which MAPQ 0 (not counted further) */
#define NGSQC_W_DEPTH        2   /* reads with start <= window.start and end >= window.end, minus one per N operation spanning the window */
#define NGSQC_W_INS          3   /* I operations of those reads at a genome position in [start, end], one per operation */
#define NGSQC_W_DEL          4   /* D operations ... */
#define NGSQC_W_MATCH        5   /* ... equal to the query allele: "+SEQ" / "-REF" (a deletion running past the reference's end, the length of the BAM
                                    header, is compared by the bases in front of the end, as FastaFileIndex::seq returns them) */
#define NGSQC_INDEL_NCOUNTERS 6
/* A read that the reference would walk (it spans the window and holds an I, D or N operation) and that holds an operation the reference throws on gives
 * NGSQC_E_FORMAT "Unknown CIGAR operation". */
int ngsqc_indel_windows(ngsqc_handle* h, const ngsqc_indel_window* windows, int64_t n_windows, int32_t include_not_properly_paired, int64_t* counts);
/* getVariantDetails for a VCF: the site pileup of the SNVs (sites and site_counts as in ngsqc_site_pileup, with site_min_mapq / site_min_baseq; the
 * reference asks getPileup for 1 / 13) and the indel windows in ONE decode of the file. count_fragments != 0: NGSQC_E_UNSUPPORTED. */
typedef struct ngsqc_variant_params {
	int32_t include_not_properly_paired;
	int32_t count_fragments;
	int32_t site_min_mapq, site_min_baseq;
} ngsqc_variant_params;
int ngsqc_variant_details(ngsqc_handle* h, const ngsqc_region* sites, int64_t n_sites, const ngsqc_indel_window* windows, int64_t n_windows,
                          const ngsqc_variant_params* p, int64_t* site_counts, int64_t* window_counts);

/* ---- raw-read QC pass: StatisticsReads::update(const BamAlignment&) (src/cppNGS/StatisticsReads.cpp:83-158), the loop
 * of `MappingQC -read_qc` (src/MappingQC/main.cpp:83-98). Secondary / supplementary records are skipped; single_end
 * counts every read as forward (otherwise read1 = forward). The reference throws on bases other than A/C/G/T/N and on
 * qualities >= 100: such records are counted in n_unknown_base / n_quality_out_of_range for the caller to throw. */
typedef struct ngsqc_read_stats {
	int64_t c_forward, c_reverse, bases_sequenced;
	int64_t bases[5];                                   /* A, C, G, T, N over all cycles (sum of the per-cycle pileups) */
	int64_t base_qualities[100];                        /* bases per quality value */
	int64_t read_qualities[100];                        /* reads per round(mean quality)  (StatisticsReads.cpp:151) */
	int64_t qscore_dist_r1[60], qscore_dist_r2[60];     /* Histogram(0,60,1) of the mean quality, forward / reverse reads (:152-153) */
	int64_t max_cycles;                                 /* longest counted read */
	int64_t n_unknown_base, n_quality_out_of_range;
} ngsqc_read_stats;
int ngsqc_scan_reads(ngsqc_handle* h, int32_t single_end, ngsqc_read_stats* st);
/* after ngsqc_scan_reads: reads per length 0..max_cycles (cap >= max_cycles + 1) */
int ngsqc_read_length_hist(ngsqc_handle* h, int64_t* out, int64_t cap);
/* after ngsqc_scan_reads: per cycle A, C, G, T, N counts and the quality sums of forward / reverse reads, out[7 * cycle + k],
 * for the first min(n_cycles, 320) cycles (per-cycle statistics only feed plots; longer reads are covered by the totals) */
int ngsqc_read_cycle_stats(ngsqc_handle* h, int64_t* out, int64_t n_cycles);

/* ---- raw-read QC of FASTQ text: FastqFileStream::readEntry + FastqEntry::validate (src/cppNGS/FastqFileStream.cpp:3-44, :133-156) and
 * StatisticsReads::update(const FastqEntry&, ReadDirection) (src/cppNGS/StatisticsReads.cpp:26-81), the loop of ReadQC (src/ReadQC/main.cpp:57-96). An
 * accumulator of its own, independent of any BAM handle. The caller inflates the file and feeds its TEXT in pieces cut anywhere (a piece and the carry in
 * front of it stay below 2 GiB); the device finds the lines (the four lines of entry r are lines 4r .. 4r + 3 of the file, by the newline count alone),
 * validates and counts every complete entry, and the rest waits as a carry in front of the next piece. direction: 0 forward, 1 reverse. last != 0 ends the
 * file: the carry is flushed and the next feed starts a new file. The kernels of a piece run while the caller prepares the next one: feed returns before
 * they end, and an error of piece k is reported by the feed of piece k + 1, by the last feed of the file or by ngsqc_fastq_result.
 * Lines end with "\n" or "\r\n"; a file need not end with a newline; lines at the end of a file that are all empty are ignored; an incomplete last entry
 * reads its missing lines as empty. An entry whose header line is empty is not validated and not counted in `entries` (FastqFileStream.cpp:151) but still
 * counted in the statistics (main.cpp:63-66), when its bases are all ACGTN, its qualities are in range and both have one length - otherwise error kind 6.
 * The first failing entry of the file, and within it the first check of validate that fails, makes feed return NGSQC_E_FORMAT with the reference's message
 * (ngsqc_fastq_last_error); the accumulator is void from then on. kinds: 1 the header does not start with '@', 2 the second header is empty or does not
 * start with '+', 3 bases and qualities differ in length, 4 a base outside ACGTN, 5 a quality character outside 33..74 (33..126 with long_read), 6 above. */
typedef struct ngsqc_fastq ngsqc_fastq;
typedef struct ngsqc_fastq_report {
	int64_t entries;                      /* entries with a non-empty header in the current (or just ended) file: FastqFileStream::index() + 1 */
	int64_t files;                        /* files begun */
	int64_t err_file, err_entry;          /* the first error: ordinal of the file, entry in it (every entry counts), -1: none */
	int32_t err_kind, reserved;
	double h2d_ms, kernels_ms, wait_ms;   /* HIP-event sums of the copies and of the kernels; host time spent waiting for a piece in flight */
} ngsqc_fastq_report;
int  ngsqc_fastq_create(int32_t device, int32_t long_read, ngsqc_fastq** out);
void ngsqc_fastq_destroy(ngsqc_fastq* f);
const char* ngsqc_fastq_last_error(const ngsqc_fastq* f);   /* f NULL: the last failing ngsqc_fastq_create of this thread */
int  ngsqc_fastq_feed(ngsqc_fastq* f, const uint8_t* text, int64_t n, int32_t direction, int32_t last);
/* waits for the piece in flight; st as ngsqc_scan_reads fills it (n_unknown_base and n_quality_out_of_range stay 0: such entries are errors). Either may be NULL. */
int  ngsqc_fastq_result(ngsqc_fastq* f, ngsqc_read_stats* st, ngsqc_fastq_report* rep);
/* after ngsqc_fastq_result: as ngsqc_read_length_hist / ngsqc_read_cycle_stats */
int  ngsqc_fastq_length_hist(ngsqc_fastq* f, int64_t* out, int64_t cap);
int  ngsqc_fastq_cycle_stats(ngsqc_fastq* f, int64_t* out, int64_t n_cycles);

/* ---- SeqPurge: adapter and quality trimming of paired-end reads (src/SeqPurge/AnalysisWorker.cpp:79-457, OutputWorker.cpp:36-77). An accumulator of its own,
 * like ngsqc_fastq: the caller inflates the two files and feeds their TEXT in pieces cut anywhere, each side with its own carry. The pairs a feed processes
 * are the entries complete on BOTH sides; the surplus of the side that is ahead waits. last != 0 ends the file pair (line structure as ngsqc_fastq: "\r\n",
 * a missing final newline, empty lines at the end, an incomplete last entry). Per pair the device fills a plan record of 8 int32: len1_in, len2_in,
 * insert_offset (-1: none), adapter_fwd (-1), adapter_rev (-1), len1_out, len2_out, flags (bit 0 / 1: read 1 / 2 quality-trimmed, bit 2 / 3: N-trimmed).
 * With outputs set, the surviving entries are written as BGZF (valid gzip, EOF member at the end) deflated on the device: both reads >= min_len to out1 /
 * out2; exactly one, when out3 is set, to out3_r1 or out3_r2; with ec the corrected bytes. Without outputs the plan is kept for ngsqc_purge_plan.
 * The first failing pair (the lowest ordinal over all file pairs, every pair counts) makes feed return NGSQC_E_FORMAT; kinds, in the order they are looked
 * for in a pair: 1 bases and qualities of a read differ in length (a message of this library's: the reference does not validate), 2 "Headers of reads do
 * not match:", 3 "Could not convert base 'x' to complement!" (read 2), 4 "Read length unsupported! ..." (1000 and more); 0: "File X has more entries than
 * Y!" at the end of a file pair (X, Y: ngsqc_purge_file_names, default in1 / in2). A byte of read 1 outside ACGTN matches nothing and is not N. create
 * refuses (NGSQC_E_ARG) adapters shorter than 15 ("Forward adapter X too short!") or with bytes outside ACGTN, and qwin < 1. */
typedef struct ngsqc_purge ngsqc_purge;
typedef struct ngsqc_purge_params {
	const char* a1; const char* a2;       /* forward / reverse adapter */
	double match_perc, mep;
	int32_t min_len, qcut, qwin, qoff, ncut, ec;
} ngsqc_purge_params;
typedef struct ngsqc_purge_stats {
	int64_t pairs;                        /* pairs processed */
	int64_t read_num, reads_trimmed_insert, reads_trimmed_adapter, reads_trimmed_q, reads_trimmed_n, reads_removed;   /* TrimmingStatistics (Auxilary.h:136-163) */
	double  bases_perc_trim_sum;          /* summed in pair order */
	int64_t bases_remaining[1000];        /* reads per length after trimming */
	int64_t acons[2 * 40 * 5];            /* consensus pile-ups [adapter 1 / 2][position][A C G T N] */
	int64_t ec_mismatch_r1[1000], ec_mismatch_r2[1000], ec_errors_per_read[1000];   /* ErrorCorrectionStatistics */
	int64_t err_pair; int32_t err_kind, reserved;   /* the first error: pair ordinal (-1: none) and kind */
	double  h2d_ms, index_ms, plan_ms, format_ms, deflate_ms, wait_ms;   /* HIP-event sums of the copies, the line index, the plan kernel and the format kernels (with their sizes and positions); host time of deflate and copy-out, and of waiting */
} ngsqc_purge_stats;
int  ngsqc_purge_create(int32_t device, const ngsqc_purge_params* params, ngsqc_purge** out);
void ngsqc_purge_destroy(ngsqc_purge* p);
const char* ngsqc_purge_last_error(const ngsqc_purge* p);   /* p NULL: the last failing ngsqc_purge_create of this thread */
/* once, before the first feed; out3_r1 and out3_r2 both NULL (no singleton files) or both set; compression_level 0..9 */
int  ngsqc_purge_outputs(ngsqc_purge* p, const char* out1, const char* out2, const char* out3_r1, const char* out3_r2, int32_t compression_level);
int  ngsqc_purge_file_names(ngsqc_purge* p, const char* name1, const char* name2);   /* the names in "File X has more entries than Y!" from now on */
int  ngsqc_purge_feed(ngsqc_purge* p, const uint8_t* text1, int64_t n1, const uint8_t* text2, int64_t n2, int32_t last);
/* closes the outputs (no feed may follow) and fills st (may be NULL); after an error the statistics hold the feeds in front of the failing one */
int  ngsqc_purge_result(ngsqc_purge* p, ngsqc_purge_stats* st);
/* without outputs: the plan rows of pairs [first, first + n) into out[n][8] */
int  ngsqc_purge_plan(ngsqc_purge* p, int64_t first, int64_t n, int32_t* out);

/* ---- the per-entry FASTQ-to-FASTQ tools: FastqTrim, FastqExtract, FastqExtractUMI, FastqConvert, FastqExtractBarcode, FastqAddBarcode, FastqDownsample,
 * FastqConcat (src/<tool>/main.cpp). "Edit every entry of a FASTQ stream
 * and write it again": an accumulator like ngsqc_purge. The caller inflates the input and feeds its TEXT in pieces cut anywhere; FastqExtractUMI has two
 * inputs ("sides"), each with its own carry, and a feed processes the entries complete on both; the other operations have one (text2 NULL, n2 0). last != 0
 * ends the input (line structure as ngsqc_fastq); with two sides the run ends silently at the shorter one. An operation has one or two output STREAMS, and
 * for the first four stream k holds the entries of side k; the table below names sides and streams of the others. last ends a FILE: a feed behind it begins
 * the next file (FastqConcat's and FastqAddBarcode's lists), output positions and entry ordinals carry on. Per entry and stream the device fills a plan record
 * of 8 int32:
 *   [0] keep     1: the entry is written, 0: dropped (the ranges below then describe the whole lines)
 *   [1] ins_at   byte offset in the header line in front of which text is inserted
 *   [2] ins_len  bytes inserted there (FastqExtractUMI: ":" cut1 "," cut2 ":" umi1 "," umi2, composed on the device from both reads; 0 otherwise)
 *   [3] b_off    [4] b_len   the kept part of the bases line
 *   [5] q_off    [6] q_len   the kept part of the quality line (the two lines may differ in length: only FastqExtract validates)
 *   [7] q_delta  added to every kept quality byte, modulo 256 (FastqConvert: -31)
 * No line ever grows: a range is cut to the line it lies in. With outputs set, the kept entries are written as BGZF (valid gzip, EOF member at the end)
 * deflated on the device: header with the insertion, kept bases, line 3 as it is, kept qualities, each followed by "\n". Without outputs the plan is kept
 * for ngsqc_fqedit_plan.
 *   NGSQC_FQEDIT_TRIM     start, end, len, max_len (all >= 0): bases >= max_len > 0: unchanged; start or end > 0: dropped when bases <= start + end, else
 *                         [start, bases - start - end) of both lines; then both cut to len > 0 when the bases are longer
 *   NGSQC_FQEDIT_EXTRACT  ids from ngsqc_fqedit_ids; the id of an entry is its trimmed header without the first byte, up to the first space. Not listed:
 *                         written only with invert. Listed without a length (-1): written only without invert. Listed with length >= 1: without invert,
 *                         written cut to that length (a length beyond the read keeps the whole read). Length 0 or below -2: dropped. Every entry with a
 *                         non-empty header is validated with the kinds 1..5 of ngsqc_fastq, long_read included: the first failing entry makes feed return NGSQC_E_FORMAT
 *                         with the reference's message, and the accumulator is void from then on
 *   NGSQC_FQEDIT_UMI      cut1, cut2 (>= 0): the first cut k bytes of the bases and quality lines of read k go (a shorter line becomes empty)
 *   NGSQC_FQEDIT_CONVERT  every quality byte - 31
 *   NGSQC_FQEDIT_BARCODE_CUT  one side, two streams, both from side 0; cut1 (>= 0) is the cut. Stream 1 (main): the bases and quality lines without their first
 *                         cut bytes (a shorter line becomes empty); stream 2 (index): the first cut bytes of each line, or the bytes there are
 *   NGSQC_FQEDIT_BARCODE_ADD  three sides (ngsqc_fqedit_feed3), two streams from sides 0 and 1: the text ":" len3 ",0:" bases3 "," - the bases line of the entry
 *                         of side 2 and its length in decimal - goes behind the first space-delimited token of both headers, composed on the device
 *   NGSQC_FQEDIT_DOWNSAMPLE  two sides, two streams; ngsqc_fqedit_downsample comes first. Pair r of the whole run (all feeds) is written when value r of glibc's
 *                         rand() behind srand(seed) says so, as ngsqc_downsample_keep(seed, percentage, r, 1) does; the decisions are made on the device
 *   NGSQC_FQEDIT_COPY     one side, one stream: every entry as it is */
enum { NGSQC_FQEDIT_TRIM = 0, NGSQC_FQEDIT_EXTRACT = 1, NGSQC_FQEDIT_UMI = 2, NGSQC_FQEDIT_CONVERT = 3,
       NGSQC_FQEDIT_BARCODE_CUT = 4, NGSQC_FQEDIT_BARCODE_ADD = 5, NGSQC_FQEDIT_DOWNSAMPLE = 6, NGSQC_FQEDIT_COPY = 7 };
typedef struct ngsqc_fqedit ngsqc_fqedit;
typedef struct ngsqc_fqedit_params {
	int32_t op, long_read;                /* NGSQC_FQEDIT_*; long_read: qualities up to 126 are valid, and a wave per entry in the plan of EXTRACT */
	int32_t start, end, len, max_len;     /* TRIM */
	int32_t cut1, cut2;                   /* UMI; BARCODE_CUT: cut1 */
	int32_t invert, reserved;             /* EXTRACT: -v */
} ngsqc_fqedit_params;
typedef struct ngsqc_fqedit_stats {
	int64_t entries;                      /* entries read (per side) */
	int64_t written[2], bytes[2];         /* entries and text bytes given to output stream 1 / 2 (counted with or without outputs) */
	int64_t err_entry; int32_t err_kind, reserved;   /* the first failing entry (-1: none) and the kind of ngsqc_fastq */
	double  h2d_ms, index_ms, plan_ms, format_ms, deflate_ms, wait_ms;   /* as ngsqc_purge_stats */
} ngsqc_fqedit_stats;
int  ngsqc_fqedit_create(int32_t device, const ngsqc_fqedit_params* params, ngsqc_fqedit** out);
void ngsqc_fqedit_destroy(ngsqc_fqedit* e);
const char* ngsqc_fqedit_last_error(const ngsqc_fqedit* e);   /* e NULL: the last failing ngsqc_fqedit_create of this thread */
/* EXTRACT, once, before the first feed: n ids, their bytes one behind the other in names, lengths[i] the length column (-1: none; lengths NULL: none has one).
 * A later duplicate of an id replaces the earlier one; an id with length -2 is as good as not listed. The table lives in device memory, open-addressed,
 * hashed by the read-name hash of the mate join (NGSQC_NAME_HASH_BITS truncates it); a hash hit is confirmed by comparing the bytes. */
int  ngsqc_fqedit_ids(ngsqc_fqedit* e, const void* names, const int32_t* name_len, const int32_t* lengths, int64_t n);
/* once, before the first feed; out2 for exactly the operations with two streams (UMI, BARCODE_CUT: the index, BARCODE_ADD, DOWNSAMPLE); compression_level 0..9 */
int  ngsqc_fqedit_outputs(ngsqc_fqedit* e, const char* out1, const char* out2, int32_t compression_level);
int  ngsqc_fqedit_feed(ngsqc_fqedit* e, const uint8_t* text1, int64_t n1, const uint8_t* text2, int64_t n2, int32_t last);   /* refuses BARCODE_ADD: it has three sides */
/* the same with a third side; an operation with fewer sides takes NULL / 0 for the sides it does not have */
int  ngsqc_fqedit_feed3(ngsqc_fqedit* e, const uint8_t* text1, int64_t n1, const uint8_t* text2, int64_t n2, const uint8_t* text3, int64_t n3, int32_t last);
/* DOWNSAMPLE, once, before the first feed: the seed of srand() and the percentage of pairs to keep (NGSQC_E_ARG outside (0, 100)); want_headers != 0 keeps the
 * header lines of side 0 of the kept pairs, gathered on the device, for ngsqc_fqedit_kept_headers */
int  ngsqc_fqedit_downsample(ngsqc_fqedit* e, uint32_t seed, double percentage, int32_t want_headers);
/* the entries seen on each side so far, those no partner came for included (behind the last piece of a file: every entry of every side) */
int  ngsqc_fqedit_side_entries(const ngsqc_fqedit* e, int64_t out[3]);
/* after ngsqc_fqedit_result: the kept header lines, each followed by "\n", n bytes in all; the text belongs to the accumulator and goes with ngsqc_fqedit_destroy */
int  ngsqc_fqedit_kept_headers(ngsqc_fqedit* e, char** text, int64_t* n);
/* closes the outputs (no feed may follow) and fills st (may be NULL) */
int  ngsqc_fqedit_result(ngsqc_fqedit* e, ngsqc_fqedit_stats* st);
/* without outputs: the plan rows of entries [first, first + n) into out[n][streams][8], streams = 2 for UMI, BARCODE_CUT, BARCODE_ADD and DOWNSAMPLE, 1 otherwise */
int  ngsqc_fqedit_plan(ngsqc_fqedit* e, int64_t first, int64_t n, int32_t* out);

/* ---- fused job: ONE pass over the BAM for every consumer --------------------------------------------------------------------
 * The reference re-reads the BAM for every pass of a tool: MappingQC runs Statistics::mapping*, then Statistics::contamination
 * (src/MappingQC/main.cpp:100-151), optionally StatisticsReads (-read_qc, :83-98) and Statistics::somaticCustomDepth
 * (-somatic_custom_bed, :153-165). Here every BGZF member is inflated once per job and each requested consumer sees every tile
 * of the inflated stream while it is resident in HBM. NULL / 0 switches a consumer off. The single-purpose entry points above
 * (ngsqc_scan_mapping, ngsqc_scan_depth, ngsqc_site_pileup, ngsqc_scan_reads) are jobs with one consumer.
 * After the job, depth set 0 holds the mapping scan's per-base depth and depth set 1 the extra depth scan's; ngsqc_depth_select
 * picks the one that ngsqc_depth_stats / _copy / ngsqc_region_sums / ngsqc_lowhigh_runs read (a job leaves set 0 selected when it
 * had a mapping scan, otherwise set 1; ngsqc_scan_depth uses set 0). */
typedef struct ngsqc_job_desc {
	const ngsqc_mapping_params* mapping;     /* Statistics::mapping / mapping_wgs, or NULL                                      */
	const ngsqc_depth_params* depth;         /* extra depth scan on its own regions (somaticCustomDepth), or NULL               */
	const ngsqc_region* sites; int64_t n_sites;   /* site pileup (Statistics::contamination), n_sites == 0: off                 */
	int32_t site_min_mapq, site_min_baseq, site_include_npp;
	int32_t read_qc, read_qc_single_end;     /* StatisticsReads::update for every record                                         */
	int32_t reserved;
} ngsqc_job_desc;
typedef struct ngsqc_job_result {
	int64_t* counters; double* gc_reads;     /* mapping: int64[NGSQC_NCOUNTERS], double[101] (may be NULL)                       */
	int64_t* site_counts;                    /* int64[8 * n_sites]                                                               */
	ngsqc_read_stats* read_stats;            /* (+ ngsqc_read_length_hist / ngsqc_read_cycle_stats afterwards)                   */
} ngsqc_job_result;
int ngsqc_run_job(ngsqc_handle* h, const ngsqc_job_desc* job, ngsqc_job_result* result);
int ngsqc_depth_select(ngsqc_handle* h, int32_t which);

/* ---- one BAM sharded over several handles / GPUs --------------------------------------------------
 * The reference reads a BAM with one sequential reader (BamReader::getNextAlignment, src/cppNGS/BamReader.h:386-398); its
 * loop bodies (Statistics.cpp:416-574, :830-917, :1068-1183) are independent per record except for two carries: the
 * running maximum read length behind bases_trimmed (:428-429,:565-568) and "a paired read has been seen" (:879,:1115).
 * A shard handle owns the records that START inside its contiguous range of BGZF members (equal compressed bytes, cut at
 * member starts); the members behind the range are inflated only to complete its last record. Protocol per shard:
 *   ngsqc_open_shard -> ngsqc_scan_mapping_partial (local scan) -> exchange the summaries (all-gather, 48 bytes each) ->
 *   ngsqc_plan_shard_fix (pure host logic, also verifies the record chain across shards) -> ngsqc_scan_mapping_finish
 *   (local fix-up on the record prefix the carries touch; returns ADDITIVE counters) -> SUM all-reduce of the counters
 *   (MAX for max_length / paired_end / yx_valid) and of the difference array (ngsqc_depth_device, in place) ->
 *   ngsqc_depth_finalize -> ngsqc_depth_stats on the summed array.                                                   */
int ngsqc_open_shard(const char* bam_path, int device, int shard, int n_shards, ngsqc_handle** out);
int ngsqc_open_memory_shard(const void* bam_bytes, size_t n_bytes, int device, int shard, int n_shards, ngsqc_handle** out);

/* ---- index-driven partial decode: what BamReader::setRegion gives the reference (src/cppNGS/BamReader.cpp:734-768, htslib sam_index_load /
 * sam_itr_queryi): a region query reads only the BGZF blocks the BAI names. ngsqc_bai_range turns a set of regions (1-based, closed) into ONE
 * virtual-offset range [beg, end) that holds every record overlapping any of them (found = 0: none can); NGSQC_E_IO when there is no <bam>.bai:
 * "Could not load index of BAM/CRAM file ..." like the reference. ngsqc_open_range opens a handle over the records of such a range: only its BGZF
 * members (and those of the BAM header) are sent to the device and inflated. Scans that only depend on the reads overlapping the regions
 * (depth scans, site pileups, read counts) give the same result as on the whole file. */
int ngsqc_bai_range(const char* bam_path, const ngsqc_region* regions, int64_t n_regions, int32_t n_ref, uint64_t* beg_voff, uint64_t* end_voff, int32_t* found);
/* the same range for EVERY region on its own (one load of the index): beg_voff[i] / end_voff[i], end_voff[i] == 0 when no record can overlap region i. Regions that lie
 * far apart in the file are better served by one partial handle per cluster of ranges than by the one range from the first to the last (host layer: avgCoverage). */
int ngsqc_bai_ranges(const char* bam_path, const ngsqc_region* regions, int64_t n_regions, int32_t n_ref, uint64_t* beg_voff, uint64_t* end_voff);
int ngsqc_open_range(const char* bam_path, int device, uint64_t beg_voff, uint64_t end_voff, ngsqc_handle** out);
/* the same in one call for named regions (reference names as in the BAM header, with or without "chr"): header -> tids -> BAI -> range. Only the BGZF
 * members of the header and of the range are walked on the host and sent to the device. No overlapping record: a handle without records. */
typedef struct ngsqc_named_region { const char* chr; int32_t start, end; } ngsqc_named_region;
int ngsqc_open_regions(const char* bam_path, int device, const ngsqc_named_region* regions, int64_t n_regions, ngsqc_handle** out);
/* the first records of the file: the BGZF members of the BAM header and n_members behind them (what BamReader::info needs, BamReader.cpp:593-730) */
int ngsqc_open_head(const char* bam_path, int device, int64_t n_members, ngsqc_handle** out);
/* SAM header text of the BAM header (NUL-terminated copy into out[cap] when out != NULL); returns its length, -1 without a handle */
int64_t ngsqc_header_text(const ngsqc_handle* h, char* out, int64_t cap);

/* The BGZF member table of a BAM image on the host (SAM spec 4.1; what ngsqc_open builds before anything reaches the device; no device needed): members that
 * inflate to nothing (the EOF block) are left out. n_threads > 1 walks the file in pieces (accepted only when the pieces join exactly; else the sequential walk).
 * NGSQC_E_FORMAT with the message of the first broken member. */
typedef struct ngsqc_bgzf_member { uint64_t file_offset, payload_offset, inflated_offset; uint32_t payload_bytes, inflated_bytes, crc32, walked_in_pieces /* 1: the table came from the multi-thread walk */; } ngsqc_bgzf_member;
int ngsqc_bgzf_scan(const void* bam_bytes, size_t n_bytes, int32_t n_threads, ngsqc_bgzf_member* out, int64_t cap, int64_t* n_members, int64_t* inflated_bytes);

/* ---- CRAM 3.0 / 3.1 input. The reference opens CRAM through the same BamReader (htslib; BamReader.cpp:482-492) with the reference genome the caller names
 * (hts_set_fai_filename). Here every ngsqc_open* entry point takes a CRAM 3.0 or 3.1 file: its container layer (containers, slices, blocks with CRC-32, gzip and rANS
 * 4x8 blocks, the encodings, read features, mate chains, the slices' reference MD5) is decoded on the HOST into BAM records, which reach the device as a BAM image
 * whose BGZF members hold stored blocks - the device path (K1's stored-block copy, record index, walk, depth, counters) is the BAM path. The quality arrays
 * (rANS blocks) of a whole-file handle are decoded on the device into that image (cram_dev.hip; NGSQC_CRAM_DEVICE_QUALS=0: on the host). Index-driven
 * requests on a CRAM (ngsqc_open_regions) decode only the slices whose headers overlap a region - what the .crai names, read from the slice headers themselves;
 * ngsqc_open_head the first two slices; ngsqc_open_range the whole file. ngsqc_set_reference names the genome (FASTA with .fai; NULL / "": none; NGSQC_REFERENCE is the
 * fallback) for files that need one (preservation key RR); without it: NGSQC_E_IO "Error while setting reference genome ...", a genome that does not match a
 * slice's MD5: NGSQC_E_FORMAT. CRAM 3.1: rANS Nx16 blocks are decoded; the adaptive arithmetic coder, fqzcomp and the name tokeniser are NGSQC_E_UNSUPPORTED - a name-tokeniser block only
 * when names are asked for (ngsqc_set_cram_skip: the tools never do) (bzip2 / lzma blocks need libbz2 / liblzma on the machine, loaded on first use). ngsqc_cram_to_bam writes the decoded records as a BAM file
 * (host only; the checker of the decoder: tests compare it record by record with oracle/cram_decode.py). */
int ngsqc_set_reference(const char* fasta_path);
/* What later ngsqc_open* calls on a CRAM need not decode (process-wide, like ngsqc_set_reference). Replaces BamReader::skipTags() and the read-name half of
 * htslib's CRAM_OPT_REQUIRED_FIELDS, src/cppNGS/BamReader.cpp:525-572: the reference's coverage workers drop bases, tags and qualities before they iterate
 * (WorkerLowOrHighCoverage.cpp:28-31). Names: every record carries "*"; tags: no optional fields except RG. Only external blocks that no other series reads are
 * left un-inflated (a series kept in the core block is decoded and dropped). No QC result reads a name; MappingQC's target-region mode reads the DP tag. */
#define NGSQC_CRAM_SKIP_NAMES 1
#define NGSQC_CRAM_SKIP_TAGS  2
int ngsqc_set_cram_skip(int32_t flags);
/* The same choice for the files the CALLING THREAD opens from now on (flags >= 0; -1: back to the process-wide choice). Returns the thread's previous value (-1: none),
 * so that a scope can restore what it found: a function that needs tags for its own reader (Statistics::mapping reads DP) must not change what a reader opened by
 * another thread decodes. */
int32_t ngsqc_set_cram_skip_thread(int32_t flags);
int ngsqc_cram_to_bam(const char* cram_path, const char* bam_path, const ngsqc_named_region* regions, int64_t n_regions);   /* regions NULL / 0: every record */

/* ---- writing a BAM: BamFilter (src/BamFilter/main.cpp:71-134) over the BGZF writer of BamWriter (src/cppNGS/BamWriter.cpp). Records with flag 0x100 or 0x800
 * are skipped; every other record, in file order, opens an entry for its exact read name or closes the open one (names that occur 3, 4, 5 times pair as
 * (1,2), (3,4), ...). A closed pair in which both records pass alignment_pass (main.cpp:35-68, the thresholds below; -1 disables max_mm / max_gap / max_is) is
 * written - the opener, then the closer, in the order of the closing records - and counted as passed, otherwise as dropped; entries still open at the end are
 * dropped silently. The output is the input's header bytes in members of their own, then the kept records byte for byte (a record whose CIGAR came from a CG
 * tag is written as htslib's bam_write1 writes it: see DESIGN.md) in BGZF members of 0xff00 bytes, then the EOF member. The pairing needs the whole file: a
 * handle opened on a shard, a range, regions or the first records (BAM or CRAM) gives NGSQC_E_ARG. Open names are kept in device memory: NGSQC_E_DEVICE when
 * they do not fit. The writer works in windows of about 1 GiB of the uncompressed output: its memory does not grow with the file. */
typedef struct { int32_t min_mq, max_mq, max_mm, max_gap, min_dup, max_is; } ngsqc_pair_filter;
int ngsqc_filter_pairs(ngsqc_handle* h, const ngsqc_pair_filter* p, const char* out_bam_path, int64_t* pairs_passed, int64_t* pairs_dropped);
/* The encoder of that writer on a buffer: BGZF members of the 0xff00-byte pieces of in (dynamic Huffman DEFLATE, or a stored block where that is smaller), no
 * EOF member; n == 0 gives no bytes. *out_n: the whole compressed size, also when it exceeds cap (then NGSQC_E_ARG, and out does not hold the result). Deterministic. */
int ngsqc_bgzf_compress(const void* in, size_t n, int device, void* out, size_t cap, size_t* out_n);
/* The same encoder at a compression level: 0 stored blocks, 1-3 a fast greedy parse (short hash chains, no lazy step), 4-9 the parse of ngsqc_bgzf_compress
 * (byte-identical to it). Deterministic at every level. NGSQC_E_ARG for a level outside 0..9. */
int ngsqc_bgzf_compress_level(const void* in, size_t n, int device, int level, void* out, size_t cap, size_t* out_n);

/* ---- BamDownsample (src/BamDownsample/main.cpp:31-101) over the same join and writer. Records with flag 0x100 or 0x800 are skipped (:58). A record without
 * flag 0x1 is a single-end record (:60-69): it draws the next random number and, when kept, is written at once. A record with flag 0x1 opens an entry for its
 * exact read name or closes the open one (:70-91; names that occur 3, 4, 5 times pair as (1,2), (3,4), ...; no filter on mapped, MAPQ or mate flags); the
 * closing record draws the next random number and, when kept, the opener and then the closer are written. Entries still open at the end are pe_unmatched (:100).
 * The k-th deciding record in file order uses the k-th value of glibc's rand() behind srand(seed) (:36; seed 0 is seed 1 in glibc) as
 * Helper::randomNumber(0, 100) = 0 + (double)rand() / RAND_MAX * 100, and is kept when that is < percentage (:63, :80). The output is written as
 * ngsqc_filter_pairs writes it (header bytes, records byte for byte, CG-tag records as bam_write1 writes them, 0xff00-byte members, the EOF member).
 * A percentage outside (0, 100) is NGSQC_E_ARG (:38), as is a handle on a shard, a range, regions or the first records. want_names != 0: *kept_names receives
 * the kept deciding records in stream order as "SE\tname\n" / "PE\tname\n" lines (NUL-terminated, malloc'ed: the caller frees it; what -test prints, :67, :85);
 * without want_names kept_names may be NULL, and *kept_names is set to NULL when it is not. */
typedef struct { double percentage; uint32_t seed; int32_t want_names; } ngsqc_downsample_params;
typedef struct { int64_t se, se_written, pe, pe_written, pe_unmatched; } ngsqc_downsample_counts;
int ngsqc_downsample(ngsqc_handle* h, const ngsqc_downsample_params* p, const char* out_bam_path, ngsqc_downsample_counts* c, char** kept_names);
/* The decision stream of that writer on its own (its generator on a range of ordinals; like ngsqc_bgzf_compress for the encoder): out[i] = 1 when the deciding
 * record with ordinal first + i is kept, else 0. One device lane walks NGSQC_DOWNSAMPLE_CHUNK consecutive values from a start state that the host reaches by
 * jumping, so the host work does not grow with first. NGSQC_E_ARG for a percentage outside (0, 100), first < 0 or n < 0. */
#define NGSQC_DOWNSAMPLE_CHUNK 3968
int ngsqc_downsample_keep(uint32_t seed, double percentage, int64_t first, int64_t n, int device, uint8_t* out);

/* ---- BamExtract (src/BamExtract/main.cpp:27-83) over the same writer, without the join. EVERY record of the file is a candidate (:64-76): secondary,
 * supplementary and unmapped records are looked up and written like any other. A record whose name is one of the listed names goes to out_bam_path (:66-70);
 * with out2_bam_path (not NULL and not "") every other record goes there (:71-75); without it the others are neither written nor counted. Each output holds
 * its records in file order. A record's name is what BamAlignment::name() returns (src/cppNGS/BamReader.h:69-72, bam_get_qname read as a C string): the bytes
 * in front of the first NUL of its l_read_name bytes. The listed names are the n_names byte strings laid end to end in names, name_len[i] bytes each, with
 * no separators; duplicates are taken once. A listed name that no record can carry (no bytes, more than 254 bytes, a NUL byte inside) matches nothing and still
 * counts as listed. counts->names: the distinct listed names (the reference's ids.count(), :45). The set of names lives in device memory for the call (a hash
 * table of 16 bytes per slot, at least two slots per name, next to the names' bytes): NGSQC_E_DEVICE "BamExtract: the set of read names does not fit in device
 * memory (N MiB needed, M MiB free)" when it does not fit. Both outputs are written as ngsqc_filter_pairs writes its output (header bytes, records byte for
 * byte, CG-tag records as bam_write1 writes them, 0xff00-byte members, the EOF member). NGSQC_E_ARG for a null pointer, a negative count or length, and for a
 * handle on a shard, a range, regions or the first records. */
typedef struct { int64_t out, out2, names; } ngsqc_extract_counts;
int ngsqc_extract_reads(ngsqc_handle* h, const void* names, const int32_t* name_len, int64_t n_names, const char* out_bam_path, const char* out2_bam_path, ngsqc_extract_counts* counts);
/* The lookup of that tool on its own (like ngsqc_downsample_keep for the decision stream): match_out[i] = 1 when the name of the i-th record of the file, in
 * file order, is one of the listed names, else 0. No file is written. cap: the bytes match_out holds; NGSQC_E_ARG when the file has more records. */
int ngsqc_match_names(ngsqc_handle* h, const void* names, const int32_t* name_len, int64_t n_names, uint8_t* match_out, int64_t cap);

/* ---- BamCleanHaloplex (src/BamCleanHaloplex/main.cpp:27-69) over the same writer, without the join. Every record of the file is written, in file order, behind
 * the input's header. A record is a candidate when it is none of unmapped (0x4), secondary (0x100), duplicate (0x400) or supplementary (0x800). A candidate whose
 * CIGAR's M operations (op 0 alone: '=' and 'X' do not count) add up to less than min_match fails: 0x4 and 0x100 are set in its flag word, and nothing else of
 * the record changes (bin, the mate fields and the tags are the input's). The CIGAR is the one htslib hands out: a record whose CIGAR sits in a CG:B,I tag is
 * judged on the tag's operations and written as bam_write1 writes it. counts: the records, the candidates, the failed ones (`int` in the reference; 64-bit
 * here, as is the sum of a CIGAR). The output is written as ngsqc_filter_pairs writes its output. NGSQC_E_ARG for a null pointer and for a handle on a shard, a
 * range, regions or the first records. */
typedef struct { int64_t reads, candidates, failed; } ngsqc_haloplex_counts;
int ngsqc_clean_haloplex(ngsqc_handle* h, int32_t min_match, const char* out_bam_path, ngsqc_haloplex_counts* counts);
/* The verdicts of that tool on their own (like ngsqc_match_names): out[i] for the i-th record of the file in file order: 0 not a candidate, 1 a candidate that
 * is kept, 2 a candidate that fails. No file is written. cap: the bytes out holds; NGSQC_E_ARG when the file has more records. */
int ngsqc_haloplex_verdicts(ngsqc_handle* h, int32_t min_match, uint8_t* out, int64_t cap);

/* ---- BamRemoveVariants (src/BamRemoveVariants/main.cpp:34-278) over the same join and writer: read pairs that carry a variant of a VCF are dropped, or with
 * mask kept with the reference base put back. Records with flag 0x100 or 0x800 are counted as skipped and take no further part (:141-145); every other record
 * takes part. A table line overlaps a record when tid matches and [beg, end] meets [pos + 1, pos + max(1, reference length)] (the reference length is 0 with flag
 * 0x4 or without a CIGAR: bam_endpos; a record with tid < 0 or pos < 0 overlaps nothing). The overlapping lines are visited in table order:
 *   SNV      the base at `start` by BamAlignment::extractBaseByCIGAR (src/cppNGS/BamReader.cpp:307-374); the record carries the line when that base is obs. An
 *            index outside [0, l_seq), which the reference reads past the sequence, gives no base. A walk that ends in front of start: error POS_NOT_FOUND (:373).
 *   OTHER    the record carries the line when extractIndelsByCIGAR(start, 50) (:376-439) is non-empty: an I / D operation at a genome position in [start - 50, start + 50].
 *   INVALID  error INVALID_LINE (what Variant(const VcfLine&) throws, src/cppNGS/VariantList.cpp:59).
 * Default mode: the visit ends at the first carried line, and the record passes when there is none. mask: a carried SNV sets the base to ref (setBases,
 * BamReader.cpp:133-175, rewrites the whole sequence: a base other than A, C, G, T, N anywhere in the read is error BAD_BASE), later lines see the new base; the
 * first carried OTHER line ends the visit and the record passes when keep_indels is set; without one it passes. modified: the sequence differs from the input's.
 * An error ends the visit and the record does not pass. Pairing is ngsqc_filter_pairs' rule (the first record of a name opens, the next closes): a pair is written,
 * opener then closer, at the closer's position when both pass; passed / dropped count closed pairs. A closer is only visited when its opener passed (:218, :251):
 * its modified and its error do not count otherwise; an opener's always do. single_end: no join, a record that passes is written at its own position, passed /
 * dropped count records, modified counts written records (:155-160). The first error in file order stops the run: NGSQC_E_FORMAT with the reference's message, and
 * counts->err_record (ordinal in the file), err_code and err_variant (index into variants; for BAD_BASE the index of the base in the read) say where.
 * variants: n lines in file order; the lines of one tid must be contiguous with non-decreasing beg (NGSQC_E_ARG otherwise); lines with tid < 0 or beyond the
 * header are ignored. The table lives in device memory for the call next to the running maximum of end, by which a record finds its first candidate line. */
enum { NGSQC_RMVAR_SNV = 0, NGSQC_RMVAR_OTHER = 1, NGSQC_RMVAR_INVALID = 2 };
enum { NGSQC_RMERR_NONE = 0, NGSQC_RMERR_INVALID_LINE = 1, NGSQC_RMERR_POS_NOT_FOUND = 2, NGSQC_RMERR_BAD_BASE = 3 };
typedef struct { int32_t tid, beg, end, start; uint8_t kind, ref, obs, pad; } ngsqc_rm_variant;   /* beg = POS, end = POS + len(REF) - 1, start: after normalize("-", true); ref / obs: the SNV's bases */
typedef struct { int32_t mask, single_end, keep_indels; } ngsqc_rm_params;
typedef struct { int64_t passed, dropped, modified, skipped; int64_t err_record; int32_t err_code, err_variant; } ngsqc_rm_counts;
int ngsqc_remove_variants(ngsqc_handle* h, const ngsqc_rm_variant* variants, int64_t n, const ngsqc_rm_params* p, const char* out_bam_path, ngsqc_rm_counts* counts);
/* The verdicts of that tool on their own (like ngsqc_match_names): out[i] for the i-th record of the file, the record's own visit whatever its mate's:
 * bit 0 passes, bit 1 modified, bit 2 skipped (flag 0x900), bit 3 error. No file is written. cap: the bytes out holds; NGSQC_E_ARG when the file has more records. */
int ngsqc_variant_verdicts(ngsqc_handle* h, const ngsqc_rm_variant* variants, int64_t n, const ngsqc_rm_params* p, uint8_t* out, int64_t cap);

/* ---- BamClipOverlap (src/BamClipOverlap/main.cpp:43-554, NGSHelper::softClipAlignment NGSHelper.cpp:670-810): the read pairs of the whole file whose two
 * alignments overlap are soft-clipped so that every reference base is covered by one of them. A record that is unpaired, secondary, supplementary, unmapped,
 * whose mate is unmapped or on another reference, or whose CIGAR holds only I / S (as htslib shows it: a CG tag's CIGAR in place) is written as it is at its own
 * place. Every other record enters the name map: the 1st and 2nd record of a name are a pair, a 3rd opens again. A pair is written at its closer's place, the
 * forward read first (the opener, unless the strands differ and the closer is the forward one). mode_bits: what a base mismatch in the overlap does -
 * precedence MAPQ > REMOVE > BASEQ > BASEN. ignore_indels: an indel within 4 bases of the clip position no longer sends the whole clip to one mate (to the
 * reverse read when the number of soft-clipped pairs in front of the pair is even, else to the forward read; removed pairs count). A clipped record has pos,
 * n_cigar_op, its CIGAR, next_pos and tlen rewritten and "BS:Z:<old CIGAR>" appended behind its tags; its bin field keeps the input's bytes. The names still open at the end are
 * written in file order (the reference: QHash order). level: -1 (default) or 0 .. 9. counts: reads, saved, clipped, mismatch, bases, bases clipped (the first
 * four are `int` in the reference; here 64-bit). The earliest error in file order stops the run: NGSQC_E_FORMAT with the reference's message and *err (may be
 * null) filled: the ordinal of the closing record, the code and its two integers (CIGAR_CHAR, SC_OP, BAD_BASE: the character; LENGTH: the two list lengths -
 * also where the reference reads behind the shorter list). A soft-clipped pair with a CG-tag CIGAR, or whose new CIGAR needs more than 65535 operations, is
 * NGSQC_E_UNSUPPORTED (code UNSUPPORTED). ORIENT, SC_ORDER, SC_START and SC_END cannot be reached. A handle on a shard, a range or regions: NGSQC_E_ARG. */
enum { NGSQC_CLIP_MAPQ = 1, NGSQC_CLIP_REMOVE = 2, NGSQC_CLIP_BASEQ = 4, NGSQC_CLIP_BASEN = 8 };
enum { NGSQC_CLIPERR_NONE = 0, NGSQC_CLIPERR_ORIENT, NGSQC_CLIPERR_CIGAR_CHAR, NGSQC_CLIPERR_LENGTH, NGSQC_CLIPERR_SC_ORDER, NGSQC_CLIPERR_SC_START, NGSQC_CLIPERR_SC_END,
       NGSQC_CLIPERR_SC_INDEX, NGSQC_CLIPERR_SC_OP, NGSQC_CLIPERR_BAD_BASE, NGSQC_CLIPERR_UNSUPPORTED };
enum { NGSQC_CLIP_ROLE_PASS = 0, NGSQC_CLIP_ROLE_FORWARD = 1, NGSQC_CLIP_ROLE_REVERSE = 2, NGSQC_CLIP_ROLE_LEFTOVER = 3 };
enum { NGSQC_CLIP_V_PAIR = 1, NGSQC_CLIP_V_MISMATCH = 2, NGSQC_CLIP_V_REMOVED = 4, NGSQC_CLIP_V_MAPQ0 = 8, NGSQC_CLIP_V_QUAL = 16, NGSQC_CLIP_V_BASES = 32, NGSQC_CLIP_V_REWRITTEN = 64 };
typedef struct { int64_t record; int32_t code, a, b; } ngsqc_clip_error;
int ngsqc_clip_overlap(ngsqc_handle* h, const char* out_bam_path, int32_t mode_bits, int32_t ignore_indels, int32_t level, int64_t* counts /* [6] */, ngsqc_clip_error* err);
/* The plan of that tool on its own, no file written: six integers per record of the file in file order - the role (NGSQC_CLIP_ROLE_*), the bases clipped from
 * this mate, the new pos, the new number of CIGAR operations, the new tlen, the verdict bits (NGSQC_CLIP_V_*; REWRITTEN: this mate was clipped). A record
 * that is written as it is shows its own fields. cap_records: the rows plan holds; NGSQC_E_ARG when the file has more records. */
int ngsqc_clip_overlap_plan(ngsqc_handle* h, int32_t mode_bits, int32_t ignore_indels, int32_t* plan /* [cap_records][6] */, int64_t cap_records, ngsqc_clip_error* err);

/* ---- BamToFastq (src/BamToFastq/main.cpp:77-214): the records of the handle in file order, secondary and supplementary records skipped; with remove_duplicates
 * the duplicates skipped and counted; with fix a record whose (name, read 1) pair came earlier in the file dropped and counted (the set of seen pairs lives in
 * device memory for the whole run). Paired-end mode (out2 not NULL and not ""): unpaired records are skipped and counted, the others are joined by read name
 * (the mate cache); a pair goes out when its second record comes, the read-1 record to out1, the other to out2. Single-end mode: every record to out1.
 * An entry is "@name\nBASES\n+\nQUALS\n" as gzputs writes it (a quality byte of 0 ends its line); a reverse-strand record is reverse-complemented; extend > 0
 * pads with 'N' / '#' to that length. Both files are BGZF (valid gzip) at the given compression level (0-9), ending with the EOF member.
 * reg_tid >= 0: only the records htslib's iterator returns for (reg_tid, reg_start, reg_end), 1-based closed (a handle from ngsqc_open_regions, or the whole
 * file). A handle on a shard or a range without a region is NGSQC_E_ARG. A reverse-strand record that would be written and holds a base other than ACGTN:
 * NGSQC_E_FORMAT "Could not convert base 'X' to complement!" for the first such entry in output order. max_cached: the largest number of open names. */
typedef struct { int32_t remove_duplicates, fix, extend, compression_level; int32_t reg_tid, reg_start, reg_end; } ngsqc_fastq_params;
typedef struct { int64_t paired, unpaired, unmatched, single_end, duplicates, fixed, max_cached; } ngsqc_fastq_counts;
int ngsqc_bam_to_fastq(ngsqc_handle* h, const ngsqc_fastq_params* p, const char* out1, const char* out2, ngsqc_fastq_counts* c);

/* ---- writing the index. The reference never builds one: every indexed path above fails with "Could not load index of BAM/CRAM file"
 * (BamReader.cpp:742-746) until `samtools index` (htslib sam_index_build: hts_idx_push / hts_idx_finish / compress_binning, hts.c) has left a
 * <bam>.bai next to the BAM. ngsqc_write_bai writes that file (bai_path NULL: <path of the handle>.bai) from a handle on the whole BAM: one pass
 * over the tiles (bin, 16 kb windows and run boundaries per record on the device), then htslib's chunk rules on the host. Same bins, chunks, linear
 * index, pseudo-bins and n_no_coor as htslib (pinned on the reference's fixture indices through oracle/bai_build.py); the order of the bins inside a
 * reference is ascending instead of htslib's hash order. NGSQC_E_FORMAT for a BAM that is not sorted by coordinate or reaches behind 2^29 (BAI limit). */
int ngsqc_write_bai(ngsqc_handle* h, const char* bai_path);
/* The CSI form of the same index (hts-specs CSIv1; `samtools index -c -m min_shift`, htslib sam_index_build3 with min_shift > 0): the binning scheme of BAI
 * with min_shift as given (<= 0: 14; 8 .. 30) and depth = the smallest n with longest reference + 256 <= 2^(min_shift + 3 n), loff per bin (the linear
 * index at the bin's first window) in place of the linear index, inside a BGZF container. csi_path NULL: <path of the handle>.csi. Every indexed entry
 * point above takes <bam>.csi before <bam>.bai, as sam_index_load (BamReader.cpp:742) does. The reference holds no .csi fixture: pinned through
 * oracle/csi_build.py, which at BAI's geometry must reproduce the htslib-written .bai fixtures' bins, chunks and (as loff) linear index. */
int ngsqc_write_csi(ngsqc_handle* h, const char* csi_path, int32_t min_shift);
/* The host half alone (several shards' runs merged by the caller; tests): runs = consecutive records of one (reference, bin) in file order, each with the
 * virtual offset of its first record (kind 0; kind 1 entries - "last record of a tile", pos clamped at 0 - only feed the sort check), lidx = first
 * virtual offset per 16 kb window (~0: none) for the windows [lidx_first[t], lidx_first[t + 1]) of reference t, counts = (mapped, unmapped) per reference
 * followed by the pair of the reads without reference. */
typedef struct ngsqc_bai_run { uint64_t voff; int32_t tid; uint32_t bin; int32_t pos; uint32_t kind; } ngsqc_bai_run;
int ngsqc_bai_assemble(const char* bai_path, int32_t n_ref, uint64_t first_record_voff, uint64_t end_voff, const ngsqc_bai_run* runs, int64_t n_runs,
                       const uint64_t* lidx, const int64_t* lidx_first, const int64_t* counts);
/* the same for a CSI index: bins of the runs and windows of lidx in the geometry (min_shift, depth) */
int ngsqc_csi_assemble(const char* csi_path, int32_t min_shift, int32_t depth, int32_t n_ref, uint64_t first_record_voff, uint64_t end_voff, const ngsqc_bai_run* runs, int64_t n_runs,
                       const uint64_t* lidx, const int64_t* lidx_first, const int64_t* counts);

typedef struct ngsqc_shard_summary {
	int64_t n_records;         /* records owned by the shard */
	int64_t first_abs;         /* inflated-stream offset (whole file) of the first record owned; -1: the shard owns no record (none starts in its own members) */
	int64_t exit_abs;          /* offset of the first record behind the shard (= the first_abs of the next shard that owns one); -1 with first_abs */
	int64_t max_len;           /* longest l_seq among counted (not secondary / supplementary) records, 0 = none */
	int64_t first_max_ord;     /* shard-local ordinal of the first counted record of that length, -1 = none */
	int64_t first_paired_ord;  /* shard-local ordinal of the first record that sets paired_end, -1 = none */
} ngsqc_shard_summary;
typedef struct ngsqc_shard_fix {
	int64_t gmax;              /* max over shards of max_len */
	int64_t floor_max;         /* max of max_len over EARLIER shards (running maximum carried into this shard) */
	int64_t trim_upto;         /* local ordinals [0, trim_upto) precede the BAM's first record of length gmax */
	int64_t paired_upto;       /* local ordinals [0, paired_upto) precede the BAM's first paired record */
	int32_t paired_end;        /* some shard saw a paired read */
	int32_t reserved;
} ngsqc_shard_fix;
int ngsqc_scan_mapping_partial(ngsqc_handle* h, const ngsqc_mapping_params* p, ngsqc_shard_summary* out);
/* the fused job of a shard (what MappingQC runs on one BAM, src/MappingQC/main.cpp:100-151): the mapping scan in shard form (job->mapping is required;
 * summary in *out, counters later from ngsqc_scan_mapping_finish), the extra depth scan without its prefix sum, the site pileup (result->site_counts:
 * additive over shards). Every BGZF member of the shard is inflated once for all consumers; the shard's first records are kept in the form the
 * cross-shard fix-ups need, so ngsqc_scan_mapping_finish does not inflate anything again. read_qc is not available on shards. */
int ngsqc_run_job_partial(ngsqc_handle* h, const ngsqc_job_desc* job, ngsqc_job_result* result, ngsqc_shard_summary* out);
/* coverage tools on a shard: ngsqc_scan_depth without the final prefix sum (the depth scan has no order-dependent carries). No summary is exchanged: the
 * shards' chains are checked where their arrays meet, in ngsqc_depth_reduce */
int ngsqc_scan_depth_partial(ngsqc_handle* h, const ngsqc_depth_params* p);
/* returns NGSQC_E_FORMAT (message via ngsqc_last_error(NULL)) when the shards' record chains do not join */
int ngsqc_plan_shard_fix(const ngsqc_shard_summary* all, int n_shards, int shard, ngsqc_shard_fix* out);
int ngsqc_scan_mapping_finish(ngsqc_handle* h, const ngsqc_shard_fix* fix, int64_t* counters, double* gc_reads);
/* the un-prefixed difference array (int32[n_slots], device memory owned by the handle) for an in-place SUM all-reduce */
int ngsqc_depth_device(ngsqc_handle* h, void** dev_ptr, int64_t* n_slots);
int ngsqc_depth_diff_copy(ngsqc_handle* h, int32_t* out, int64_t cap);       /* host copy of the same array (CPU collectives) */
int ngsqc_depth_diff_set(ngsqc_handle* h, const int32_t* in, int64_t n);
/* dst's difference array += the arrays of the other shard handles; arrays on other GPUs are pulled with peer copies over xGMI
 * (no host staging). All handles must have scanned the same regions with ngsqc_scan_*_partial. The shard handles among dst and srcs are held to the
 * chain rule of ngsqc_plan_shard_fix, in the order of their shard index: NGSQC_E_FORMAT (same message, on dst) when their record chains do not join,
 * and nothing is added. */
int ngsqc_depth_reduce(ngsqc_handle* dst, ngsqc_handle* const* srcs, int n_srcs);
int ngsqc_depth_finalize(ngsqc_handle* h);                                    /* difference array -> per-base depth (K6 prefix sum) */

/* ---- the collective of the multi-GPU path: RCCL over xGMI, one process per GPU (round 4; BASELINE.json north_star: "only a final RCCL reduce of the
 * counter vectors"). The reference is a single process and has no counterpart (its parallelism: Statistics.cpp:2614-2638).
 * Rank 0 makes a unique id and hands it to the other ranks out of band (a file, MPI, the launcher's store); every rank then makes its communicator on its
 * own device. The calls are collective: every rank of the communicator must make them in the same order. librccl is loaded by the first of these calls.
 *   one BAM per GPU (config 4): ngsqc_run_job on every rank -> ngsqc_comm_allreduce_counters (and _i64 for site counts, _f64 for gc_reads)
 *   one BAM over the GPUs     : ngsqc_run_job_partial -> ngsqc_comm_allgather_summaries -> ngsqc_plan_shard_fix -> ngsqc_scan_mapping_finish ->
 *                               ngsqc_comm_allreduce_counters / _f64 / _i64 -> ngsqc_comm_allreduce_depth (in place, device memory) -> ngsqc_depth_finalize */
#define NGSQC_COMM_ID_BYTES 128
typedef struct ngsqc_comm ngsqc_comm;
int ngsqc_comm_unique_id(void* id /* NGSQC_COMM_ID_BYTES, out */);
int ngsqc_comm_init(int rank, int world, const void* id, int device, ngsqc_comm** out);
int ngsqc_comm_rank(const ngsqc_comm* c);
int ngsqc_comm_world(const ngsqc_comm* c);
const char* ngsqc_comm_last_error(const ngsqc_comm* c);
int ngsqc_comm_destroy(ngsqc_comm* c);
/* int64[NGSQC_NCOUNTERS] on the host, in place: SUM; MAX for max_length, paired_end, roi_bases, half_depth, yx_valid */
int ngsqc_comm_allreduce_counters(ngsqc_comm* c, int64_t* counters);
int ngsqc_comm_allreduce_i64(ngsqc_comm* c, int64_t* v, int64_t n, int take_max);   /* host vector in place: SUM (take_max = 0) or MAX */
int ngsqc_comm_allreduce_f64(ngsqc_comm* c, double* v, int64_t n);                  /* host vector in place: SUM (gc_reads) */
int ngsqc_comm_allgather_summaries(ngsqc_comm* c, const ngsqc_shard_summary* mine, ngsqc_shard_summary* all /* [world], rank order */);
int ngsqc_comm_allreduce_depth(ngsqc_comm* c, ngsqc_handle* h);                     /* the handle's int32 difference array, in place on the device */

/* ---- measurement: HIP-event timings (ms) of the stages of the last job on this handle ---- */
typedef struct ngsqc_timings {
	double h2d_ms, inflate_ms, index_ms, scan_ms, finalize_ms, total_ms;
	int64_t inflate_launches, scan_launches;
	int64_t scan_algorithmic_bytes;   /* sum over records of (4 + block_size)  — SURVEY.md §8(d) */
	int64_t compressed_bytes, inflated_bytes, n_records;
	double scan_kernel_ms;            /* K3-K5 kernels only (HIP events around the scan launches on the handle's stream) */
	double depth_kernel_ms;           /* K6 prefix sum + histogram kernels */
	double inflate_huff_ms;           /* K1 phase 1: huff_tokens_kernel, sum over its launches (0 when the group kernel ran) */
	double inflate_lz77_ms;           /* K1 phase 2: lz77 resolve kernel (sum over its launches; overlaps phase 1 of the next member chunk) */
	int64_t inflate_huff_launches;    /* K1 phase-1 launches of the last decode (member chunks of one "round" of decoder lanes) */
	/* tile stream (round 2): stage times are sums of HIP-event intervals on the handle's main stream; with more than one tile
	 * they overlap K1 of the next tile, so their sum exceeds the job's wall time */
	int64_t n_tiles;                  /* tiles of the handle's member table */
	int64_t members_inflated;         /* BGZF members that went through K1 during the last job (== members of the tiles visited) */
	double depth_scan_ms;             /* the extra depth scan of a job */
	double pileup_ms, reads_ms;       /* site pileup (+ the indel windows of ngsqc_indel_windows / ngsqc_variant_details) / raw-read QC consumers */
	double job_wall_ms;               /* host wall time of the last ngsqc_run_job (setup, all tiles, result copies) */
	int64_t members_second_chance;    /* members whose launch ran out of token pages and that were inflated again with the worst-case pool (since the handle was opened) */
	int64_t members_third_chance;     /* ... and again with the bound that holds for every valid member (members of thousands of DEFLATE blocks) */
	/* record index (round 5): how the tiles of the last decode found their record chains */
	int64_t tiles_chain_on_device;    /* tiles whose chain passed the check on the device (every walker's exit = the next walker's start): no host verification */
	int64_t tiles_scan_fused;         /* ... of which the job's mapping / depth scan rode the chain walk (one read of every record's first line) */
	int64_t walkers_per_member;       /* walkers per BGZF member of the last tile's fast path (NGSQC_WALKERS) */
	/* round 6: the state of the switches that can change a RESULT (all others only change a schedule). NGSQC_SW_* bits; the defaults are NGSQC_SW_VERIFY_CRC alone */
	int64_t switches;
} ngsqc_timings;
#define NGSQC_SW_VERIFY_CRC        1   /* every member's CRC32 is checked against its gzip trailer (NGSQC_VERIFY_CRC=0 turns it off: a measurement switch) */
#define NGSQC_SW_CRAM_IGNORE_MD5   2   /* NGSQC_CRAM_IGNORE_MD5=1: a slice's reference MD5 is not compared (htslib's ignore_md5 option) */
#define NGSQC_SW_CRAM_NO_REFERENCE 4   /* NGSQC_CRAM_NO_REFERENCE=1: bases that come from the genome are N (the reference's skipBases mode; test switch) */
/* The struct grows at its END from round to round and this call writes sizeof(ngsqc_timings) of the LIBRARY: a caller compiled against an older header must be
 * rebuilt - or call ngsqc_get_timings_sized with ITS sizeof: at most that many bytes are written (the fields it knows). ngsqc_abi_version() is the round of the
 * header the library was built from (6). */
int ngsqc_get_timings(const ngsqc_handle* h, ngsqc_timings* t);
int ngsqc_get_timings_sized(const ngsqc_handle* h, void* t, size_t struct_size);
int32_t ngsqc_abi_version(void);

/* library / device info string (static storage) */
const char* ngsqc_version(void);

/* Number of HIP devices this process sees (0 when there is none or the runtime cannot start; never an error): what a caller that opens one handle per device -
 * the reference's per-sample loop of src/MappingQC/main.cpp:60-67 spread over a node, SURVEY.md 8(e) - sizes its rank list with. */
int32_t ngsqc_device_count(void);

#ifdef __cplusplus
}
#endif
#endif /* NGSQC_H */
