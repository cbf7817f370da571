"""ngs-bits_amd — MI355X-native BAM mapping-QC / coverage hot path (drop-in for one path of imgag/ngs-bits).

The product is the C-ABI library libngsqc_hip.so (include/ngsqc.h) built from csrc/*.hip plus the C++ host tools under
host/. This Python package is only a thin ctypes binding used by tests/ and bench.py; it fails loudly if the HIP
library has not been built (there is no CPU fallback).
"""
from .capi import (  # noqa: F401
    NgsqcError, Handle, Region, MappingParams, lib, lib_path, build_library,
    MODE_ROI, MODE_NOROI, MODE_WGS, NCOUNTERS, COUNTER_NAMES, ShardSummary, ShardFix, SUMMARY_FIELDS, plan_shard_fix, bai_range, bai_ranges, set_reference, set_cram_skip, set_cram_skip_thread, CRAM_SKIP_NAMES, CRAM_SKIP_TAGS, cram_to_bam, bai_assemble, bgzf_scan, Comm, device_count,
    IndelWindow, VariantParams, ALLELE_NONE, ALLELE_INS, ALLELE_DEL, INDEL_COUNTER_NAMES,
    PairFilter, bgzf_compress, FastqParams, FastqCounts, FASTQ_COUNT_NAMES,
    DownsampleParams, DownsampleCounts, DOWNSAMPLE_COUNT_NAMES, DOWNSAMPLE_CHUNK, downsample_keep,
    ExtractCounts, EXTRACT_COUNT_NAMES, HaloplexCounts, HALOPLEX_COUNT_NAMES,
    RmVariant, RmParams, RmCounts, RM_COUNT_NAMES, RMVAR_SNV, RMVAR_OTHER, RMVAR_INVALID, RMERR_NONE, RMERR_INVALID_LINE, RMERR_POS_NOT_FOUND, RMERR_BAD_BASE,
    ClipError, CLIP_MAPQ, CLIP_REMOVE, CLIP_BASEQ, CLIP_BASEN, CLIP_COUNT_NAMES, CLIP_PLAN_COLUMNS, CLIPERR_NONE, CLIPERR_ORIENT, CLIPERR_CIGAR_CHAR, CLIPERR_LENGTH, CLIPERR_SC_ORDER,
    CLIPERR_SC_START, CLIPERR_SC_END, CLIPERR_SC_INDEX, CLIPERR_SC_OP, CLIPERR_BAD_BASE, CLIPERR_UNSUPPORTED,
    FastqStats, FastqReport, Purge, PurgeParams, PurgeStats, purge_plan, PURGE_PLAN_COLUMNS,
    FastqEdit, FqEditParams, FqEditStats, fastq_edit_plan, FQEDIT_PLAN_COLUMNS, FQEDIT_OPS, FQEDIT_SHAPE,
)
from .dist import allreduce_counters, combine_counters_local, shard_blocks, scan_mapping_sharded, scan_mapping_sharded_local, scan_depth_sharded_local  # noqa: F401,E402
