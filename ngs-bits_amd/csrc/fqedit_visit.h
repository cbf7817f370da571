// One FASTQ entry as the per-entry FASTQ-to-FASTQ tools see it (src/FastqTrim/main.cpp:47-73, src/FastqConvert/main.cpp:33-41, src/FastqExtract/main.cpp:61-90,
// src/FastqExtractUMI/main.cpp:48-74): the plan record of an entry for each tool, the id of a header, validation as FastqExtract's stream does it, the bytes an
// entry gives its output stream and byte k of them, the UMI text included - the text csrc/fqedit.hip compiles into its kernels, kept free of HIP so that
// tests/emul/fqedit_emul.cpp runs the same text on the CPU against the Python model (tests/fqedit_oracle.py). Plain integer code.
// The same for src/FastqExtractBarcode/main.cpp:44-60, src/FastqAddBarcode/main.cpp:50-72, src/FastqDownsample/main.cpp:58-71 and src/FastqConcat/main.cpp:46-50
// (tests/emul/fqedit2_emul.cpp, tests/fqedit2_oracle.py): there an output stream is no longer the input side of the same number - fe_shape says which side
// every stream of an operation reads.
#pragma once
#include "fastq_visit.h"

namespace ngsqc {
namespace {
constexpr int FE_PLAN = 8;   // int32 per entry and stream (include/ngsqc.h)
enum { FE_KEEP = 0, FE_INS_AT = 1, FE_INS_LEN = 2, FE_B_OFF = 3, FE_B_LEN = 4, FE_Q_OFF = 5, FE_Q_LEN = 6, FE_QDELTA = 7 };
enum { FE_OP_TRIM = 0, FE_OP_EXTRACT = 1, FE_OP_UMI = 2, FE_OP_CONVERT = 3, FE_OP_BARCODE_CUT = 4, FE_OP_BARCODE_ADD = 5, FE_OP_DOWNSAMPLE = 6, FE_OP_COPY = 7, FE_N_OPS = 8 };
constexpr int FE_MAX_SIDES = 3, FE_MAX_STREAMS = 2;
// the table of the operations: input sides, output streams, and the side stream k takes its entries from
struct FeShape { int sides, streams, src[FE_MAX_STREAMS]; };
FQ_DEV FeShape fe_shape(int op)
{
	switch (op)
	{
	case FE_OP_UMI: case FE_OP_DOWNSAMPLE: return FeShape{2, 2, {0, 1}};
	case FE_OP_BARCODE_CUT: return FeShape{1, 2, {0, 0}};   // main and index, both from the one input
	case FE_OP_BARCODE_ADD: return FeShape{3, 2, {0, 1}};   // the third side is only read for its bases
	default: return FeShape{1, 1, {0, 0}};
	}
}
constexpr int32_t FE_NO_LENGTH = -1, FE_ABSENT = -2;   // the sentinels of FastqExtract (main.cpp:46, :69)

struct FeParams { int op, long_read, start, end, len, max_len, cut1, cut2, invert; };

// the entry as it is: every tool starts here. A dropped entry keeps these ranges and has keep = 0.
FQ_DEV void fe_plan_whole(int32_t* row, uint32_t bl, uint32_t ql)
{
	row[FE_KEEP] = 1; row[FE_INS_AT] = 0; row[FE_INS_LEN] = 0; row[FE_B_OFF] = 0; row[FE_B_LEN] = (int32_t)bl; row[FE_Q_OFF] = 0; row[FE_Q_LEN] = (int32_t)ql; row[FE_QDELTA] = 0;
}
// FastqTrim (main.cpp:52-70); start, end, len, max_len >= 0. The qualities take the range of the bases (QByteArray::mid clips it to the line); no line grows.
FQ_DEV void fe_plan_trim(int32_t* row, const FeParams& P, uint32_t bl, uint32_t ql)
{
	fe_plan_whole(row, bl, ql);
	if (P.max_len > 0 && (int64_t)bl >= P.max_len) return;
	int64_t bo = 0, bn = bl, qo = 0, qn = ql;
	if (P.start > 0 || P.end > 0)
	{
		if ((int64_t)bl <= (int64_t)P.start + P.end) { row[FE_KEEP] = 0; return; }
		bo = P.start; bn = (int64_t)bl - P.start - P.end;
		qo = P.start < (int64_t)ql ? P.start : (int64_t)ql;
		qn = bn < (int64_t)ql - qo ? bn : (int64_t)ql - qo;
	}
	if (P.len > 0 && bn > P.len) { bn = P.len; qn = qn < P.len ? qn : P.len; }
	row[FE_B_OFF] = (int32_t)bo; row[FE_B_LEN] = (int32_t)bn; row[FE_Q_OFF] = (int32_t)qo; row[FE_Q_LEN] = (int32_t)qn;
}
// FastqConvert (main.cpp:36-39): every quality byte - 31, byte arithmetic
FQ_DEV void fe_plan_convert(int32_t* row, uint32_t bl, uint32_t ql) { fe_plan_whole(row, bl, ql); row[FE_QDELTA] = -31; }

// FastqExtract (main.cpp:69-89): payload = the id's length column, FE_NO_LENGTH without one, FE_ABSENT when the id is not listed
FQ_DEV void fe_plan_extract(int32_t* row, int32_t payload, int invert, uint32_t bl, uint32_t ql)
{
	fe_plan_whole(row, bl, ql);
	if (payload == FE_ABSENT) { row[FE_KEEP] = invert ? 1 : 0; return; }
	if (payload == FE_NO_LENGTH) { row[FE_KEEP] = invert ? 0 : 1; return; }
	if (payload < 1 || invert) { row[FE_KEEP] = 0; return; }
	if ((uint32_t)payload < bl) row[FE_B_LEN] = payload;   // (a length beyond the read keeps the whole read: FastqExtract_out4)
	if ((uint32_t)payload < ql) row[FE_Q_LEN] = payload;
}
// FastqExtractBarcode (main.cpp:50-56): the main stream loses the first cut bytes of both lines, the index stream is those bytes; each line is cut on its
// own, and where QByteArray(read1.bases, cut) would read behind a shorter line the bytes that exist are taken (as for the UMI of a short read)
FQ_DEV void fe_plan_barcode_main(int32_t* row, uint32_t cut, uint32_t bl, uint32_t ql)
{
	fe_plan_whole(row, bl, ql);
	const uint32_t bo = cut < bl ? cut : bl, qo = cut < ql ? cut : ql;
	row[FE_B_OFF] = (int32_t)bo; row[FE_B_LEN] = (int32_t)(bl - bo); row[FE_Q_OFF] = (int32_t)qo; row[FE_Q_LEN] = (int32_t)(ql - qo);
}
FQ_DEV void fe_plan_barcode_index(int32_t* row, uint32_t cut, uint32_t bl, uint32_t ql)
{
	fe_plan_whole(row, bl, ql);
	row[FE_B_LEN] = (int32_t)(cut < bl ? cut : bl); row[FE_Q_LEN] = (int32_t)(cut < ql ? cut : ql);
}
// FastqDownsample (main.cpp:64-70) and FastqConcat (main.cpp:48-49): the entry as it is, written when the decision says so (FastqConcat: always)
FQ_DEV void fe_plan_keep(int32_t* row, uint32_t keep, uint32_t bl, uint32_t ql) { fe_plan_whole(row, bl, ql); row[FE_KEEP] = keep ? 1 : 0; }
FQ_DEV bool fe_is_space(uint32_t c) { return c == ' ' || (c >= 9u && c <= 13u); }   // QByteArray::trimmed
// the id of a header (main.cpp:65-68): the trimmed header without its first byte, up to the first space. [start, start + len) of the text.
FQ_DEV void fe_id_range(const uint8_t* text, const FqLine& h, uint32_t& start, uint32_t& len)
{
	uint32_t a = h.start, b = h.start + h.len;
	while (a < b && fe_is_space(text[a])) ++a;
	while (b > a && fe_is_space(text[b - 1])) --b;
	if (a < b) ++a;
	uint32_t e = a;
	while (e < b && text[e] != ' ') ++e;
	start = a; len = e - a;
}
// FastqFileStream::readEntry with auto_validate (FastqFileStream.cpp:151-157): an entry with an empty header is not validated. The first three checks:
FQ_DEV uint32_t fe_entry_kind(const uint8_t* text, const FqEntry& e) { return e.header.len ? fq_entry_kind(text, e) : (uint32_t)FQ_OK; }
// ... and one cycle of the last two (both lines have one length then): bit 0 a base outside ACGTN, bit 1 a quality out of range
FQ_DEV uint32_t fe_cycle_bad(uint32_t base_c, uint32_t qual_c, int long_read) { return (fq_base_class(base_c) == 5u ? 1u : 0u) | (fq_quality_ok(qual_c, long_read) ? 0u : 2u); }

// FastqExtractUMI (main.cpp:55-70): the text ":" cut1 "," cut2 ":" umi1 "," umi2 goes behind the first space-delimited token of both headers; umi k = the
// first cut k bases of read k, or the bases there are
FQ_DEV uint32_t fe_digits(uint32_t v) { uint32_t d = 1; while (v >= 10u) { v /= 10u; ++d; } return d; }
FQ_DEV uint8_t fe_digit(uint32_t v, uint32_t d, uint32_t k) { for (uint32_t i = k + 1; i < d; ++i) v /= 10u; return (uint8_t)('0' + v % 10u); }   // digit k of d, from the left
struct FeUmi { const uint8_t* b1; const uint8_t* b2; uint32_t u1, u2, cut1, cut2; };
FQ_DEV uint32_t fe_umi_len(const FeUmi& u) { return 4u + fe_digits(u.cut1) + fe_digits(u.cut2) + u.u1 + u.u2; }
FQ_DEV uint8_t fe_umi_byte(const FeUmi& u, uint32_t j)
{
	const uint32_t d1 = fe_digits(u.cut1), d2 = fe_digits(u.cut2);
	if (j == 0) return ':';
	j -= 1;
	if (j < d1) return fe_digit(u.cut1, d1, j);
	if (j == d1) return ',';
	j -= d1 + 1;
	if (j < d2) return fe_digit(u.cut2, d2, j);
	if (j == d2) return ':';
	j -= d2 + 1;
	if (j < u.u1) return u.b1[j];
	if (j == u.u1) return ',';
	return u.b2[j - u.u1 - 1];
}
FQ_DEV FeUmi fe_umi_of(const uint8_t* text1, const FqEntry& e1, const uint8_t* text2, const FqEntry& e2, int cut1, int cut2)
{
	FeUmi u; u.b1 = text1 + e1.bases.start; u.b2 = text2 + e2.bases.start; u.cut1 = (uint32_t)cut1; u.cut2 = (uint32_t)cut2;
	u.u1 = u.cut1 < e1.bases.len ? u.cut1 : e1.bases.len; u.u2 = u.cut2 < e2.bases.len ? u.cut2 : e2.bases.len;
	return u;
}
// FastqAddBarcode (main.cpp:59-68): the text ":" len3 ",0:" bases3 "," goes behind the first space-delimited token of both headers; bases3 = the bases line of
// the barcode read, len3 its length: 5 bytes, the digits of len3 and the bases
FQ_DEV uint32_t fe_addbarcode_len(uint32_t len3) { return 5u + fe_digits(len3) + len3; }
FQ_DEV uint8_t fe_addbarcode_byte(const uint8_t* b3, uint32_t len3, uint32_t j)
{
	const uint32_t d = fe_digits(len3);
	if (j == 0) return ':';
	j -= 1;
	if (j < d) return fe_digit(len3, d, j);
	j -= d;
	if (j < 3) return j == 0 ? ',' : j == 1 ? '0' : ':';
	j -= 3;
	return j < len3 ? b3[j] : (uint8_t)',';
}
// what the format kernel splices into a header: nothing, the UMI text of a pair, or the barcode text of a third read
enum { FE_INS_NONE = 0, FE_INS_UMI = 1, FE_INS_BARCODE = 2 };
struct FeIns { int kind; FeUmi u; const uint8_t* b3; uint32_t len3; };
FQ_DEV FeIns fe_ins_umi(const FeUmi& u) { FeIns i{}; i.kind = FE_INS_UMI; i.u = u; return i; }
FQ_DEV FeIns fe_ins_barcode(const uint8_t* text3, const FqEntry& e3) { FeIns i{}; i.kind = FE_INS_BARCODE; i.b3 = text3 + e3.bases.start; i.len3 = e3.bases.len; return i; }
FQ_DEV uint8_t fe_ins_byte(const FeIns& i, uint32_t j) { return i.kind == FE_INS_BARCODE ? fe_addbarcode_byte(i.b3, i.len3, j) : fe_umi_byte(i.u, j); }
// one read of FastqAddBarcode: the lines stay, ins_len bytes come in behind the header's first token (the header's first space, or its end)
FQ_DEV void fe_plan_addbarcode(int32_t* row, const uint8_t* text, const FqEntry& e, uint32_t len3)
{
	fe_plan_whole(row, e.bases.len, e.quals.len);
	uint32_t at = 0;
	while (at < e.header.len && text[e.header.start + at] != ' ') ++at;
	row[FE_INS_AT] = (int32_t)at; row[FE_INS_LEN] = (int32_t)fe_addbarcode_len(len3);
}
// one read of a pair: the first cut bytes of both lines go (a shorter line becomes empty), ins_len bytes come in behind the header's first token
FQ_DEV void fe_plan_umi(int32_t* row, const uint8_t* text, const FqEntry& e, uint32_t cut, uint32_t ins_len)
{
	fe_plan_whole(row, e.bases.len, e.quals.len);
	uint32_t at = 0;
	while (at < e.header.len && text[e.header.start + at] != ' ') ++at;
	const uint32_t bo = cut < e.bases.len ? cut : e.bases.len, qo = cut < e.quals.len ? cut : e.quals.len;
	row[FE_INS_AT] = (int32_t)at; row[FE_INS_LEN] = (int32_t)ins_len;
	row[FE_B_OFF] = (int32_t)bo; row[FE_B_LEN] = (int32_t)(e.bases.len - bo); row[FE_Q_OFF] = (int32_t)qo; row[FE_Q_LEN] = (int32_t)(e.quals.len - qo);
}

// the bytes an entry gives its output stream
FQ_DEV uint64_t fe_entry_bytes(const int32_t* row, const FqEntry& e)
{
	if (!row[FE_KEEP]) return 0;
	return (uint64_t)e.header.len + (uint64_t)row[FE_INS_LEN] + (uint64_t)row[FE_B_LEN] + (uint64_t)e.header2.len + (uint64_t)row[FE_Q_LEN] + 4ull;
}
// byte k of them: the header with the insertion spliced in, the kept bases, line 3 as it is, the kept qualities with the delta added modulo 256
FQ_DEV uint8_t fe_entry_byte(const uint8_t* text, const FqEntry& e, const int32_t* row, uint64_t k, const FeIns& u)
{
	const uint64_t at = (uint64_t)row[FE_INS_AT], il = (uint64_t)row[FE_INS_LEN], hl = (uint64_t)e.header.len + il;
	if (k < hl) return k < at ? text[e.header.start + k] : k < at + il ? fe_ins_byte(u, (uint32_t)(k - at)) : text[e.header.start + (k - il)];
	if (k == hl) return '\n';
	k -= hl + 1;
	const uint64_t bn = (uint64_t)row[FE_B_LEN];
	if (k < bn) return text[e.bases.start + (uint64_t)row[FE_B_OFF] + k];
	if (k == bn) return '\n';
	k -= bn + 1;
	if (k < e.header2.len) return text[e.header2.start + k];
	if (k == e.header2.len) return '\n';
	k -= (uint64_t)e.header2.len + 1;
	const uint64_t qn = (uint64_t)row[FE_Q_LEN];
	return k < qn ? (uint8_t)(text[e.quals.start + (uint64_t)row[FE_Q_OFF] + k] + (uint32_t)row[FE_QDELTA]) : (uint8_t)'\n';
}
// FastqDownsample -test (main.cpp:69): the bytes a pair gives the text of kept headers - the header line of read 1 and a line feed, nothing when dropped - and byte k of them
FQ_DEV uint64_t fe_header_bytes(const int32_t* row, const FqEntry& e) { return row[FE_KEEP] ? (uint64_t)e.header.len + 1ull : 0ull; }
FQ_DEV uint8_t fe_header_byte(const uint8_t* text, const FqEntry& e, uint64_t k) { return k < e.header.len ? text[e.header.start + k] : (uint8_t)'\n'; }
FQ_DEV uint8_t fe_entry_byte(const uint8_t* text, const FqEntry& e, const int32_t* row, uint64_t k, const FeUmi& u) { return fe_entry_byte(text, e, row, k, fe_ins_umi(u)); }
} // namespace
} // namespace ngsqc
