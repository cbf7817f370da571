// The host's view of FASTQ text (ngs-bits_amd/csrc/fastq_text.h: where a text ends, the lines of an entry from the device's line offsets, the messages of
// FastqEntry::validate) as a stand-alone program, so that it can be built with -fsanitize=address,undefined and run on its own
// (tests/test_cpu_seqpurge_emul.py). Usage: fastq_text_main LONG_READ TEXT...
// Every TEXT is a file read as the last piece of a file: a missing final newline is added, the empty lines at the end are stripped, and the text lies in a heap
// buffer of exactly the stripped size. The line offsets the device would give come from a byte loop; every entry gets exactly the offsets the host would fetch
// for it. Prints, per text: "text STRIPPED_AS_FED STRIPPED LINES", then per entry "entry R KIND" and five lines in hex: the four lines of the entry and the
// message (empty unless KIND is 1 .. 5). KIND is what the kernels' text (fastq_visit.h) says about the entry, whose lines must be the host's.
#include "../../ngs-bits_amd/csrc/fastq_text.h"
#include <cstdio>
#include <cstdlib>

using namespace ngsqc;

static std::vector<uint8_t> slurp(const char* path)
{
	FILE* f = fopen(path, "rb");
	if (!f) { perror(path); exit(2); }
	std::vector<uint8_t> v; uint8_t buf[65536]; size_t k;
	while ((k = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + k);
	fclose(f);
	return v;
}
static void put_hex(const std::string& s) { for (unsigned char c : s) printf("%02x", c); printf("\n"); }

int main(int argc, char** argv)
{
	if (argc < 2) { fprintf(stderr, "usage: %s LONG_READ TEXT...\n", argv[0]); return 2; }
	const int long_read = atoi(argv[1]);
	for (int f = 2; f < argc; ++f)
	{
		std::vector<uint8_t> fed = slurp(argv[f]);
		const size_t as_fed = fq_strip_empty_lines(fed.data(), fed.size());   // (in the middle of a file: what would be indexed, the rest waits)
		if (!fed.empty() && fed.back() != '\n') fed.push_back('\n');
		const size_t n = fq_strip_empty_lines(fed.data(), fed.size());
		uint8_t* text = (uint8_t*)malloc(n ? n : 1);                          // exactly the indexed bytes
		for (size_t i = 0; i < n; ++i) text[i] = fed[i];
		uint64_t L = 0;
		for (size_t i = 0; i < n; ++i) L += text[i] == '\n';
		uint32_t* lines = (uint32_t*)malloc((L + 1) * sizeof(uint32_t));     // ... and exactly lines[0 .. L]
		lines[0] = 0; L = 0;
		for (size_t i = 0; i < n; ++i) if (text[i] == '\n') lines[++L] = (uint32_t)i + 1;
		const uint64_t E = (L + 3) / 4;
		printf("text %zu %zu %llu\n", as_fed, n, (unsigned long long)L);
		for (uint64_t r = 0; r < E; ++r)
		{
			const std::vector<uint32_t> lo(lines + 4 * r, lines + 4 * r + fq_entry_offsets(r, L));
			std::string ln[4]; fq_entry_lines(text, lo, ln);
			const FqEntry e = fq_entry(text, lines, L, r);
			const FqLine dev[4] = {e.header, e.bases, e.header2, e.quals};
			for (int k = 0; k < 4; ++k)
				if (ln[k] != std::string((const char*)text + dev[k].start, dev[k].len)) { fprintf(stderr, "entry %llu line %d: the host's line is not the device's\n", (unsigned long long)r, k); return 3; }
			uint32_t kind = fq_entry_kind(text, e);
			if (!kind)
			{
				bool bb = false, bq = false;
				for (uint32_t i = 0; i < e.bases.len; ++i) { const FqChar c = fq_char(text[e.bases.start + i], text[e.quals.start + i], long_read); bb |= c.cls == 5; bq |= !c.ok; }
				kind = fq_char_kind(e.header.len == 0, bb, bq);
			}
			printf("entry %llu %u\n", (unsigned long long)r, kind);
			for (int k = 0; k < 4; ++k) put_hex(ln[k]);
			put_hex(kind >= FQ_ERR_HEADER && kind <= FQ_ERR_QUALITY ? fq_validate_message((int)kind, ln, long_read) : std::string());
		}
		free(text); free(lines);
	}
	return 0;
}
