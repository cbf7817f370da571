// BamToFastq's per-entry text under the emulator as a stand-alone program, so that it can be built with -fsanitize=address,undefined and run on its own
// (tests/test_cpu_tofastq_designed.py). Usage: tofastq_emul_main RECS OFFS EXTEND DENSE
// RECS: the records end to end; OFFS: int64[n + 1]. Every record is copied into a heap buffer of exactly its size and its entry written into one of exactly
// the size the info word announces, so a read outside the record or a write behind the entry ends the run. Prints size, throws and the entry's FNV-1a per
// record, then the verdict of the range splits against the entry fq_byte gave.
#include "tofastq_emul.cpp"
#include <cinttypes>
#include <cstdio>
#include <cstdlib>

static std::vector<uint8_t> slurp(const char* path)
{
	FILE* f = fopen(path, "rb");
	if (!f) { perror(path); exit(2); }
	std::vector<uint8_t> v; uint8_t buf[65536]; size_t k;
	while ((k = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + k);
	fclose(f);
	v.shrink_to_fit();
	return v;
}

int main(int argc, char** argv)
{
	if (argc != 5) { fprintf(stderr, "usage: %s RECS OFFS EXTEND DENSE\n", argv[0]); return 2; }
	const std::vector<uint8_t> recs = slurp(argv[1]), offs = slurp(argv[2]);
	const int32_t extend = atoi(argv[3]), dense = atoi(argv[4]);
	const int64_t n = (int64_t)offs.size() / 8 - 1;
	std::vector<int64_t> recoff(n + 1); memcpy(recoff.data(), offs.data(), 8 * (size_t)(n + 1));
	for (int64_t i = 0; i < n; ++i)
	{
		const std::vector<uint8_t> rec(recs.begin() + recoff[i], recs.begin() + recoff[i + 1]);
		const int64_t zero = 0; uint32_t info; uint8_t inr; int64_t endpos;
		tofastq_info(rec.data(), &zero, 1, extend, -1, 0, 0, &info, &inr, &endpos);
		const uint32_t size = info & INFO_SIZE;
		std::vector<uint8_t> entry(size);
		tofastq_entry(rec.data(), size, extend, entry.data());
		uint64_t h = 0xcbf29ce484222325ull;
		for (uint8_t c : entry) h = (h ^ c) * 0x100000001b3ull;
		const int64_t bad = tofastq_splits(rec.data(), size, extend, entry.data(), dense);
		printf("%" PRId64 " size %u throws %d entry %016" PRIx64 " splits %" PRId64 "\n", i, size, (info & INFO_THROWS) ? 1 : 0, h, bad);
		if (bad != -1) return 3;
	}
	return 0;
}
