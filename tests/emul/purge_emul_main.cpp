// SeqPurge's per-pair text under the emulator as a stand-alone program, so that it can be built with -fsanitize=address,undefined and run on its own
// (tests/test_cpu_seqpurge_emul.py). Usage: purge_emul_main TEXT1 TEXT2 A1 A2 MIN_LEN QCUT QWIN QOFF NCUT EC OUT3
// TEXT1 / TEXT2: the two FASTQ texts as the accumulator hands them to the device, each read into a heap buffer of exactly its size. Prints the plan, a row
// per pair, and the sizes of the four output texts.
#include "purge_emul.cpp"
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
	if (argc != 12) { fprintf(stderr, "usage: %s TEXT1 TEXT2 A1 A2 MIN_LEN QCUT QWIN QOFF NCUT EC OUT3\n", argv[0]); return 2; }
	std::vector<uint8_t> t1 = slurp(argv[1]), t2 = slurp(argv[2]);
	int32_t ip[6]; for (int i = 0; i < 6; ++i) ip[i] = atoi(argv[5 + i]);
	const int out3 = atoi(argv[11]);
	const int64_t cap = (int64_t)std::max(t1.size(), t2.size()) / 4 + 2;
	std::vector<int32_t> plan((size_t)cap * PG_PLAN); std::vector<uint64_t> acons(400), ec(3000); uint64_t out[4];
	if (purge_emul(t1.data(), (int64_t)t1.size(), t2.data(), (int64_t)t2.size(), 1, 0, argv[3], argv[4], 80.0, 1e-6, ip, plan.data(), cap, acons.data(), ec.data(), out) != 0) return 3;
	for (uint64_t r = 0; r < out[0]; ++r) { for (int k = 0; k < PG_PLAN; ++k) printf("%d%c", plan[PG_PLAN * r + k], k + 1 < PG_PLAN ? ' ' : '\n'); }
	if (out[1] != FQ_NO_ERROR) { printf("error %" PRIu64 " %" PRIu64 "\n", (uint64_t)(out[1] >> 8), (uint64_t)(out[1] & 255)); return 0; }
	std::vector<uint8_t> text(t1.size() + t2.size() + 16);
	for (int k = 0; k < 4; ++k) printf("stream %d: %" PRId64 " bytes\n", k, purge_format(t1.data(), (int64_t)t1.size(), t2.data(), (int64_t)t2.size(), plan.data(), (int64_t)out[0], ip[0], out3, k, text.data(), (int64_t)text.size()));
	return 0;
}
