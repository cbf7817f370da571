// The per-entry text of FastqExtractBarcode, FastqAddBarcode, FastqDownsample and FastqConcat under the emulator as a stand-alone program, so that it can be
// built with -fsanitize=address,undefined and run on its own (tests/test_cpu_fqedit2_emul.py). Usage: fqedit2_emul_main OP CUT KEEP|- TEXT...
// TEXT: the texts of one file per side of the op, as the accumulator hands them to the device, each read into a heap buffer of exactly its size. KEEP: a file
// of one byte (0 / 1) per entry. Prints the plan, a row per entry and stream, the sizes of the output texts and that of the kept headers.
#include "fqedit2_emul.cpp"
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
	if (argc < 5) { fprintf(stderr, "usage: %s OP CUT KEEP|- TEXT...\n", argv[0]); return 2; }
	const int op = atoi(argv[1]), cut = atoi(argv[2]);
	const FeShape sh = fe_shape(op);
	if (argc != 4 + sh.sides) { fprintf(stderr, "operation %d takes %d texts\n", op, sh.sides); return 2; }
	std::vector<uint8_t> text[FE_MAX_SIDES], keep;
	if (strcmp(argv[3], "-")) keep = slurp(argv[3]);
	const uint8_t* t[FE_MAX_SIDES] = {nullptr, nullptr, nullptr}; int64_t n[FE_MAX_SIDES] = {0, 0, 0};
	size_t longest = 0, all = 0;
	for (int k = 0; k < sh.sides; ++k) { text[k] = slurp(argv[4 + k]); t[k] = text[k].data(); n[k] = (int64_t)text[k].size(); longest = std::max(longest, text[k].size()); all += text[k].size(); }
	const int64_t cap = (int64_t)longest / 4 + 2;
	std::vector<int32_t> plan((size_t)cap * FE_PLAN * sh.streams); uint64_t out[4];
	if (fqedit2_emul(t, n, op, cut, keep.data(), plan.data(), cap, out) != 0) return 3;
	if (op == FE_OP_DOWNSAMPLE && keep.size() < out[0]) return 4;
	for (uint64_t r = 0; r < out[0] * (uint64_t)sh.streams; ++r) { for (int k = 0; k < FE_PLAN; ++k) printf("%d%c", plan[FE_PLAN * r + k], k + 1 < FE_PLAN ? ' ' : '\n'); }
	// a buffer of exactly the size the plan announces: a byte written behind an entry ends the run
	std::vector<uint8_t> probe(2 * all + 128 * out[0] + 64);
	for (int k = 0; k < sh.streams; ++k)
	{
		const int64_t need = fqedit2_format(t, n, op, plan.data(), (int64_t)out[0], k, probe.data(), (int64_t)probe.size());
		if (need < 0) return 5;
		std::vector<uint8_t> exact((size_t)need);
		printf("stream %d: %" PRId64 " bytes\n", k, fqedit2_format(t, n, op, plan.data(), (int64_t)out[0], k, exact.data(), (int64_t)exact.size()));
	}
	if (op == FE_OP_DOWNSAMPLE)
	{
		const int64_t need = fqedit2_headers(t, n, op, plan.data(), (int64_t)out[0], probe.data(), (int64_t)probe.size());
		if (need < 0) return 6;
		std::vector<uint8_t> exact((size_t)need);
		printf("headers: %" PRId64 " bytes\n", fqedit2_headers(t, n, op, plan.data(), (int64_t)out[0], exact.data(), (int64_t)exact.size()));
	}
	return 0;
}
