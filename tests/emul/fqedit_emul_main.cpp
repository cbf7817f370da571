// The per-entry text of the FASTQ tools under the emulator as a stand-alone program, so that it can be built with -fsanitize=address,undefined and run on its
// own (tests/test_cpu_fqedit_emul.py). Usage: fqedit_emul_main TEXT1 TEXT2|- IDS|- OP LONG_READ START END LEN MAX_LEN CUT1 CUT2 INVERT
// TEXT1 / TEXT2: the FASTQ texts as the accumulator hands them to the device, each read into a heap buffer of exactly its size. IDS: lines "id<TAB>payload".
// Prints the plan, a row per entry and side, and the sizes of the output texts.
#include "fqedit_emul.cpp"
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
	if (argc != 13) { fprintf(stderr, "usage: %s TEXT1 TEXT2|- IDS|- OP LONG_READ START END LEN MAX_LEN CUT1 CUT2 INVERT\n", argv[0]); return 2; }
	const int sides = strcmp(argv[2], "-") ? 2 : 1;
	std::vector<uint8_t> t1 = slurp(argv[1]), t2 = sides == 2 ? slurp(argv[2]) : std::vector<uint8_t>();
	std::vector<uint8_t> id_bytes; std::vector<int32_t> id_len, id_payload;
	if (strcmp(argv[3], "-"))
	{
		const std::vector<uint8_t> f = slurp(argv[3]);
		size_t b = 0;
		for (size_t i = 0; i < f.size(); ++i)
		{
			if (f[i] != '\n') continue;
			size_t tab = b; while (f[tab] != '\t') ++tab;
			id_bytes.insert(id_bytes.end(), f.begin() + (ptrdiff_t)b, f.begin() + (ptrdiff_t)tab); id_len.push_back((int32_t)(tab - b));
			id_payload.push_back(atoi(std::string(f.begin() + (ptrdiff_t)tab + 1, f.begin() + (ptrdiff_t)i).c_str()));
			b = i + 1;
		}
		id_bytes.shrink_to_fit();
	}
	int32_t ip[9]; for (int i = 0; i < 9; ++i) ip[i] = atoi(argv[4 + i]);
	const int64_t cap = (int64_t)std::max(t1.size(), t2.size()) / 4 + 2;
	std::vector<int32_t> plan((size_t)cap * FE_PLAN * sides); uint64_t out[4];
	if (fqedit_emul(t1.data(), (int64_t)t1.size(), t2.data(), (int64_t)t2.size(), sides, 1, ip, id_bytes.data(), id_len.data(), id_payload.data(), (int64_t)id_len.size(), plan.data(), cap, out) != 0) return 3;
	for (uint64_t r = 0; r < out[0] * (uint64_t)sides; ++r) { for (int k = 0; k < FE_PLAN; ++k) printf("%d%c", plan[FE_PLAN * r + k], k + 1 < FE_PLAN ? ' ' : '\n'); }
	if (out[1] != FQ_NO_ERROR) { printf("error %" PRIu64 " %" PRIu64 "\n", (uint64_t)(out[1] >> 8), (uint64_t)(out[1] & 255)); return 0; }
	// a buffer of exactly the size the plan announces: a byte written behind an entry ends the run
	for (int k = 0; k < sides; ++k)
	{
		uint64_t need = 0;
		{ std::vector<uint8_t> probe(2 * (t1.size() + t2.size()) + 64 * out[0] + 64); need = (uint64_t)fqedit_format(t1.data(), (int64_t)t1.size(), t2.data(), (int64_t)t2.size(), sides, ip, plan.data(), (int64_t)out[0], k, probe.data(), (int64_t)probe.size()); }
		std::vector<uint8_t> text((size_t)need);
		printf("stream %d: %" PRId64 " bytes\n", k, fqedit_format(t1.data(), (int64_t)t1.size(), t2.data(), (int64_t)t2.size(), sides, ip, plan.data(), (int64_t)out[0], k, text.data(), (int64_t)text.size()));
	}
	return 0;
}
