// The K1 kernels under the wave emulator as a stand-alone program, so that it can be built with -fsanitize=address,undefined and run on its own
// (tests/test_cpu_inflate_designed.py). Usage: k1_emul_main CASEFILE [tok_mode]
// CASEFILE: int64 member count, then per member uint32 clen, uint32 usize and clen payload bytes. The members are laid out as in a BGZF file: some
// bytes in front (a different alignment for every member), the payload, a zero CRC field and ISIZE. Prints "produced error" per member.
#include "k1_emul.cpp"
#include <cinttypes>

int main(int argc, char** argv)
{
	if (argc < 2) { fprintf(stderr, "usage: %s CASEFILE [tok_mode]\n", argv[0]); return 2; }
	FILE* f = fopen(argv[1], "rb");
	if (!f) { perror(argv[1]); return 2; }
	int64_t n = 0;
	if (fread(&n, sizeof n, 1, f) != 1 || n <= 0 || n > (1 << 20)) { fprintf(stderr, "bad member count\n"); return 2; }
	std::vector<uint8_t> img; std::vector<BlockDesc> bd((size_t)n);
	uint64_t up = 0;
	for (int64_t i = 0; i < n; ++i)
	{
		uint32_t hd[2];
		if (fread(hd, sizeof hd, 1, f) != 1 || hd[0] > 65536u || hd[1] > 65536u) { fprintf(stderr, "bad member %" PRId64 "\n", i); return 2; }
		img.insert(img.end(), (size_t)(18 + (i * 7) % 16), (uint8_t)0xa5);
		bd[(size_t)i] = BlockDesc{(uint64_t)img.size(), up, hd[0], hd[1]}; up += hd[1];
		const size_t at = img.size(); img.resize(at + hd[0]);
		if (hd[0] && fread(img.data() + at, 1, hd[0], f) != hd[0]) { fprintf(stderr, "short member %" PRId64 "\n", i); return 2; }
		for (int k = 0; k < 4; ++k) img.push_back(0);
		for (int k = 0; k < 4; ++k) img.push_back((uint8_t)(hd[1] >> (8 * k)));
	}
	fclose(f);
	img.insert(img.end(), 64, 0);
	std::vector<uint8_t> out((size_t)up + 64);
	std::vector<BlockStatus> st((size_t)n);
	k1_emul_inflate(img.data(), bd.data(), n, out.data(), st.data(), 16, argc > 2 ? atoi(argv[2]) : 0, 0, 0, 1, nullptr);
	for (int64_t i = 0; i < n; ++i) printf("%u %u\n", st[(size_t)i].produced, st[(size_t)i].error);
	// the inflated bytes of the members without an error, as one checksum (the caller holds the expected value)
	uint64_t h = 1469598103934665603ull;
	for (int64_t i = 0; i < n; ++i)
		if (!st[(size_t)i].error)
			for (uint32_t k = 0; k < bd[(size_t)i].usize; ++k) { h ^= out[(size_t)bd[(size_t)i].upos + k]; h *= 1099511628211ull; }
	printf("fnv %016" PRIx64 "\n", h);
	return 0;
}
