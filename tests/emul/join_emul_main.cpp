// The mate join's text under the emulator as a stand-alone program, so that it can be built with -fsanitize=address,undefined and run on its own
// (tests/test_cpu_join_designed.py). Usage: join_emul_main RECS OFFS TILES PART PASS BITS
// RECS: the records end to end; OFFS: int64[n + 1]; TILES: int32[n]; PART, PASS: uint8[n]; BITS: the hash bits. Every file is read into a heap buffer of exactly
// its size. Prints a line per closing record, the held entries and pool bytes behind every tile, the open records and the counts.
#include "join_emul.cpp"
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
	if (argc != 7) { fprintf(stderr, "usage: %s RECS OFFS TILES PART PASS BITS\n", argv[0]); return 2; }
	const std::vector<uint8_t> recs = slurp(argv[1]), offs = slurp(argv[2]), tiles = slurp(argv[3]), part = slurp(argv[4]), pass = slurp(argv[5]);
	const int64_t n = (int64_t)part.size();
	if ((int64_t)offs.size() != 8 * (n + 1) || (int64_t)tiles.size() != 4 * n || (int64_t)pass.size() != n) { fprintf(stderr, "sizes do not agree\n"); return 2; }
	std::vector<int64_t> recoff(n + 1); memcpy(recoff.data(), offs.data(), offs.size());
	std::vector<int32_t> tile_of(n + 1); memcpy(tile_of.data(), tiles.data(), tiles.size());
	const int32_t n_tiles = n ? tile_of[n - 1] + 1 : 0;
	std::vector<int64_t> opener_of(n + 1), h_after(n_tiles + 1), pool_after(n_tiles + 1), open_idx(n + 1); std::vector<uint8_t> kept(n + 1);
	unsigned long long counts[4];
	const int64_t H = join_emul(recs.data(), recoff.data(), tile_of.data(), n, n_tiles, part.data(), pass.data(), name_hash_mask(atoi(argv[6])), opener_of.data(), kept.data(),
	                            h_after.data(), pool_after.data(), open_idx.data(), counts);
	if (H < 0) { printf("held order broken behind tile %" PRId64 "\n", -1 - H); return 3; }
	for (int64_t i = 0; i < n; ++i) if (opener_of[i] >= 0) printf("pair %" PRId64 " %" PRId64 " %d\n", opener_of[i], i, (int)kept[i]);
	for (int32_t t = 0; t < n_tiles; ++t) printf("tile %d held %" PRId64 " bytes %" PRId64 "\n", t, h_after[t], pool_after[t]);
	for (int64_t e = 0; e < H; ++e) printf("open %" PRId64 "\n", open_idx[e]);
	printf("counts %llu %llu\n", counts[0], counts[1]);
	return 0;
}
