// The position table under the emulator as a stand-alone program, so that it can be built with -fsanitize=address,undefined and run on its own
// (tests/test_cpu_postable.py). Usage: postable_emul_main CASE
// CASE: whitespace-separated integers - rules n_ref, the reference lengths, n and seven numbers per item (PtItem), the number of queries and (form tid x) per
// query. Items, lengths and the table's arrays live in heap buffers of exactly their size. Prints "error MESSAGE", or the five arrays and an answer per query.
#include "postable_emul.cpp"
#include <cinttypes>
#include <cstdio>
#include <cstdlib>

int main(int argc, char** argv)
{
	if (argc != 2) { fprintf(stderr, "usage: %s CASE\n", argv[0]); return 2; }
	FILE* f = fopen(argv[1], "r");
	if (!f) { perror(argv[1]); return 2; }
	std::vector<int64_t> in; long long v;
	while (fscanf(f, "%lld", &v) == 1) in.push_back(v);
	fclose(f);
	size_t k = 0;
	auto next = [&]() -> int64_t { if (k >= in.size()) { fprintf(stderr, "the case ends early\n"); exit(2); } return in[k++]; };
	const int rules = (int)next(); const int32_t n_ref = (int32_t)next();
	std::vector<int64_t> ref_lens((size_t)n_ref); for (auto& l : ref_lens) l = next();
	std::vector<PtItem> items((size_t)next());
	for (auto& x : items) for (int32_t* p : {&x.tid, &x.start, &x.end, &x.kind, &x.len, &x.has_allele, &x.has_slice}) *p = (int32_t)next();
	char err[256];
	void* t = postable_emul_build(rules, items.data(), (int64_t)items.size(), ref_lens.data(), n_ref, err);
	if (!t) { printf("error %s\n", err); return 0; }
	for (int which = 0; which < 5; ++which)
	{
		const int64_t n = postable_emul_array(t, which, nullptr, -1);
		std::vector<int64_t> w((size_t)n); std::vector<int32_t> n32((size_t)n);
		postable_emul_array(t, which, which == 4 ? (void*)w.data() : (void*)n32.data(), n);
		printf("array %d:", which);
		for (int64_t i = 0; i < n; ++i) printf(" %" PRId64, which == 4 ? w[(size_t)i] : (int64_t)n32[(size_t)i]);
		printf("\n");
	}
	for (int64_t q = next(); q > 0; --q)
	{
		const int form = (int)next(); const int32_t tid = (int32_t)next(); const int64_t x = next(); int32_t a;
		postable_emul_lower(t, form, tid, &x, 1, &a);
		printf("%d\n", a);
	}
	postable_emul_free(t);
	return 0;
}
