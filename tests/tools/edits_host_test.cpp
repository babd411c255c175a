// edits_host_test.cpp — the host form of the edit-operation profile (csrc/edits.hpp: ed_profile_host, ed_add) and the `hipedits` stream
// (csrc/cli/edits_stream.hpp: pack, unpack) as a stand-alone program (own main, nothing preloaded, no HIP), for a build under
// AddressSanitizer and UBSan (tests/test_edits_cpu.py builds and runs it):
//   edits_host_test FILE
// FILE: u32 n_refs, (n_refs + 1) u64 offsets, the reference codes; u64 n_cases, then per case u64 n_reads, (n_reads + 1) u64 offsets, the
// stream bytes.  Per case: the profile whole — a refused case must leave the total as it was — and split in two calls at each read
// boundary and added (must be the same); the stream packed, unpacked and packed again must be the same bytes; prints the stream in hex, or
// the refusal.
#include "../../colord_amd/csrc/cli/edits_stream.hpp"
#include <cinttypes>

static bool same(const cl_edits& a, const cl_edits& b) { return memcmp(&a, &b, sizeof(cl_edits)) == 0; }

int main(int argc, char** argv)
{
	if (argc != 2) { fprintf(stderr, "usage: edits_host_test FILE\n"); return 2; }
	FILE* f = fopen(argv[1], "rb");
	if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
	uint32_t n_refs = 0; uint64_t n_cases = 0;
	if (fread(&n_refs, 4, 1, f) != 1) return 2;
	std::vector<uint64_t> roff((size_t)n_refs + 1);
	if (fread(roff.data(), 8, roff.size(), f) != roff.size()) return 2;
	std::vector<uint8_t> rc(roff[n_refs]);                                     // exactly the bytes: one past them is the sanitizer's to report
	if (!rc.empty() && fread(rc.data(), 1, rc.size(), f) != rc.size()) return 2;
	if (fread(&n_cases, 8, 1, f) != 1) return 2;
	for (uint64_t c = 0; c < n_cases; ++c)
	{
		uint64_t n = 0;
		if (fread(&n, 8, 1, f) != 1) return 2;
		std::vector<uint64_t> off(n + 1);
		if (fread(off.data(), 8, n + 1, f) != n + 1) return 2;
		std::vector<uint8_t> es(off[n]);
		if (off[n] && fread(es.data(), 1, off[n], f) != off[n]) return 2;
		EditsSet whole; whole.e->reads = 7; whole.e->alt_hist[64] = 9;           // something in the total already
		const cl_edits before = *whole.e;
		uint64_t bad = 0; uint32_t code = 0;
		if (!ed_profile_host(rc.data(), roff.data(), n_refs, es.data(), off.data(), n, whole.e.get(), &bad, &code))
		{
			if (!same(before, *whole.e)) { fprintf(stderr, "case %" PRIu64 ": a refused batch changed the total\n", c); return 1; }
			printf("case refused read %" PRIu64 ": %s\n", bad, ed_error_text(code));
			continue;
		}
		whole.e->reads -= 7; whole.e->alt_hist[64] -= 9;
		for (uint64_t cut = 0; cut <= n; cut += n > 64 ? n / 7 + 1 : 1)
		{
			EditsSet a, b;
			if (!ed_profile_host(rc.data(), roff.data(), n_refs, es.data(), off.data() + cut, n - cut, a.e.get(), nullptr, nullptr)) return 1;
			if (!ed_profile_host(rc.data(), roff.data(), n_refs, es.data(), off.data(), cut, b.e.get(), nullptr, nullptr)) return 1;
			ed_add(a.e.get(), b.e.get());
			if (!same(*whole.e, *a.e)) { fprintf(stderr, "case %" PRIu64 ": split at %" PRIu64 " differs\n", c, cut); return 1; }
		}
		const std::vector<uint8_t> packed = whole.pack();
		EditsSet back;
		if (packed.size() != EditsSet::BYTES || !back.unpack(packed) || !same(*back.e, *whole.e) || back.pack() != packed) { fprintf(stderr, "case %" PRIu64 ": the stream does not round-trip\n", c); return 1; }
		EditsSet t; std::vector<uint8_t> other = packed; other[0] = 2;
		if (t.unpack(other) || t.unpack(std::vector<uint8_t>(packed.begin(), packed.end() - 1))) { fprintf(stderr, "case %" PRIu64 ": a stream of another shape was read\n", c); return 1; }
		(void)edits_derived(*whole.e);
		printf("case ");
		for (uint8_t b : packed) printf("%02x", b);
		printf("\n");
	}
	fclose(f);
	if (ed_bit_len(0) != 0 || ed_bit_len(1) != 1 || ed_bit_len(3) != 2 || ed_bit_len(4) != 3 || ed_bit_len(0x0fffffffu) != 28 || ed_run_bin(16) != 16 || ed_run_bin(17) != 16 || ed_run_bin(1) != 1) { fprintf(stderr, "bins\n"); return 1; }
	printf("ok: %" PRIu64 " cases\n", n_cases);
	return 0;
}
