// overlaps_host_test.cpp — the host form of the overlap records (csrc/overlaps.hpp: ov_walk_host) and the `hipoverlaps` stream
// (csrc/cli/overlaps_stream.hpp: pack, unpack, PAF) as a stand-alone program (own main, nothing preloaded, no HIP), for a build under
// AddressSanitizer and UBSan (tests/test_overlaps_cpu.py builds and runs it):
//   overlaps_host_test FILE
// FILE: u32 n_refs, (n_refs + 1) u64 offsets, the reference codes; u64 n_cases, then per case u64 n_reads, (n_reads + 1) u64 offsets, the
// stream bytes.  Per case: the records whole with a translation table (id -> 1000 + id) and first read 7 — a refused case must leave the
// output as it was — and split in two calls at each read boundary (must be the same records); the stream packed, unpacked and packed
// again must be the same bytes, one of another shape must be refused; prints the stream in hex, or the refusal.
#include "../../colord_amd/csrc/cli/overlaps_stream.hpp"
#include <cinttypes>

static bool same(const std::vector<cl_overlap>& a, const std::vector<cl_overlap>& b) { return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * sizeof(cl_overlap)) == 0); }

int main(int argc, char** argv)
{
	if (argc != 2) { fprintf(stderr, "usage: overlaps_host_test FILE\n"); return 2; }
	FILE* f = fopen(argv[1], "rb");
	if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
	uint32_t n_refs = 0; uint64_t n_cases = 0;
	if (fread(&n_refs, 4, 1, f) != 1) return 2;
	std::vector<uint64_t> roff((size_t)n_refs + 1);
	if (fread(roff.data(), 8, roff.size(), f) != roff.size()) return 2;
	std::vector<uint8_t> rc(roff[n_refs]);                                     // exactly the bytes: one past them is the sanitizer's to report
	if (!rc.empty() && fread(rc.data(), 1, rc.size(), f) != rc.size()) return 2;
	std::vector<uint32_t> table(n_refs);                                       // exactly n_refs entries
	for (uint32_t i = 0; i < n_refs; ++i) table[i] = 1000 + i;
	if (fread(&n_cases, 8, 1, f) != 1) return 2;
	const uint64_t first = 7;
	for (uint64_t c = 0; c < n_cases; ++c)
	{
		uint64_t n = 0;
		if (fread(&n, 8, 1, f) != 1) return 2;
		std::vector<uint64_t> off(n + 1);
		if (fread(off.data(), 8, n + 1, f) != n + 1) return 2;
		std::vector<uint8_t> es(off[n]);
		if (off[n] && fread(es.data(), 1, off[n], f) != off[n]) return 2;
		OverlapSet whole; whole.recs.resize(2); memset(whole.recs.data(), 0x5a, 2 * sizeof(cl_overlap));      // something in the output already
		const std::vector<cl_overlap> before = whole.recs;
		uint64_t bad = 0; uint32_t code = 0;
		if (!ov_walk_host(rc.data(), roff.data(), n_refs, es.data(), off.data(), n, first, table.data(), n_refs, whole.recs, &bad, &code))
		{
			if (!same(before, whole.recs)) { fprintf(stderr, "case %" PRIu64 ": a refused batch changed the output\n", c); return 1; }
			printf("case refused read %" PRIu64 ": %s\n", bad, ed_error_text(code));
			continue;
		}
		whole.recs.erase(whole.recs.begin(), whole.recs.begin() + 2);
		for (uint64_t cut = 0; cut <= n; cut += n > 64 ? n / 7 + 1 : 1)
		{
			std::vector<cl_overlap> ab;
			if (!ov_walk_host(rc.data(), roff.data(), n_refs, es.data(), off.data(), cut, first, table.data(), n_refs, ab, nullptr, nullptr)) return 1;
			if (!ov_walk_host(rc.data(), roff.data(), n_refs, es.data(), off.data() + cut, n - cut, first + cut, table.data(), n_refs, ab, nullptr, nullptr)) return 1;
			if (!same(whole.recs, ab)) { fprintf(stderr, "case %" PRIu64 ": split at %" PRIu64 " differs\n", c, cut); return 1; }
		}
		// a table one entry short refuses the read that names the last reference, and only such a read
		{
			std::vector<cl_overlap> t; uint32_t cd = 0;
			const bool ok = n_refs ? ov_walk_host(rc.data(), roff.data(), n_refs, es.data(), off.data(), n, first, table.data(), n_refs - 1, t, nullptr, &cd) : true;
			if (!ok && cd != EDE_REF_ID) { fprintf(stderr, "case %" PRIu64 ": a short table gave code %u\n", c, cd); return 1; }
			if (ok && n_refs && !same(whole.recs, t)) { fprintf(stderr, "case %" PRIu64 ": a short table changed the records\n", c); return 1; }
		}
		const std::vector<uint8_t> packed = whole.pack();
		OverlapSet back;
		if (packed.size() != OverlapSet::HEAD + whole.recs.size() * 48 || !back.unpack(packed) || !same(back.recs, whole.recs) || back.pack() != packed) { fprintf(stderr, "case %" PRIu64 ": the stream does not round-trip\n", c); return 1; }
		OverlapSet t; std::vector<uint8_t> other = packed, size = packed; other[0] = 2; size[4] = 44;
		if (t.unpack(other) || t.unpack(size) || t.unpack(std::vector<uint8_t>(packed.begin(), packed.end() - 1)) || t.unpack(std::vector<uint8_t>(packed.begin(), packed.begin() + 8)))
		{ fprintf(stderr, "case %" PRIu64 ": a stream of another shape was read\n", c); return 1; }
		for (const cl_overlap& o : whole.recs) (void)ov_block(o);
		printf("case ");
		for (uint8_t b : packed) printf("%02x", b);
		printf("\n");
	}
	fclose(f);
	printf("ok: %" PRIu64 " cases\n", n_cases);
	return 0;
}
