// mappings_host_test.cpp — the host twin of the lift (csrc/mappings.hpp: map_piece_first, map_lift_host) and the `hipmappings` stream
// (csrc/cli/mappings_stream.hpp: pack, unpack, PAF, coverage, summary) as a stand-alone program (own main, nothing preloaded, no HIP), for a
// build under AddressSanitizer and UBSan (tests/test_mappings_cpu.py builds and runs it):
//   mappings_host_test FILE
// FILE: u32 n_seqs, n_seqs u64 lengths, u32 read_len, u32 overlap; u64 n_cases, then per case u64 n and n records of twelve u32.
// Per case: the lift whole — a refused case must leave the output as it was — and split in two calls at record boundaries (must be the same
// records); the stream packed, unpacked and packed again must be the same bytes, one of another shape must be refused; the printers run
// into a scratch file; prints the stream in hex, or the refusal.
#include "../../colord_amd/csrc/cli/mappings_stream.hpp"
#include <cinttypes>

static bool same(const std::vector<cl_overlap>& a, const std::vector<cl_overlap>& b) { return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * sizeof(cl_overlap)) == 0); }

int main(int argc, char** argv)
{
	if (argc != 2) { fprintf(stderr, "usage: mappings_host_test FILE\n"); return 2; }
	FILE* f = fopen(argv[1], "rb");
	if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
	uint32_t n_seqs = 0, read_len = 0, overlap = 0; uint64_t n_cases = 0;
	if (fread(&n_seqs, 4, 1, f) != 1) return 2;
	std::vector<uint64_t> seq_len(n_seqs);                                     // exactly the entries: one past them is the sanitizer's to report
	if (n_seqs && fread(seq_len.data(), 8, n_seqs, f) != n_seqs) return 2;
	if (fread(&read_len, 4, 1, f) != 1 || fread(&overlap, 4, 1, f) != 1 || fread(&n_cases, 8, 1, f) != 1) return 2;
	std::vector<uint32_t> pf;
	if (map_piece_first(seq_len.data(), n_seqs, read_len, overlap, pf) != CL_OK || pf.size() != (size_t)n_seqs + 1) { fprintf(stderr, "the geometry is refused\n"); return 1; }
	const MapGeom G{ seq_len.data(), pf.data(), n_seqs, pf[n_seqs], read_len, read_len - overlap };
	FILE* sink = tmpfile();
	if (!sink) return 2;
	for (uint64_t c = 0; c < n_cases; ++c)
	{
		uint64_t n = 0;
		if (fread(&n, 8, 1, f) != 1) return 2;
		std::vector<cl_overlap> in(n);
		if (n && fread(in.data(), sizeof(cl_overlap), n, f) != n) return 2;
		MappingSet whole; whole.recs.resize(2); memset(whole.recs.data(), 0x5a, 2 * sizeof(cl_overlap));      // something in the output already
		const std::vector<cl_overlap> before = whole.recs;
		uint64_t bad = 0; uint32_t code = 0;
		if (!map_lift_host(G, in.data(), n, whole.recs, &bad, &code))
		{
			if (!same(before, whole.recs)) { fprintf(stderr, "case %" PRIu64 ": a refused batch changed the output\n", c); return 1; }
			printf("case refused record %" PRIu64 ": %u %s\n", bad, code, map_error_text(code));
			continue;
		}
		whole.recs.erase(whole.recs.begin(), whole.recs.begin() + 2);
		for (uint64_t cut = 0; cut <= n; cut += n > 64 ? n / 7 + 1 : 1)
		{
			std::vector<cl_overlap> ab;
			if (!map_lift_host(G, in.data(), cut, ab, nullptr, nullptr) || !map_lift_host(G, in.data() + cut, n - cut, ab, nullptr, nullptr)) return 1;
			if (!same(whole.recs, ab)) { fprintf(stderr, "case %" PRIu64 ": split at %" PRIu64 " differs\n", c, cut); return 1; }
		}
		whole.read_len = read_len; whole.overlap = overlap; whole.seq_len = seq_len;
		for (uint32_t s = 0; s < n_seqs; ++s) whole.names.push_back(s == 2 ? std::string() : "s" + std::to_string(s));      // (one sequence without a name)
		const std::vector<uint8_t> packed = whole.pack();
		MappingSet back;
		if (!back.unpack(packed) || !same(back.recs, whole.recs) || back.names != whole.names || back.seq_len != whole.seq_len || back.pack() != packed) { fprintf(stderr, "case %" PRIu64 ": the stream does not round-trip\n", c); return 1; }
		MappingSet t; std::vector<uint8_t> other = packed, size = packed, seqs = packed; other[0] = 2; size[4] = 44; seqs[8] = (uint8_t)(seqs[8] + 1);
		if (t.unpack(other) || t.unpack(size) || t.unpack(seqs) || t.unpack(std::vector<uint8_t>(packed.begin(), packed.end() - 1)) || t.unpack(std::vector<uint8_t>(packed.begin(), packed.begin() + 8)) ||
		    t.unpack(std::vector<uint8_t>(packed.begin(), packed.begin() + std::min<size_t>(packed.size(), MappingSet::HEAD + 5))))
		{ fprintf(stderr, "case %" PRIu64 ": a stream of another shape was read\n", c); return 1; }
		if (!whole.recs.empty())
		{	// a record that names a sequence the table does not hold, and one that ends behind its sequence
			MappingSet bad_t = whole, bad_e = whole;
			bad_t.recs[0].t = n_seqs; bad_e.recs.back().te = (uint32_t)seq_len[bad_e.recs.back().t] + 1;
			if (t.unpack(bad_t.pack()) || t.unpack(bad_e.pack())) { fprintf(stderr, "case %" PRIu64 ": a record outside its sequence was read\n", c); return 1; }
		}
		if (!print_mappings_paf(sink, back, 0, nullptr)) return 1;
		print_mappings_coverage(sink, back, 1); print_mappings_coverage(sink, back, 64); print_mappings_coverage(sink, back, 1000);
		print_mappings_summary(sink, summarize_mappings(back, 5000), true); print_mappings_summary(sink, summarize_mappings(back, 5000), false);
		printf("case ");
		for (uint8_t b : packed) printf("%02x", b);
		printf("\n");
	}
	fclose(sink); fclose(f);
	printf("ok: %" PRIu64 " cases\n", n_cases);
	return 0;
}
