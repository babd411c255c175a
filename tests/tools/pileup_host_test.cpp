// pileup_host_test.cpp — the host twin of the pileup (csrc/pileup.hpp: pile_geometry, the visitor of es_walk_host, the fold, the sites) and the
// `hippileup` stream (csrc/cli/pileup_stream.hpp: pack, unpack, table, VCF, summary) as a stand-alone program (own main, nothing preloaded, no
// HIP), for a build under AddressSanitizer and UBSan (tests/test_pileup_cpu.py builds and runs it):
//   pileup_host_test FILE
// FILE: u32 n_seqs, n_seqs u64 lengths, u32 read_len, u32 overlap, three u32 thresholds; u32 n_refs, n_refs + 1 u64 offsets, the reference codes;
// u64 n_cases, then per case u64 n_reads, n_reads + 1 u64 offsets and the stream bytes.
// Per case: the batch whole and split in two adds at every read boundary (or every seventh part) must give the same table; the stream packed,
// unpacked and packed again must be the same bytes, one of another shape must be refused; the printers run into a scratch file; prints the
// columns' and the stream's bytes in hex, or the refusal.
#include "../../colord_amd/csrc/cli/pileup_stream.hpp"
#include <cinttypes>

int main(int argc, char** argv)
{
	if (argc != 2) { fprintf(stderr, "usage: pileup_host_test FILE\n"); return 2; }
	FILE* f = fopen(argv[1], "rb");
	if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
	uint32_t n_seqs = 0, read_len = 0, overlap = 0, thr[3] = { 0, 0, 0 }, n_refs = 0; uint64_t n_cases = 0;
	if (fread(&n_seqs, 4, 1, f) != 1) return 2;
	std::vector<uint64_t> seq_len(n_seqs);                                     // exactly the entries: one past them is the sanitizer's to report
	if (n_seqs && fread(seq_len.data(), 8, n_seqs, f) != n_seqs) return 2;
	if (fread(&read_len, 4, 1, f) != 1 || fread(&overlap, 4, 1, f) != 1 || fread(thr, 4, 3, f) != 3 || fread(&n_refs, 4, 1, f) != 1) return 2;
	std::vector<uint64_t> ref_off((size_t)n_refs + 1);
	if (fread(ref_off.data(), 8, ref_off.size(), f) != ref_off.size()) return 2;
	std::vector<uint8_t> ref_codes(ref_off[n_refs]);
	if (!ref_codes.empty() && fread(ref_codes.data(), 1, ref_codes.size(), f) != ref_codes.size()) return 2;
	if (fread(&n_cases, 8, 1, f) != 1) return 2;
	const PileThresholds T{ thr[0], thr[1], thr[2] };
	FILE* sink = tmpfile();
	if (!sink) return 2;
	for (uint64_t c = 0; c < n_cases; ++c)
	{
		uint64_t n = 0;
		if (fread(&n, 8, 1, f) != 1) return 2;
		std::vector<uint64_t> off(n + 1);
		if (fread(off.data(), 8, off.size(), f) != off.size()) return 2;
		std::vector<uint8_t> es(off[n]);                                       // exactly the bytes
		if (!es.empty() && fread(es.data(), 1, es.size(), f) != es.size()) return 2;
		PileHost H;
		if (H.init(seq_len.data(), n_seqs, read_len, overlap) != CL_OK || H.G.n_pseudo > n_refs) { fprintf(stderr, "the geometry is refused\n"); return 1; }
		uint64_t bad = 0; uint32_t code = 0;
		if (!pile_add_host(H, ref_codes.data(), ref_off.data(), n_refs, es.data(), off.data(), n, &bad, &code))
		{
			printf("case refused read %" PRIu64 ": %u %s\n", bad, code, ed_error_text(code));
			continue;
		}
		for (uint64_t cut = 0; cut <= n; cut += n > 64 ? n / 7 + 1 : 1)
		{	// two adds are one
			PileHost A;
			if (A.init(seq_len.data(), n_seqs, read_len, overlap) != CL_OK) return 1;
			if (!pile_add_host(A, ref_codes.data(), ref_off.data(), n_refs, es.data(), off.data(), cut, nullptr, nullptr) ||
			    !pile_add_host(A, ref_codes.data(), ref_off.data(), n_refs, es.data(), off.data() + cut, n - cut, nullptr, nullptr)) return 1;
			if (A.cols != H.cols || A.diff != H.diff || memcmp(&A.sums, &H.sums, sizeof(A.sums)) != 0) { fprintf(stderr, "case %" PRIu64 ": split at %" PRIu64 " differs\n", c, cut); return 1; }
		}
		pile_fold_host(H, ref_codes.data(), ref_off.data());
		PileupSet S; S.read_len = read_len; S.overlap = overlap; S.thr = T; S.sums = H.sums; S.seq_len = seq_len;
		for (uint32_t s = 0; s < n_seqs; ++s) S.names.push_back(s == 2 ? std::string() : "s" + std::to_string(s));      // (one sequence without a name)
		pile_sites_host(H, T, S.sites);
		const std::vector<uint8_t> packed = S.pack();
		PileupSet back;
		if (!back.unpack(packed) || back.sites.size() != S.sites.size() || back.names != S.names || back.seq_len != S.seq_len || back.pack() != packed) { fprintf(stderr, "case %" PRIu64 ": the stream does not round-trip\n", c); return 1; }
		PileupSet t; std::vector<uint8_t> other = packed, size = packed, seqs = packed; other[0] = 2; size[4] = 44; seqs[8] = (uint8_t)(seqs[8] + 1);
		if (t.unpack(other) || t.unpack(size) || t.unpack(seqs) || t.unpack(std::vector<uint8_t>(packed.begin(), packed.end() - 1)) || t.unpack(std::vector<uint8_t>(packed.begin(), packed.begin() + 8)) ||
		    t.unpack(std::vector<uint8_t>(packed.begin(), packed.begin() + std::min<size_t>(packed.size(), PileupSet::HEAD + 5))))
		{ fprintf(stderr, "case %" PRIu64 ": a stream of another shape was read\n", c); return 1; }
		if (!S.sites.empty())
		{	// a site on a sequence the table does not hold, one behind its sequence's end, a base and a kind out of range, two sites in the wrong order
			PileupSet b1 = S, b2 = S, b3 = S, b4 = S, b5 = S;
			b1.sites[0].seq = n_seqs; b2.sites.back().pos = (uint32_t)seq_len[b2.sites.back().seq]; b3.sites[0].ref = 4; b4.sites[0].kind = 6; b5.sites.push_back(b5.sites[0]);
			if (t.unpack(b1.pack()) || t.unpack(b2.pack()) || t.unpack(b3.pack()) || t.unpack(b4.pack()) || t.unpack(b5.pack())) { fprintf(stderr, "case %" PRIu64 ": a site that cannot be was read\n", c); return 1; }
		}
		print_pileup_table(sink, back, 0, 0); print_pileup_table(sink, back, 5, 500); print_pileup_vcf(sink, back, 0, 0); print_pileup_summary(sink, back, true); print_pileup_summary(sink, back, false);
		printf("case ");
		for (uint32_t v : H.cols) printf("%08x", v);
		printf(" ");
		for (uint8_t b : packed) printf("%02x", b);
		printf("\n");
	}
	fclose(sink); fclose(f);
	printf("ok: %" PRIu64 " cases\n", n_cases);
	return 0;
}
