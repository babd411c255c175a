// report_host_test.cpp — the host loops of the content report (csrc/report.hpp: rp_bases_host, rp_quals_host, rp_values_host, rp_add,
// rp_nxx) and the `hipreport` stream (csrc/cli/report_stream.hpp: pack, unpack, report_mismatch) as a stand-alone program (own main,
// nothing preloaded, no HIP), for a build under AddressSanitizer and UBSan (tests/test_report_cpu.py builds and runs it):
//   report_host_test FILE
// FILE: u64 n_cases, then per case i32 mode, u32 n_fwd, 8 x u32 fwd, u32 n_rev, 8 x u32 rev, u64 n_reads, (n_reads + 1) u64 offsets, the
// base codes, the input quality bytes (both of offsets[n_reads] bytes).  Per case: the report whole, and split in two calls at each read
// boundary and added (must be the same); the values of dg_qual_values_host through rp_values_host must give the OUT marginal; the
// stream packed, unpacked and packed again must be the same bytes; prints the stream in hex.
#include "../../colord_amd/csrc/cli/report_stream.hpp"
#include <cinttypes>

static bool same(const cl_report& a, const cl_report& b) { return memcmp(&a, &b, sizeof(cl_report)) == 0; }

int main(int argc, char** argv)
{
	if (argc != 2) { fprintf(stderr, "usage: report_host_test FILE\n"); return 2; }
	FILE* f = fopen(argv[1], "rb");
	if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
	uint64_t n_cases = 0;
	if (fread(&n_cases, 8, 1, f) != 1) return 2;
	for (uint64_t c = 0; c < n_cases; ++c)
	{
		cl_qual_params P{}; uint64_t n = 0;
		if (fread(&P.mode, 4, 1, f) != 1 || fread(&P.n_fwd, 4, 1, f) != 1 || fread(P.fwd, 4, 8, f) != 8 || fread(&P.n_rev, 4, 1, f) != 1 || fread(P.rev, 4, 8, f) != 8) return 2;
		if (fread(&n, 8, 1, f) != 1) return 2;
		P.level = 1;
		std::vector<uint64_t> off(n + 1);
		if (fread(off.data(), 8, n + 1, f) != n + 1) return 2;
		std::vector<uint8_t> codes(off[n]), quals(off[n]), values(off[n]);        // exactly the bytes: one past them is the sanitizer's to report
		if (off[n] && (fread(codes.data(), 1, off[n], f) != off[n] || fread(quals.data(), 1, off[n], f) != off[n])) return 2;
		ReportSet whole;
		if (!rp_bases_host(codes.data(), off.data(), n, whole.r.get()) || !rp_quals_host(&P, quals.data(), off.data(), n, whole.r.get())) { fprintf(stderr, "case %" PRIu64 ": refused\n", c); return 1; }
		for (uint64_t cut = 0; cut <= n; ++cut)
		{
			ReportSet a, b;
			if (!rp_bases_host(codes.data(), off.data() + cut, n - cut, a.r.get()) || !rp_quals_host(&P, quals.data(), off.data() + cut, n - cut, a.r.get())) return 1;
			if (!rp_bases_host(codes.data(), off.data(), cut, b.r.get()) || !rp_quals_host(&P, quals.data(), off.data(), cut, b.r.get())) return 1;
			rp_add(a.r.get(), b.r.get());
			if (!same(*whole.r, *a.r)) { fprintf(stderr, "case %" PRIu64 ": split at %" PRIu64 " differs\n", c, cut); return 1; }
		}
		if (P.mode != 8)
		{	// what a decoder would hand on: the values, counted as decoded bytes, give the OUT marginal and nothing of the IN side
			ReportSet v;
			if (!dg_qual_values_host(&P, quals.data(), off.data(), n, values.data(), 0, nullptr) || !rp_values_host(values.data(), off.data(), n, v.r.get())) return 1;
			for (int j = 0; j < 96; ++j) if (v.out_marginal(j) != whole.out_marginal(j) || v.r->q_joint[0][j] != v.out_marginal(j)) { fprintf(stderr, "case %" PRIu64 ": OUT marginal of value %d differs\n", c, j); return 1; }
			if (v.r->q_reads != whole.r->q_reads || v.r->q_symbols != whole.r->q_symbols || v.r->reads) return 1;      // (only the quality part is filled)
		}
		std::vector<uint64_t> lens; for (uint64_t i = 0; i < n; ++i) lens.push_back(off[i + 1] - off[i]);
		whole.n50 = rp_nxx(lens, 50); whole.n90 = rp_nxx(lens, 90);
		const std::vector<uint8_t> packed = whole.pack();
		ReportSet back;
		if (!back.unpack(packed) || !same(*back.r, *whole.r) || back.n50 != whole.n50 || back.pack() != packed || !report_mismatch(whole, back).empty()) { fprintf(stderr, "case %" PRIu64 ": the stream does not round-trip\n", c); return 1; }
		for (size_t cut = 0; cut < packed.size(); cut += packed.size() / 97 + 1)
		{	// no prefix of a stream is a stream
			ReportSet t; if (t.unpack(std::vector<uint8_t>(packed.begin(), packed.begin() + cut))) { fprintf(stderr, "case %" PRIu64 ": a stream cut at %zu was read\n", c, cut); return 1; }
		}
		printf("case ");
		for (uint8_t b : packed) printf("%02x", b);
		printf("\n");
	}
	fclose(f);
	// what the layout refuses: *-fix without a -D value for every bin, a -D value above 95; mode none adds nothing
	cl_qual_params P{}; P.mode = 6; P.level = 1; P.n_fwd = 1; P.fwd[0] = 7; P.n_rev = 1; P.rev[0] = 1;
	ReportSet r; const uint64_t off1[2] = { 0, 0 };
	if (rp_quals_host(&P, nullptr, off1, 1, r.r.get())) { fprintf(stderr, "2-fix with one -D value was accepted\n"); return 1; }
	P.n_rev = 2; P.rev[1] = 96;
	if (rp_quals_host(&P, nullptr, off1, 1, r.r.get())) { fprintf(stderr, "a -D value of 96 was accepted\n"); return 1; }
	P.rev[1] = 95;
	if (!rp_quals_host(&P, nullptr, off1, 1, r.r.get()) || r.r->q_reads != 1 || !r.r->has_qual) { fprintf(stderr, "a -D value of 95 was refused\n"); return 1; }
	P.mode = 8; P.n_fwd = 0;
	ReportSet none;
	if (!rp_quals_host(&P, nullptr, off1, 1, none.r.get()) || none.r->has_qual || none.r->q_reads) { fprintf(stderr, "mode none\n"); return 1; }
	if (rp_len_bin(0) != 0 || rp_len_bin(1) != 1 || rp_len_bin(3) != 2 || rp_len_bin(4) != 3 || rp_len_bin(0xffffffffULL) != 32 || rp_len_bin(~0ULL) != 32) { fprintf(stderr, "rp_len_bin\n"); return 1; }
	printf("ok: %" PRIu64 " cases\n", n_cases);
	return 0;
}
