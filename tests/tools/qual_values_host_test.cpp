// qual_values_host_test.cpp — the host loops of the qual-values digest (csrc/digest.hpp: dg_value_layout, dg_qual_values_host,
// dg_qual_ascii_host) as a stand-alone program (own main, nothing preloaded, no HIP), for a build under AddressSanitizer and UBSan
// (tests/test_qual_values_cpu.py builds and runs it):
//   qual_values_host_test FILE
// FILE: u64 n_cases, then per case i32 mode, u32 n_fwd, 8 x u32 fwd, u32 n_rev, 8 x u32 rev, u64 first_read, u64 n_reads, (n_reads + 1) u64
// offsets, the input quality bytes.  Per case: the values into a buffer of exactly the bytes, their digest from the input, the digest of the
// values as a decoder would hand them on (must be the same), both once whole and split in two calls at each read boundary; prints the triple
// and the values in hex.
#include "../../colord_amd/csrc/digest.hpp"
#include <cinttypes>
#include <cstdio>
#include <vector>

static bool same(const cl_digest& a, const cl_digest& b) { return a.reads == b.reads && a.symbols == b.symbols && a.sum == b.sum; }

int main(int argc, char** argv)
{
	if (argc != 2) { fprintf(stderr, "usage: qual_values_host_test FILE\n"); return 2; }
	FILE* f = fopen(argv[1], "rb");
	if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
	uint64_t n_cases = 0;
	if (fread(&n_cases, 8, 1, f) != 1) return 2;
	for (uint64_t c = 0; c < n_cases; ++c)
	{
		cl_qual_params P{}; uint64_t first = 0, n = 0;
		if (fread(&P.mode, 4, 1, f) != 1 || fread(&P.n_fwd, 4, 1, f) != 1 || fread(P.fwd, 4, 8, f) != 8 || fread(&P.n_rev, 4, 1, f) != 1 || fread(P.rev, 4, 8, f) != 8) return 2;
		if (fread(&first, 8, 1, f) != 1 || fread(&n, 8, 1, f) != 1) return 2;
		P.level = 1;
		std::vector<uint64_t> off(n + 1);
		if (fread(off.data(), 8, n + 1, f) != n + 1) return 2;
		std::vector<uint8_t> in(off[n]), out(off[n]);                             // exactly the bytes: one past them is the sanitizer's to report
		if (off[n] && fread(in.data(), 1, off[n], f) != off[n]) return 2;
		cl_digest whole{ 0, 0, 0 }, again{ 0, 0, 0 };
		if (!dg_qual_values_host(&P, in.data(), off.data(), n, out.data(), first, &whole)) { fprintf(stderr, "case %" PRIu64 ": refused\n", c); return 1; }
		if (!dg_qual_ascii_host(out.data(), off.data(), n, first, &again) || !same(whole, again)) { fprintf(stderr, "case %" PRIu64 ": the digest of the values differs\n", c); return 1; }
		for (uint64_t cut = 0; cut <= n; ++cut)
		{
			cl_digest two{ 0, 0, 0 }, three{ 0, 0, 0 };
			if (!dg_qual_values_host(&P, in.data(), off.data() + cut, n - cut, nullptr, first + cut, &two) || !dg_qual_values_host(&P, in.data(), off.data(), cut, nullptr, first, &two) || !same(whole, two)) { fprintf(stderr, "case %" PRIu64 ": split at %" PRIu64 " differs\n", c, cut); return 1; }
			if (!dg_qual_ascii_host(out.data(), off.data(), cut, first, &three) || !dg_qual_ascii_host(out.data(), off.data() + cut, n - cut, first + cut, &three) || !same(whole, three)) { fprintf(stderr, "case %" PRIu64 ": split at %" PRIu64 " differs\n", c, cut); return 1; }
		}
		printf("case reads=%" PRIu64 " symbols=%" PRIu64 " sum=0x%016" PRIx64 " values=", whole.reads, whole.symbols, whole.sum);
		for (uint8_t v : out) printf("%02x", v);
		printf("\n");
	}
	fclose(f);
	// what the layout refuses: *-fix without a -D value for every bin, a -D value that does not fit the byte, mode none, indices from 2^63
	cl_qual_params P{}; P.mode = 6; P.level = 1; P.n_fwd = 1; P.fwd[0] = 7; P.n_rev = 1; P.rev[0] = 1;
	DigestValueLayout V; cl_digest d{ 0, 0, 0 }; const uint64_t off1[2] = { 0, 0 };
	if (dg_value_layout(&P, V)) { fprintf(stderr, "2-fix with one -D value was accepted\n"); return 1; }
	P.n_rev = 2; P.rev[1] = 223;
	if (dg_value_layout(&P, V)) { fprintf(stderr, "a -D value of 223 was accepted\n"); return 1; }
	P.rev[1] = 222;
	if (!dg_value_layout(&P, V)) { fprintf(stderr, "a -D value of 222 was refused\n"); return 1; }
	P.mode = 8; P.n_fwd = 0;
	if (dg_value_layout(&P, V)) { fprintf(stderr, "mode none was accepted\n"); return 1; }
	if (dg_qual_ascii_host(nullptr, off1, 1, 1ULL << 63, &d) || !dg_qual_ascii_host(nullptr, off1, 1, (1ULL << 63) - 1, &d)) { fprintf(stderr, "range check\n"); return 1; }
	printf("ok: %" PRIu64 " cases\n", n_cases);
	return 0;
}
