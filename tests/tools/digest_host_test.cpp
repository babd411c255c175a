// digest_host_test.cpp — the host side of the content digest as a stand-alone program (own main, nothing preloaded), for a build under
// AddressSanitizer and UBSan (tests/test_digest_cpu.py builds and runs it):
//   digest_host_test cases FILE        the host loops of csrc/digest.hpp over cases the test wrote; prints one triple a case
//   digest_host_test decode ARCHIVE    the library's DNA and quality decoders (csrc/decode.hip, compiled for the host into this program) over
//                                      every part of an archive, the quality decoder digesting what it decodes; prints the dna and qual triples
// FILE: u64 n_cases, then per case u32 kind (0 = bases, else the kind of a byte digest), u64 first_read, u64 n_reads, (n_reads + 1) u64
// offsets, the bytes.  Every case is run once whole and once split in two calls at each read boundary (additivity).
#include "../../colord_amd/csrc/decode.hip"
#include "../../colord_amd/csrc/cli/reader.hpp"
#include <cinttypes>

static void print(const char* what, const cl_digest& d) { printf("%s reads=%" PRIu64 " symbols=%" PRIu64 " sum=0x%016" PRIx64 "\n", what, d.reads, d.symbols, d.sum); }
static bool same(const cl_digest& a, const cl_digest& b) { return a.reads == b.reads && a.symbols == b.symbols && a.sum == b.sum; }

static int run_cases(const char* path)
{
	FILE* f = fopen(path, "rb");
	if (!f) { fprintf(stderr, "cannot open %s\n", path); return 2; }
	uint64_t n_cases = 0;
	if (fread(&n_cases, 8, 1, f) != 1) return 2;
	for (uint64_t c = 0; c < n_cases; ++c)
	{
		uint32_t kind = 0; uint64_t first = 0, n = 0;
		if (fread(&kind, 4, 1, f) != 1 || fread(&first, 8, 1, f) != 1 || fread(&n, 8, 1, f) != 1) return 2;
		std::vector<uint64_t> off(n + 1);
		if (fread(off.data(), 8, n + 1, f) != n + 1) return 2;
		std::vector<uint8_t> bytes(off[n]);                                      // exactly the bytes: a read past the last one is the sanitizer's to report
		if (off[n] && fread(bytes.data(), 1, off[n], f) != off[n]) return 2;
		auto run = [&](uint64_t r0, uint64_t r1, cl_digest* acc) {
			return kind == 0 ? dg_bases_host(bytes.data(), off.data() + r0, r1 - r0, first + r0, acc) : dg_bytes_host(kind, bytes.data(), off.data() + r0, r1 - r0, first + r0, acc);
		};
		cl_digest whole{ 0, 0, 0 };
		if (!run(0, n, &whole)) { fprintf(stderr, "case %" PRIu64 ": refused\n", c); return 1; }
		for (uint64_t cut = 0; cut <= n; ++cut)
		{
			cl_digest two{ 0, 0, 0 };
			if (!run(cut, n, &two) || !run(0, cut, &two) || !same(whole, two)) { fprintf(stderr, "case %" PRIu64 ": split at %" PRIu64 " differs\n", c, cut); return 1; }
		}
		print("case", whole);
	}
	fclose(f);
	// the range of read indices: first_read + n stays below 2^63
	cl_digest d{ 0, 0, 0 }; const uint64_t off1[2] = { 0, 0 };
	if (dg_bases_host(nullptr, off1, 1, (1ULL << 63), &d) || dg_bytes_host(DG_HEADER, nullptr, off1, 1, ~0ULL, &d) || !dg_bases_host(nullptr, off1, 1, (1ULL << 63) - 1, &d)) { fprintf(stderr, "range check\n"); return 1; }
	printf("ok: %" PRIu64 " cases\n", n_cases);
	return 0;
}

// one model domain, no reference genome: the golden archives of the quality modes
static int run_decode(const char* path)
{
	using namespace colord_hip_reader;
	ArchiveReader ar;
	if (!ar.open(path)) { fprintf(stderr, "cannot open %s\n", path); return 2; }
	const int s_dna = ar.id("dna"), s_qual = ar.id("qual"), s_meta = ar.id("meta");
	std::vector<uint8_t> mb, in; uint64_t mm = 0;
	if (s_dna < 0 || s_qual < 0 || s_meta < 0 || !ar.part(s_meta, 0, mb, mm)) return 2;
	const Meta M = parse_meta(mb, true);
	if (M.genome || ar.id("hipdomains") >= 0) return 2;
	cl_dna_decoder* d = nullptr; cl_qual_decoder* q = nullptr;
	if (cl_dna_decoder_create(M.max_candidates, M.level, 0, 0, M.ref_mode == 0, M.sparse_range, M.sparse_exp, &d) != CL_OK) return 2;
	cl_qual_params qp{}; qp.mode = M.qual_mode; qp.source = M.source; qp.level = M.level; qp.n_rev = (uint32_t)M.rev.size();
	for (size_t i = 0; i < M.rev.size(); ++i) qp.rev[i] = M.rev[i];
	if (cl_qual_decoder_create(&qp, &q) != CL_OK) return 2;
	cl_digest zero{ 1, 1, 1 };
	if (cl_qual_decoder_digest(q, &zero) != CL_OK || zero.reads || zero.symbols || zero.sum) return 1;      // off by default: zeroes
	const uint64_t first = 1ULL << 33;
	if (cl_qual_decoder_set_digest(q, 1, first) != CL_OK || cl_qual_decoder_set_digest(q, 1, 1ULL << 63) == CL_OK) return 1;
	cl_digest dna{ 0, 0, 0 }; uint64_t g = first;
	for (size_t p = 0; p < ar.n_parts(s_dna); ++p)
	{
		uint64_t n_reads = 0, got = 0;
		if (!ar.part(s_dna, p, in, n_reads)) return 2;
		std::vector<uint64_t> off(n_reads + 1); std::vector<uint8_t> bases(1);
		cl_status s = cl_dna_decode_part(d, in.data(), in.size(), (uint32_t)n_reads, bases.data(), 0, off.data(), &got);
		if (s == CL_E_CAPACITY) { bases.resize(got); s = cl_dna_decode_part(d, in.data(), in.size(), (uint32_t)n_reads, bases.data(), got, off.data(), &got); }   // exactly the bases
		if (s != CL_OK) return 1;
		if (!dg_bases_host(bases.data(), off.data(), n_reads, g, &dna)) return 1;
		g += n_reads;
		if (!ar.part(s_qual, p, in, mm)) return 2;
		std::vector<uint8_t> quals(got);
		if (cl_qual_decode_part(q, in.data(), in.size(), bases.data(), off.data(), (uint32_t)n_reads, quals.data()) != CL_OK) return 1;
	}
	cl_digest qd{ 0, 0, 0 };
	if (cl_qual_decoder_digest(q, &qd) != CL_OK) return 1;
	print("dna", dna); print("qual", qd);
	cl_qual_decoder_free(q); cl_dna_decoder_free(d); ar.close();
	printf("ok: decoded\n");
	return 0;
}

int main(int argc, char** argv)
{
	if (argc == 3 && std::string(argv[1]) == "cases") return run_cases(argv[2]);
	if (argc == 3 && std::string(argv[1]) == "decode") return run_decode(argv[2]);
	fprintf(stderr, "usage: digest_host_test cases FILE | decode ARCHIVE\n");
	return 2;
}
