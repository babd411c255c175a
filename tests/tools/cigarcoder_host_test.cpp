// cigarcoder_host_test.cpp — the coded CIGARs on the host (csrc/cigar_coder.hpp: the host twin cgc_pack_host, the decoder cgc_unpack over
// hostrc::RangeDec) and the reader of `hipcigars` version 2 (csrc/cli/cigars_stream.hpp) as a stand-alone program (own main, nothing
// preloaded, no HIP), for a build under AddressSanitizer and UBSan (tests/test_cigarcoder_cpu.py builds and runs it):
//   cigarcoder_host_test FILE
// FILE: u64 n_cases, per case u32 part_ops, u32 seg_ops, u64 n, the n words; then u64 n_bad, per entry u64 n, the n bytes of a corrupted
// segment.  Per case: the segments (printed in hex; a word that is no operation: the refusal with its index, and nothing appended), decoded
// back to the words; every prefix of a small case's bytes and every single-byte change of it goes through the decoder, which must refuse or
// decode and never read outside (the sanitizer's to report) — a prefix that is no whole number of segments must be refused.  Per corrupted
// segment: the refusal's code.  Last: one record's CIGAR through the version-2 stream and its reader, and refusals of the reader.
#include "../../colord_amd/csrc/cli/cigars_stream.hpp"
#include <cinttypes>

static int stream_check()
{
	// one record: 10= 1X 300= 2I 5= 1D 7=  (read 0 .. 325, target 100 .. 424)
	const uint32_t op[] = { CG_EQ, CG_X, CG_EQ, CG_I, CG_EQ, CG_D, CG_EQ }, len[] = { 10, 1, 300, 2, 5, 1, 7 };
	std::vector<uint32_t> ops;
	for (int i = 0; i < 7; ++i) ops.push_back(len[i] << 4 | op[i]);
	MappingSet M; M.seq_len = { 1000 };
	cl_overlap o{}; o.q = 0; o.t = 0; o.qlen = 330; o.qs = 0; o.qe = 325; o.ts = 100; o.te = 424; o.matches = 322; o.subst = 1; o.flags = OV_GENOME | OV_MAIN;
	M.recs.push_back(o);
	std::vector<uint8_t> seg; uint64_t bad = 0, esc = 0;
	if (!cgc_pack_host(ops.data(), ops.size(), 2, 4, seg, &bad, &esc) || esc != 1) return 1;
	const std::vector<uint8_t> v2 = CigarSet::pack_coded({ 7 }, seg, 7, 2);
	CigarSet G;
	if (!G.unpack(v2, M) || G.ops != ops || G.version != 2 || G.coded_segments != 2 || G.coded_escapes != 1 || G.coded_bytes != seg.size()) return 2;
	if (G.text(0, false) != "10=1X300=2I5=1D7=") return 3;
	CigarSet V1; V1.rec_ops = { 7 }; V1.ops = ops;
	CigarSet B;
	if (!B.unpack(V1.pack(), M) || B.ops != ops || B.version != 1) return 4;      // version 1 still reads, into the same set
	std::vector<uint8_t> t;
	t = v2; t[24] = 3; if (G.unpack(t, M)) return 5;                                // another segment count
	t = v2; t[16] = 8; if (G.unpack(t, M)) return 6;                                // another operation count
	t = v2; t[32] ^= 1; if (G.unpack(t, M)) return 7;                               // segment bytes the stream does not hold
	t = v2; t.pop_back(); if (G.unpack(t, M)) return 8;
	t = v2; t[CigarSet::HEAD_CODED] = 6; if (G.unpack(t, M)) return 9;              // the record's count against the operations
	for (size_t i = 0; i < v2.size(); ++i) { t = v2; t[i] ^= 0x40; (void)G.unpack(t, M); }      // (any answer, inside the bytes)
	o.qe = 324; M.recs[0] = o; if (G.unpack(v2, M)) return 10;                      // decoded, then held against the mapping record as before
	return 0;
}

int main(int argc, char** argv)
{
	if (argc != 2) { fprintf(stderr, "usage: cigarcoder_host_test FILE\n"); return 2; }
	FILE* f = fopen(argv[1], "rb");
	if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
	uint64_t n_cases = 0, n_bad = 0;
	if (fread(&n_cases, 8, 1, f) != 1) return 2;
	for (uint64_t c = 0; c < n_cases; ++c)
	{
		uint32_t knobs[2]; uint64_t n = 0;
		if (fread(knobs, 4, 2, f) != 2 || fread(&n, 8, 1, f) != 1) return 2;
		std::vector<uint32_t> w(n);                                              // exactly the words: one past them is the sanitizer's to report
		if (n && fread(w.data(), 4, n, f) != n) return 2;
		std::vector<uint8_t> out = { 0x5a, 0x5a };                               // something in the output already
		uint64_t bad = 0, esc = 0;
		if (!cgc_pack_host(w.data(), n, knobs[0], knobs[1], out, &bad, &esc))
		{
			if (out != std::vector<uint8_t>{ 0x5a, 0x5a }) { fprintf(stderr, "case %" PRIu64 ": a refused call changed the output\n", c); return 1; }
			printf("case refused word %" PRIu64 "\n", bad);
			continue;
		}
		out.erase(out.begin(), out.begin() + 2);
		std::vector<uint8_t> exact(out);                                         // (capacity = size)
		std::vector<uint32_t> back = { 77 }; uint64_t n_seg = 0, n_esc = 0;
		if (cgc_unpack(exact.data(), exact.size(), back, &n_seg, &n_esc) != CGC_OK || back.size() != n + 1 || !std::equal(w.begin(), w.end(), back.begin() + 1) || n_esc != esc)
		{ fprintf(stderr, "case %" PRIu64 ": the segments do not decode to the words\n", c); return 1; }
		if (exact.size() <= 1600)
		{
			uint64_t whole = 0;
			for (size_t cut = 0; cut < exact.size(); ++cut)
			{
				std::vector<uint8_t> p(exact.begin(), exact.begin() + cut);
				std::vector<uint32_t> got;
				const uint32_t r = cgc_unpack(p.data(), p.size(), got);
				if (r == CGC_OK) { ++whole; if (got.size() > n || !std::equal(got.begin(), got.end(), w.begin())) { fprintf(stderr, "case %" PRIu64 ": a prefix of %zu bytes decodes to other words\n", c, cut); return 1; } }
			}
			if (whole > n_seg) { fprintf(stderr, "case %" PRIu64 ": %" PRIu64 " prefixes decode, there are %" PRIu64 " segments\n", c, whole, n_seg); return 1; }
			for (size_t i = 0; i < exact.size(); ++i)
				for (uint8_t x : { (uint8_t)0x01, (uint8_t)0x80, (uint8_t)0xff })
				{
					std::vector<uint8_t> p(exact); p[i] ^= x;
					std::vector<uint32_t> got = { 5 };
					if (cgc_unpack(p.data(), p.size(), got) != CGC_OK && got != std::vector<uint32_t>{ 5 }) { fprintf(stderr, "case %" PRIu64 ": a refusal changed the output\n", c); return 1; }
				}
		}
		printf("case ");
		for (uint8_t b : exact) printf("%02x", b);
		printf("\n");
	}
	if (fread(&n_bad, 8, 1, f) != 1) return 2;
	for (uint64_t c = 0; c < n_bad; ++c)
	{
		uint64_t n = 0;
		if (fread(&n, 8, 1, f) != 1) return 2;
		std::vector<uint8_t> b(n);
		if (n && fread(b.data(), 1, n, f) != n) return 2;
		std::vector<uint32_t> got;
		const uint32_t r = cgc_unpack(b.data(), b.size(), got);
		if (r != CGC_OK && !got.empty()) return 1;
		printf("bad %u %s\n", r, cgc_refusal_text(r));
	}
	fclose(f);
	if (const int r = stream_check()) { fprintf(stderr, "the version-2 stream: check %d failed\n", r); return 1; }
	printf("stream ok\nok: %" PRIu64 " cases, %" PRIu64 " corrupted segments\n", n_cases, n_bad);
	return 0;
}
