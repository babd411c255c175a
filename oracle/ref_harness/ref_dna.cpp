// ref_dna — the `dna` stream parts of constructed tuple streams from the UNMODIFIED reference coder (TEST INFRASTRUCTURE ONLY).
//
// Includes the reference's dna_coder.h / reference_reads.h from where they lie and links its objects (oracle/Makefile.ref).
// Drives CReferenceReads::Add and CDNACoder::Init / Encode / Finish / GetOutput / Restart exactly as CEntrComprReads does
// (entr_read.h:53,56-80): one coder for all parts, Finish + GetOutput + Restart after the reads of a part.  The tuple streams
// are given in es_t's own byte layout (utils.h:56-273); every tuple is handed to es_t::append, which rebuilds the same bytes.
// What tests/golden/make_dnaruns.py records, and what the oracle's and the device's DNA coders are pinned to.
//
// usage: ref_dna CASE
//   CASE    binary, little-endian: "DNARUNS1", u32 level, u32 max alternatives, u32 start read id,
//           u32 n_refs, n_refs x { u32 len, len bytes of symbols 0..3 },
//           u32 n_reads, n_reads x { u32 tuple count, u32 n_bytes, n_bytes of tuple stream },
//           u32 n_parts, (n_parts + 1) x u32 ascending read bounds, the first 0 and the last n_reads
//   stdout  one line a part: <reads> <bytes> <sha256 of the part's bytes>
#include "utils.h"
#include "reference_reads.h"
#include "dna_coder.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "sha256.hpp"

namespace {
struct In {
	std::vector<uint8_t> b; size_t p = 0;
	void need(size_t n) { if (p + n > b.size()) { fprintf(stderr, "ref_dna: case file ends early\n"); exit(2); } }
	uint32_t u32() { need(4); uint32_t v; memcpy(&v, &b[p], 4); p += 4; return v; }
	const uint8_t* bytes(size_t n) { need(n); const uint8_t* q = &b[p]; p += n; return q; }
};

// the tuples of one stream, through es_t::append (utils.h:161-208)
es_t to_es(const uint8_t* p, uint32_t n_bytes, uint32_t n_tuples)
{
	es_t es;
	const uint8_t* e = p + n_bytes;
	while (p < e)
	{
		const tuple_types t = (tuple_types)(p[0] >> 4);
		switch (t)
		{
		case tuple_types::insertion: case tuple_types::substitution: case tuple_types::plain: es.append(t, p[0] & 0xf, 1); p += 1; break;
		case tuple_types::anchor: case tuple_types::skip:
			es.append(t, 0, (int)(((uint32_t)(p[0] & 0xf) << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3])); p += 4; break;
		case tuple_types::alt_id: case tuple_types::start_es:
			es.append(t, (int)(((uint32_t)p[1] << 24) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 8) | p[4]), p[0] & 0xf); p += 5; break;
		case tuple_types::deletion: case tuple_types::match: case tuple_types::main_ref: case tuple_types::start_plain: case tuple_types::start_plain_with_Ns:
			es.append(t, 0, 0); p += 1; break;
		default: fprintf(stderr, "ref_dna: tuple type %d\n", (int)t); exit(2);
		}
	}
	if (p != e || es.size() != n_tuples || es.raw_size() != n_bytes) { fprintf(stderr, "ref_dna: a stream does not hold its %u tuples in %u bytes\n", n_tuples, n_bytes); exit(2); }
	return es;
}
} // namespace

int main(int argc, char** argv)
{
	if (argc != 2) { fprintf(stderr, "usage: ref_dna CASE\n"); return 2; }
	In in;
	{
		FILE* f = fopen(argv[1], "rb");
		if (!f) { perror("ref_dna"); return 2; }
		uint8_t tmp[1 << 16]; size_t n;
		while ((n = fread(tmp, 1, sizeof(tmp), f)) > 0) in.b.insert(in.b.end(), tmp, tmp + n);
		fclose(f);
	}
	if (memcmp(in.bytes(8), "DNARUNS1", 8) != 0) { fprintf(stderr, "ref_dna: not a case file\n"); return 2; }
	const uint32_t level = in.u32(), max_alt = in.u32(), start_id = in.u32();
	const uint32_t n_refs = in.u32();
	CReferenceReads ref_reads(n_refs);
	for (uint32_t i = 0; i < n_refs; ++i)
	{
		const uint32_t len = in.u32(); const uint8_t* s = in.bytes(len);
		read_t r(s, s + len);
		r.push_back(255);                                   // guard, as every read_t carries (utils.h:372-376)
		ref_reads.Add(r);
	}
	const uint32_t n_reads = in.u32();
	std::vector<es_t> reads; reads.reserve(n_reads);
	for (uint32_t i = 0; i < n_reads; ++i)
	{
		const uint32_t nt = in.u32(), nb = in.u32();
		reads.emplace_back(to_es(in.bytes(nb), nb, nt));
	}
	const uint32_t n_parts = in.u32();
	std::vector<uint32_t> bounds(n_parts + 1);
	for (auto& b : bounds) b = in.u32();
	if (bounds.front() != 0 || bounds.back() != n_reads) { fprintf(stderr, "ref_dna: part bounds do not cover the reads\n"); return 2; }

	entropy_coder::CDNACoder dna_coder(ref_reads, false);
	dna_coder.Init(true, max_alt, (int)level, 0, start_id);                    // entr_read.h:53
	std::vector<uint8_t> v_output;
	for (uint32_t p = 0; p < n_parts; ++p)
	{
		for (uint32_t i = bounds[p]; i < bounds[p + 1]; ++i) dna_coder.Encode(reads[i]);   // :64-67
		dna_coder.Finish();                                                     // :69
		dna_coder.GetOutput(v_output);                                          // :71
		dna_coder.Restart();                                                    // :72
		Sha256 h; h.add(v_output.data(), v_output.size());
		printf("%u %zu %s\n", bounds[p + 1] - bounds[p], v_output.size(), h.hex().c_str());
		v_output.clear();                                                       // :77
	}
	return 0;
}
