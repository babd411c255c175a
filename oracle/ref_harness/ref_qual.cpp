// ref_qual — the `qual` stream parts of constructed read sets from the UNMODIFIED reference coder (TEST INFRASTRUCTURE ONLY).
//
// Includes the reference's quality_coder.h from where it lies and links its objects (oracle/Makefile.ref).  Drives
// CQualityCoder::Init / Encode / Finish / GetOutput / Restart exactly as CEntrComprQuals does (entr_qual.h:68-79,97,114): one coder
// for all parts, Finish + GetOutput + Restart after the reads of a part.  At levels 2 and 3 the per-base class letters of a read
// ('A' inside an anchor, 'M' unit match, ' ' insertion or substitution, 'P' plain read) are turned into an es_t with es_t::append —
// a start tuple, then one anchor a run of 'A', one match an 'M', one insertion a ' ', or start_plain alone — so that the reference's
// own analyze_es (quality_coder_impl.cpp:25-75) makes the letters again.
// What tests/golden/make_qualruns.py records, and what the oracle's and the device's quality coders are pinned to.
//
// usage: ref_qual CASE
//   CASE    binary, little-endian: "QUALRUN1", u32 mode, u32 source, u32 level, u32 n_fwd, n_fwd x u32, u32 n_rev, n_rev x u32,
//           u32 n_reads, n_reads x { u32 len, len bytes of symbols 0..4, len quality bytes (Phred + 33), len class letters },
//           u32 n_parts, (n_parts + 1) x u32 ascending read bounds, the first 0 and the last n_reads
//   stdout  one line a part: <reads> <bytes> <sha256 of the part's bytes>
#include "utils.h"
#include "quality_coder.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "sha256.hpp"

namespace {
struct In {
	std::vector<uint8_t> b; size_t p = 0;
	void need(size_t n) { if (p + n > b.size()) { fprintf(stderr, "ref_qual: case file ends early\n"); exit(2); } }
	uint32_t u32() { need(4); uint32_t v; memcpy(&v, &b[p], 4); p += 4; return v; }
	const uint8_t* bytes(size_t n) { need(n); const uint8_t* q = &b[p]; p += n; return q; }
};

es_t to_es(const uint8_t* letters, uint32_t len)
{
	es_t es;
	bool plain = len == 0;
	for (uint32_t i = 0; i < len; ++i)
	{
		if (letters[i] != 'A' && letters[i] != 'M' && letters[i] != ' ' && letters[i] != 'P') { fprintf(stderr, "ref_qual: class letter %d\n", letters[i]); exit(2); }
		if (letters[i] == 'P') plain = true;
		else if (plain) { fprintf(stderr, "ref_qual: a plain read has the letter P at every base\n"); exit(2); }
	}
	if (plain) { es.append(tuple_types::start_plain, 0, 0); return es; }
	es.append(tuple_types::start_es, 0, 0);
	for (uint32_t i = 0; i < len; )
	{
		if (letters[i] == 'A')
		{
			uint32_t j = i;
			while (j < len && letters[j] == 'A') ++j;
			es.append(tuple_types::anchor, 0, (int)(j - i));
			i = j;
		}
		else if (letters[i] == 'M') { es.append(tuple_types::match, 0, 0); ++i; }
		else { es.append(tuple_types::insertion, 0, 1); ++i; }
	}
	return es;
}
} // namespace

int main(int argc, char** argv)
{
	if (argc != 2) { fprintf(stderr, "usage: ref_qual CASE\n"); return 2; }
	In in;
	{
		FILE* f = fopen(argv[1], "rb");
		if (!f) { perror("ref_qual"); return 2; }
		std::vector<uint8_t> tmp(1 << 16); size_t n;
		while ((n = fread(tmp.data(), 1, tmp.size(), f)) > 0) in.b.insert(in.b.end(), tmp.begin(), tmp.begin() + n);
		fclose(f);
	}
	if (memcmp(in.bytes(8), "QUALRUN1", 8) != 0) { fprintf(stderr, "ref_qual: not a case file\n"); return 2; }
	const uint32_t mode = in.u32(), source = in.u32(), level = in.u32();
	if (mode > 8 || source > 2 || level < 1 || level > 3) { fprintf(stderr, "ref_qual: mode 0..8, source 0..2, level 1..3\n"); return 2; }
	std::vector<uint32_t> fwd(in.u32());
	for (auto& v : fwd) v = in.u32();
	std::vector<uint32_t> rev(in.u32());
	for (auto& v : rev) v = in.u32();
	const uint32_t n_reads = in.u32();
	std::vector<read_t> reads(n_reads); std::vector<qual_t> quals(n_reads); std::vector<es_t> scripts;
	scripts.reserve(n_reads);
	for (uint32_t i = 0; i < n_reads; ++i)
	{
		const uint32_t len = in.u32();
		const uint8_t* s = in.bytes(len); reads[i].assign(s, s + len);
		reads[i].push_back(255);                                // guard, as every read_t carries (utils.h:372-376)
		const uint8_t* q = in.bytes(len); quals[i].assign(q, q + len);
		scripts.emplace_back(to_es(in.bytes(len), len));
	}
	const uint32_t n_parts = in.u32();
	std::vector<uint32_t> bounds(n_parts + 1);
	for (auto& b : bounds) b = in.u32();
	if (bounds.front() != 0 || bounds.back() != n_reads) { fprintf(stderr, "ref_qual: part bounds do not cover the reads\n"); return 2; }

	entropy_coder::CQualityCoder quality_coder(false);
	quality_coder.Init(true, (QualityComprMode)mode, (DataSource)source, fwd, rev, (int)level, 0);   // entr_qual.h:97
	std::vector<uint8_t> v_output;
	for (uint32_t p = 0; p < n_parts; ++p)
	{
		for (uint32_t i = bounds[p]; i < bounds[p + 1]; ++i) quality_coder.Encode(reads[i], quals[i], scripts[i]);   // :114
		quality_coder.Finish();                                                  // :70
		quality_coder.GetOutput(v_output);                                       // :72
		quality_coder.Restart();                                                 // :77
		Sha256 h; h.add(v_output.data(), v_output.size());
		printf("%u %zu %s\n", bounds[p + 1] - bounds[p], v_output.size(), h.hex().c_str());
		v_output.clear();
	}
	return 0;
}
