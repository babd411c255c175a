// digest_stream.hpp — the `hipdigest` stream of an archive: the content digests of the input, made at compress time
// (`colord_hip compress-* --digest`: dna and qual on the device, header on the host) and checked by `colord_hip decompress` / `check`
// against what the decoders return.  One part, little-endian.  Version 1, 80 bytes: u32 version = 1, u32 flags (bit 0 dna, bit 1 qual, bit 2
// header), then the triples reads / symbols / sum of dna, qual, header (zeroes where the flag is off).  Version 2, 104 bytes, written only with
// --digest-values: u32 version = 2, u32 flags (bit 3 = qual-values), the same three triples, then the triple of qual-values.  The reference's
// decompressor finds its streams by name and never sees this one.
#pragma once
#include "archive.hpp"
#include "../digest.hpp"

struct DigestSet {
	uint32_t flags = 0; cl_digest d[4] = { { 0, 0, 0 }, { 0, 0, 0 }, { 0, 0, 0 }, { 0, 0, 0 } };      // dna, qual, header, qual-values
	static const char* name(int i) { static const char* const n[4] = { "dna", "qual", "header", "qual-values" }; return n[i]; }
	static int in_order(int j) { static const int o[4] = { 0, 1, 3, 2 }; return o[j]; }           // as messages list them: qual-values next to qual
	void add(int i, const cl_digest& x) { d[i].reads += x.reads; d[i].symbols += x.symbols; d[i].sum += x.sum; }
	std::vector<uint8_t> pack() const
	{
		std::vector<uint8_t> v;
		auto le = [&](uint64_t x, int n) { for (int i = 0; i < n; ++i) v.push_back((uint8_t)(x >> (8 * i))); };
		const bool v2 = (flags >> 3) & 1;                                         // version 1 whenever there is no qual-values digest
		le(v2 ? 2 : 1, 4); le(flags, 4);
		for (int i = 0; i < (v2 ? 4 : 3); ++i) { const bool on = (flags >> i) & 1; le(on ? d[i].reads : 0, 8); le(on ? d[i].symbols : 0, 8); le(on ? d[i].sum : 0, 8); }
		return v;
	}
	bool unpack(const std::vector<uint8_t>& v)
	{
		if (v.size() != 80 && v.size() != 104) return false;
		auto le = [&](size_t at, int n) { uint64_t x = 0; for (int i = 0; i < n; ++i) x |= (uint64_t)v[at + i] << (8 * i); return x; };
		const uint64_t version = le(0, 4);
		if (version != (v.size() == 80 ? 1u : 2u)) return false;
		const int n = version == 1 ? 3 : 4;
		flags = (uint32_t)le(4, 4) & (version == 1 ? 7u : 15u);
		for (int i = 0; i < 4; ++i) d[i] = i < n ? cl_digest{ le(8 + 24 * i, 8), le(16 + 24 * i, 8), le(24 + 24 * i, 8) } : cl_digest{ 0, 0, 0 };
		return true;
	}
	std::string line(int i) const
	{
		char b[160]; snprintf(b, sizeof(b), "%s reads=%llu symbols=%llu sum=0x%016llx", name(i), (unsigned long long)d[i].reads, (unsigned long long)d[i].symbols, (unsigned long long)d[i].sum);
		return b;
	}
	std::string names() const { std::string s; for (int j = 0; j < 4; ++j) { const int i = in_order(j); if ((flags >> i) & 1) { if (!s.empty()) s += ", "; s += name(i); } } return s; }
};
// the stored digests of an archive: 0 none, 1 read, -1 a `hipdigest` stream this build cannot read
inline int read_hipdigest(const std::string& path, DigestSet& out)
{
	ArchiveReader ar;
	if (!ar.open(path)) return 0;                                              // (the decoder reports what is wrong with the file)
	const int s = ar.id("hipdigest");
	std::vector<uint8_t> b; uint64_t meta = 0; int r = 0;
	if (s >= 0) r = ar.part(s, 0, b, meta) && out.unpack(b) ? 1 : -1;
	ar.close();
	return r;
}
// the streams of `stored` that `computed` does not confirm, each with both triples; empty: every stored digest is confirmed
inline std::string digest_mismatch(const DigestSet& stored, const DigestSet& computed)
{
	std::string msg;
	for (int j = 0; j < 4; ++j)
	{
		const int i = DigestSet::in_order(j);
		if (!((stored.flags >> i) & 1)) continue;
		const cl_digest& a = stored.d[i]; const cl_digest& b = computed.d[i];
		if (((computed.flags >> i) & 1) && a.reads == b.reads && a.symbols == b.symbols && a.sum == b.sum) continue;
		msg += std::string(msg.empty() ? "" : "; ") + "stored " + stored.line(i) + ", computed " + computed.line(i);
	}
	return msg;
}
