// digest_stream.hpp — the `hipdigest` stream of an archive: the content digests of the input, made at compress time
// (`colord_hip compress-* --digest`: dna and qual on the device, header on the host) and checked by `colord_hip decompress` / `check`
// against what the decoders return.  One part of 80 bytes, little-endian: u32 version = 1, u32 flags (bit 0 dna, bit 1 qual, bit 2
// header), then the triples reads / symbols / sum of dna, qual, header (zeroes where the flag is off).  The reference's decompressor
// finds its streams by name and never sees this one.
#pragma once
#include "archive.hpp"
#include "../digest.hpp"

struct DigestSet {
	uint32_t flags = 0; cl_digest d[3] = { { 0, 0, 0 }, { 0, 0, 0 }, { 0, 0, 0 } };      // dna, qual, header
	static const char* name(int i) { static const char* const n[3] = { "dna", "qual", "header" }; return n[i]; }
	void add(int i, const cl_digest& x) { d[i].reads += x.reads; d[i].symbols += x.symbols; d[i].sum += x.sum; }
	std::vector<uint8_t> pack() const
	{
		std::vector<uint8_t> v;
		auto le = [&](uint64_t x, int n) { for (int i = 0; i < n; ++i) v.push_back((uint8_t)(x >> (8 * i))); };
		le(1, 4); le(flags, 4);
		for (int i = 0; i < 3; ++i) { const bool on = (flags >> i) & 1; le(on ? d[i].reads : 0, 8); le(on ? d[i].symbols : 0, 8); le(on ? d[i].sum : 0, 8); }
		return v;
	}
	bool unpack(const std::vector<uint8_t>& v)
	{
		if (v.size() != 80) return false;
		auto le = [&](size_t at, int n) { uint64_t x = 0; for (int i = 0; i < n; ++i) x |= (uint64_t)v[at + i] << (8 * i); return x; };
		if (le(0, 4) != 1) return false;
		flags = (uint32_t)le(4, 4) & 7u;
		for (int i = 0; i < 3; ++i) d[i] = cl_digest{ le(8 + 24 * i, 8), le(16 + 24 * i, 8), le(24 + 24 * i, 8) };
		return true;
	}
	std::string line(int i) const
	{
		char b[160]; snprintf(b, sizeof(b), "%s reads=%llu symbols=%llu sum=0x%016llx", name(i), (unsigned long long)d[i].reads, (unsigned long long)d[i].symbols, (unsigned long long)d[i].sum);
		return b;
	}
	std::string names() const { std::string s; for (int i = 0; i < 3; ++i) if ((flags >> i) & 1) { if (!s.empty()) s += ", "; s += name(i); } return s; }
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
	for (int i = 0; i < 3; ++i)
	{
		if (!((stored.flags >> i) & 1)) continue;
		const cl_digest& a = stored.d[i]; const cl_digest& b = computed.d[i];
		if (((computed.flags >> i) & 1) && a.reads == b.reads && a.symbols == b.symbols && a.sum == b.sum) continue;
		msg += std::string(msg.empty() ? "" : "; ") + "stored " + stored.line(i) + ", computed " + computed.line(i);
	}
	return msg;
}
