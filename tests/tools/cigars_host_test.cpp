// cigars_host_test.cpp — the host twin of the CIGARs (csrc/cigars.hpp: cg_walk_host, the functions it shares with the kernel) and the
// `hipcigars` stream (csrc/cli/cigars_stream.hpp: pack, unpack with its checks, the texts) as a stand-alone program (own main, nothing
// preloaded, no HIP), for a build under AddressSanitizer and UBSan (tests/test_cigars_cpu.py builds and runs it):
//   cigars_host_test FILE ID_LIMIT
// FILE: u32 n_refs, (n_refs + 1) u64 offsets, the reference codes; u64 n_cases, then per case u64 n_reads, (n_reads + 1) u64 offsets, the
// stream bytes.  First the per-run function at its limit, by itself and through the visitor (a run of 2^28 bases inside a record refuses
// the read, the same run behind the last aligned column does not).  Then per case: the CIGARs whole — a refused case must leave the
// outputs as they were, with the read and the code of ov_walk_host — and split in two calls at each read boundary (must be the same);
// every record's operations against its overlap record (cg_check); with ID_LIMIT the counts are 0 exactly for the records on ids at or
// past it and the others keep their operations; the stream packed, unpacked against the records and packed again must be the same bytes,
// and one of another shape or with one broken relation must be refused; prints the stream in hex, or the refusal.
#include "../../colord_amd/csrc/cli/cigars_stream.hpp"
#include <cinttypes>

static int run_limit()
{
	uint32_t w = 0;
	if (!cg_word(CG_D, CG_LEN_MAX, w) || cg_len(w) != CG_LEN_MAX || cg_op(w) != CG_D) return 1;
	if (cg_word(CG_D, CG_LEN_MAX + 1, w) || cg_word(CG_EQ, 1ull << 40, w)) return 2;
	if (!cg_word(CG_X, 1, w) || w != ((1u << 4) | CG_X)) return 3;
	EsHostWalk W; W.cur.id = 0; W.cur.len = 1ull << 40;
	const uint32_t half = 1u << 27;
	{	// = D(2^27) D(2^27) = : the merged run lies inside the record
		CgHostVisitor v{ 0xffffffffu }; v.begin(W);
		v.tuple(W, T_MATCH, 0, 1, 0); v.tuple(W, T_SKIP, 0, half, 255); v.tuple(W, T_SKIP, 0, half, 255); v.tuple(W, T_MATCH, 0, 1, 0);
		if (v.end(W, 10) != CGE_RUN) return 4;
	}
	{	// one base less fits
		CgHostVisitor v{ 0xffffffffu }; v.begin(W);
		v.tuple(W, T_MATCH, 0, 1, 0); v.tuple(W, T_SKIP, 0, half, 255); v.tuple(W, T_SKIP, 0, half - 1, 255); v.tuple(W, T_MATCH, 0, 1, 0);
		if (v.end(W, 10) != EDE_NONE || v.rec_ops != std::vector<uint32_t>{ 3 } || cg_len(v.ops[1]) != CG_LEN_MAX) return 5;
	}
	{	// the same run behind the last aligned column is no part of the record
		CgHostVisitor v{ 0xffffffffu }; v.begin(W);
		v.tuple(W, T_MATCH, 0, 1, 0); v.tuple(W, T_SKIP, 0, half, 255); v.tuple(W, T_SKIP, 0, half, 255);
		if (v.end(W, 10) != EDE_NONE || v.rec_ops != std::vector<uint32_t>{ 1 } || v.ops.size() != 1) return 6;
	}
	{	// an = run of anchors
		CgHostVisitor v{ 0xffffffffu }; v.begin(W);
		v.tuple(W, T_ANCHOR, 0, half, 255); v.tuple(W, T_ANCHOR, 0, 0, 255); v.tuple(W, T_ANCHOR, 0, half, 255);
		if (v.end(W, 10) != CGE_RUN) return 7;
	}
	return 0;
}

int main(int argc, char** argv)
{
	if (argc != 3) { fprintf(stderr, "usage: cigars_host_test FILE ID_LIMIT\n"); return 2; }
	if (const int r = run_limit()) { fprintf(stderr, "the run limit: check %d failed\n", r); return 1; }
	printf("run limit ok\n");
	const uint32_t id_limit = (uint32_t)strtoul(argv[2], nullptr, 10);
	FILE* f = fopen(argv[1], "rb");
	if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
	uint32_t n_refs = 0; uint64_t n_cases = 0;
	if (fread(&n_refs, 4, 1, f) != 1) return 2;
	std::vector<uint64_t> roff((size_t)n_refs + 1);
	if (fread(roff.data(), 8, roff.size(), f) != roff.size()) return 2;
	std::vector<uint8_t> rc(roff[n_refs]);                                     // exactly the bytes: one past them is the sanitizer's to report
	if (!rc.empty() && fread(rc.data(), 1, rc.size(), f) != rc.size()) return 2;
	if (fread(&n_cases, 8, 1, f) != 1) return 2;
	for (uint64_t c = 0; c < n_cases; ++c)
	{
		uint64_t n = 0;
		if (fread(&n, 8, 1, f) != 1) return 2;
		std::vector<uint64_t> off(n + 1);
		if (fread(off.data(), 8, n + 1, f) != n + 1) return 2;
		std::vector<uint8_t> es(off[n]);
		if (off[n] && fread(es.data(), 1, off[n], f) != off[n]) return 2;
		CigarSet whole; whole.rec_ops = { 0x5a5a5a5au }; whole.ops = { 0x5a5a5a5au, 0x5a5a5a5au };      // something in the outputs already
		const std::vector<uint32_t> rec_before = whole.rec_ops, ops_before = whole.ops;
		uint64_t bad = 0, ov_bad = 0; uint32_t code = 0, ov_code = 0;
		MappingSet M;
		const bool ov_ok = ov_walk_host(rc.data(), roff.data(), n_refs, es.data(), off.data(), n, 0, nullptr, 0, M.recs, &ov_bad, &ov_code);
		if (!cg_walk_host(rc.data(), roff.data(), n_refs, es.data(), off.data(), n, 0, whole.rec_ops, whole.ops, &bad, &code))
		{
			if (whole.rec_ops != rec_before || whole.ops != ops_before) { fprintf(stderr, "case %" PRIu64 ": a refused batch changed the outputs\n", c); return 1; }
			if (ov_ok || ov_bad != bad || ov_code != code) { fprintf(stderr, "case %" PRIu64 ": refused as read %" PRIu64 " code %u, the overlaps say %d read %" PRIu64 " code %u\n", c, bad, code, (int)ov_ok, ov_bad, ov_code); return 1; }
			printf("case refused read %" PRIu64 ": %s\n", bad, cg_error_text(code));
			continue;
		}
		if (!ov_ok) { fprintf(stderr, "case %" PRIu64 ": the overlaps refuse what the CIGARs walk\n", c); return 1; }
		whole.rec_ops.erase(whole.rec_ops.begin()); whole.ops.erase(whole.ops.begin(), whole.ops.begin() + 2);
		for (uint64_t cut = 0; cut <= n; cut += n > 64 ? n / 7 + 1 : 1)
		{
			std::vector<uint32_t> r2, o2;
			if (!cg_walk_host(rc.data(), roff.data(), n_refs, es.data(), off.data(), cut, 0, r2, o2, nullptr, nullptr)) return 1;
			if (!cg_walk_host(rc.data(), roff.data(), n_refs, es.data(), off.data() + cut, n - cut, 0, r2, o2, nullptr, nullptr)) return 1;
			if (r2 != whole.rec_ops || o2 != whole.ops) { fprintf(stderr, "case %" PRIu64 ": split at %" PRIu64 " differs\n", c, cut); return 1; }
		}
		// every record against its overlap record; unpack does the same once more
		if (M.recs.size() != whole.rec_ops.size()) { fprintf(stderr, "case %" PRIu64 ": %zu records, %zu counts\n", c, M.recs.size(), whole.rec_ops.size()); return 1; }
		uint64_t at = 0;
		for (size_t i = 0; i < M.recs.size(); ++i)
		{
			if (const uint32_t k = cg_check(M.recs[i], whole.ops.data() + at, whole.rec_ops[i])) { fprintf(stderr, "case %" PRIu64 ": record %zu breaks relation %u\n", c, i, k); return 1; }
			at += whole.rec_ops[i];
		}
		if (id_limit)
		{	// the counts are 0 exactly for the records at or past the limit; the others keep their operations, in their order
			std::vector<uint32_t> rl, ol, want;
			if (!cg_walk_host(rc.data(), roff.data(), n_refs, es.data(), off.data(), n, id_limit, rl, ol, nullptr, nullptr) || rl.size() != M.recs.size()) return 1;
			at = 0;
			for (size_t i = 0; i < M.recs.size(); ++i)
			{
				const bool kept = M.recs[i].t < id_limit;
				if (rl[i] != (kept ? whole.rec_ops[i] : 0u)) { fprintf(stderr, "case %" PRIu64 ": record %zu under the limit\n", c, i); return 1; }
				if (kept) want.insert(want.end(), whole.ops.begin() + at, whole.ops.begin() + at + whole.rec_ops[i]);
				at += whole.rec_ops[i];
			}
			if (ol != want) { fprintf(stderr, "case %" PRIu64 ": the operations under the limit\n", c); return 1; }
		}
		const std::vector<uint8_t> packed = whole.pack();
		CigarSet back;
		if (packed.size() != CigarSet::HEAD + 4 * (whole.rec_ops.size() + whole.ops.size()) || !back.unpack(packed, M) || back.rec_ops != whole.rec_ops || back.ops != whole.ops || back.pack() != packed)
		{ fprintf(stderr, "case %" PRIu64 ": the stream does not round-trip\n", c); return 1; }
		for (size_t i = 0; i < M.recs.size(); ++i) { (void)back.text(i, false); if (back.text(i, true).empty()) return 1; (void)back.edit_distance(i); }
		CigarSet t; std::vector<uint8_t> other = packed, size = packed; other[0] = 2; size[4] = 8;
		bool read_bad = t.unpack(other, M) || t.unpack(size, M) || t.unpack(std::vector<uint8_t>(packed.begin(), packed.begin() + 8), M);
		if (!whole.ops.empty())
		{
			std::vector<uint8_t> flipped = packed; flipped[packed.size() - 4] ^= 0x10;      // the last operation one base longer
			MappingSet fewer = M; fewer.recs.pop_back();
			read_bad = read_bad || t.unpack(std::vector<uint8_t>(packed.begin(), packed.end() - 1), M) || t.unpack(std::vector<uint8_t>(packed.begin(), packed.end() - 4), M) || t.unpack(flipped, M) || t.unpack(packed, fewer);
		}
		if (read_bad) { fprintf(stderr, "case %" PRIu64 ": a stream of another shape was read\n", c); return 1; }
		printf("case ");
		for (uint8_t b : packed) printf("%02x", b);
		printf("\n");
	}
	fclose(f);
	printf("ok: %" PRIu64 " cases\n", n_cases);
	return 0;
}
