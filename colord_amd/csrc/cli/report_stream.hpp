// report_stream.hpp — the `hipreport` stream of an archive: what the archive holds and what the quality mode changed,
// counted on the device from the INPUT at compress time (`colord_hip compress-* --report`), printed by `colord_hip info [--report
// [--json]]` without decoding anything and compared by `decompress` / `check` with what they decode.  One part, little-endian:
//   u32 version = 1, u32 flags (bit 0: quality part present),
//   reads, bases, base_count[5] (A C G T N), len_min, len_max, n50, n90, len_hist[33], len_bases[33]          (u64 each)
//   with bit 0: q_reads, q_symbols, mean_q_hist[96] (u64), u32 n_cells, the non-zero cells of q_joint as (u8 in, u8 out, u64 count),
//   ascending by (in, out)
// N50 / N90 are not additive: the command-line host computes them from all read lengths (rp_nxx).  The reference's decompressor finds
// its streams by name and never sees this one.
#pragma once
#include "archive.hpp"
#include "../report.hpp"
#include <cmath>
#include <memory>

struct ReportSet {
	std::unique_ptr<cl_report> r{ new cl_report }; uint64_t n50 = 0, n90 = 0;
	ReportSet() { rp_clear(r.get()); }
	std::vector<uint8_t> pack() const
	{
		std::vector<uint8_t> v;
		auto le = [&](uint64_t x, int n) { for (int i = 0; i < n; ++i) v.push_back((uint8_t)(x >> (8 * i))); };
		le(1, 4); le(r->has_qual ? 1 : 0, 4);
		le(r->reads, 8); le(r->bases, 8); for (int i = 0; i < 5; ++i) le(r->base_count[i], 8);
		le(r->len_min, 8); le(r->len_max, 8); le(n50, 8); le(n90, 8);
		for (int i = 0; i < 33; ++i) le(r->len_hist[i], 8);
		for (int i = 0; i < 33; ++i) le(r->len_bases[i], 8);
		if (!r->has_qual) return v;
		le(r->q_reads, 8); le(r->q_symbols, 8); for (int i = 0; i < 96; ++i) le(r->mean_q_hist[i], 8);
		uint32_t cells = 0; for (int i = 0; i < 96; ++i) for (int j = 0; j < 96; ++j) cells += r->q_joint[i][j] != 0;
		le(cells, 4);
		for (int i = 0; i < 96; ++i) for (int j = 0; j < 96; ++j) if (r->q_joint[i][j]) { le((uint64_t)i, 1); le((uint64_t)j, 1); le(r->q_joint[i][j], 8); }
		return v;
	}
	// false: another version, a size that does not fit its own counts, a cell outside 96 x 96 or out of order
	bool unpack(const std::vector<uint8_t>& v)
	{
		rp_clear(r.get()); n50 = n90 = 0;
		size_t at = 0; bool ok = true;
		auto le = [&](int n) { uint64_t x = 0; if (v.size() - at < (size_t)n) { ok = false; at = v.size(); return x; } for (int i = 0; i < n; ++i) x |= (uint64_t)v[at + i] << (8 * i); at += n; return x; };
		if (v.size() < 8 + 77 * 8 || le(4) != 1) return false;
		const uint64_t flags = le(4);
		if (flags > 1) return false;
		r->reads = le(8); r->bases = le(8); for (int i = 0; i < 5; ++i) r->base_count[i] = le(8);
		r->len_min = le(8); r->len_max = le(8); n50 = le(8); n90 = le(8);
		for (int i = 0; i < 33; ++i) r->len_hist[i] = le(8);
		for (int i = 0; i < 33; ++i) r->len_bases[i] = le(8);
		if (flags & 1)
		{
			r->has_qual = 1; r->q_reads = le(8); r->q_symbols = le(8); for (int i = 0; i < 96; ++i) r->mean_q_hist[i] = le(8);
			const uint64_t cells = le(4);
			if (!ok || cells > 96 * 96 || v.size() - at != cells * 10) return false;
			int last = -1;
			for (uint64_t c = 0; c < cells; ++c)
			{
				const int i = (int)le(1), j = (int)le(1); const uint64_t n = le(8);
				if (i > 95 || j > 95 || i * 96 + j <= last || !n) return false;
				last = i * 96 + j; r->q_joint[i][j] = n;
			}
		}
		return ok && at == v.size();
	}
	uint64_t out_marginal(int j) const { uint64_t s = 0; for (int i = 0; i < 96; ++i) s += r->q_joint[i][j]; return s; }
	uint64_t in_marginal(int i) const { uint64_t s = 0; for (int j = 0; j < 96; ++j) s += r->q_joint[i][j]; return s; }
};

// the stored report of an archive: 0 none, 1 read, -1 a `hipreport` stream this build cannot read
inline int read_hipreport(const std::string& path, ReportSet& out)
{
	ArchiveReader ar;
	if (!ar.open(path)) return 0;
	const int s = ar.id("hipreport");
	std::vector<uint8_t> b; uint64_t meta = 0; int r = 0;
	if (s >= 0) r = ar.part(s, 0, b, meta) && out.unpack(b) ? 1 : -1;
	ar.close();
	return r;
}
inline std::string rp_num(uint64_t x)                                          // 1 204 331
{
	std::string s = std::to_string(x);
	for (int i = (int)s.size() - 3; i > 0; i -= 3) s.insert((size_t)i, " ");
	return s;
}
// The output side — what a decoder can recompute: reads, bases, base_count, lengths (histogram, min, max, N50, N90) and, with a quality
// part on both sides, q_reads, q_symbols and the OUT marginal — of `stored` against `decoded`: the first field that differs with both
// numbers, or empty.  The IN side of q_joint and mean_q_hist cannot be recomputed from a lossy archive and are not compared.
inline std::string report_mismatch(const ReportSet& stored, const ReportSet& decoded)
{
	const cl_report& a = *stored.r; const cl_report& b = *decoded.r;
	auto diff = [](const std::string& what, uint64_t s, uint64_t d) { return what + ": stored " + rp_num(s) + ", decoded " + rp_num(d); };
	static const char* const base[5] = { "A", "C", "G", "T", "N" };
	if (a.reads != b.reads) return diff("reads", a.reads, b.reads);
	if (a.bases != b.bases) return diff("bases", a.bases, b.bases);
	for (int i = 0; i < 5; ++i) if (a.base_count[i] != b.base_count[i]) return diff(std::string("base count ") + base[i], a.base_count[i], b.base_count[i]);
	if (a.len_min != b.len_min) return diff("shortest read", a.len_min, b.len_min);
	if (a.len_max != b.len_max) return diff("longest read", a.len_max, b.len_max);
	if (stored.n50 != decoded.n50) return diff("N50", stored.n50, decoded.n50);
	if (stored.n90 != decoded.n90) return diff("N90", stored.n90, decoded.n90);
	for (int i = 0; i < 33; ++i) if (a.len_hist[i] != b.len_hist[i]) return diff("reads of length bin " + std::to_string(i), a.len_hist[i], b.len_hist[i]);
	for (int i = 0; i < 33; ++i) if (a.len_bases[i] != b.len_bases[i]) return diff("bases of length bin " + std::to_string(i), a.len_bases[i], b.len_bases[i]);
	if (!a.has_qual) return "";
	if (!b.has_qual) return "quality part: stored, but the archive decodes to no quality values";
	if (a.q_reads != b.q_reads) return diff("reads with qualities", a.q_reads, b.q_reads);
	if (a.q_symbols != b.q_symbols) return diff("quality values", a.q_symbols, b.q_symbols);
	for (int j = 0; j < 96; ++j) if (stored.out_marginal(j) != decoded.out_marginal(j)) return diff("quality value " + std::to_string(j), stored.out_marginal(j), decoded.out_marginal(j));
	return "";
}
// what the quality mode changed, from q_joint alone
struct ReportLoss { double unchanged = 1, mae = 0, rmse = 0; int max_abs = 0; };
inline ReportLoss report_loss(const cl_report& r)
{
	ReportLoss L; long double n = 0, same = 0, ad = 0, sq = 0;
	for (int i = 0; i < 96; ++i) for (int j = 0; j < 96; ++j) if (const uint64_t c = r.q_joint[i][j])
	{
		const int d = i > j ? i - j : j - i;
		n += c; if (!d) same += c; ad += (long double)c * d; sq += (long double)c * d * d; if (d > L.max_abs) L.max_abs = d;
	}
	if (n > 0) { L.unchanged = (double)(same / n); L.mae = (double)(ad / n); L.rmse = (double)sqrtl(sq / n); }
	return L;
}
// `out_only`: a report made from decoded records (check without a stored stream) — no IN side, no loss
inline void print_report(FILE* f, const ReportSet& S, bool out_only)
{
	const cl_report& r = *S.r;
	fprintf(f, "reads: %llu\nbases: %llu\n", (unsigned long long)r.reads, (unsigned long long)r.bases);
	if (r.reads) fprintf(f, "read length: min %llu, max %llu, mean %.1f, N50 %llu, N90 %llu\n", (unsigned long long)r.len_min, (unsigned long long)r.len_max, (double)r.bases / (double)r.reads, (unsigned long long)S.n50, (unsigned long long)S.n90);
	const double nb = r.bases ? (double)r.bases : 1.0;
	fprintf(f, "base composition: A %llu, C %llu, G %llu, T %llu, N %llu; GC %.4f, N %.6f\n", (unsigned long long)r.base_count[0], (unsigned long long)r.base_count[1], (unsigned long long)r.base_count[2],
		(unsigned long long)r.base_count[3], (unsigned long long)r.base_count[4], (double)(r.base_count[1] + r.base_count[2]) / nb, (double)r.base_count[4] / nb);
	fprintf(f, "read lengths (bin = bit length of the length: reads, bases):\n");
	for (int i = 0; i < 33; ++i) if (r.len_hist[i]) fprintf(f, "  %2d  [%llu, %llu]  %llu  %llu\n", i, i ? 1ull << (i - 1) : 0ull, i ? (1ull << i) - 1 : 0ull, (unsigned long long)r.len_hist[i], (unsigned long long)r.len_bases[i]);
	if (!r.has_qual) { fprintf(f, "qualities: none (FASTA input or -q none)\n"); return; }
	fprintf(f, "reads with qualities: %llu, quality values: %llu\n", (unsigned long long)r.q_reads, (unsigned long long)r.q_symbols);
	fprintf(f, out_only ? "quality values (value: decoded):\n" : "quality values (value: input, stored):\n");
	for (int q = 0; q < 96; ++q)
	{
		const uint64_t in = S.in_marginal(q), out = S.out_marginal(q);
		if (out_only) { if (out) fprintf(f, "  %2d  %llu\n", q, (unsigned long long)out); }
		else if (in || out) fprintf(f, "  %2d  %llu  %llu\n", q, (unsigned long long)in, (unsigned long long)out);
	}
	if (out_only) return;
	fprintf(f, "mean quality per read (arithmetic mean of the Phred values, NOT the error-probability mean: reads):\n");
	for (int q = 0; q < 96; ++q) if (r.mean_q_hist[q]) fprintf(f, "  %2d  %llu\n", q, (unsigned long long)r.mean_q_hist[q]);
	const ReportLoss L = report_loss(r);
	fprintf(f, "quality loss: %.6f of the bases unchanged, MAE %.4f, RMSE %.4f, max |delta| %d\n", L.unchanged, L.mae, L.rmse, L.max_abs);
	fprintf(f, "joint cells (input, stored: bases):\n");
	for (int i = 0; i < 96; ++i) for (int j = 0; j < 96; ++j) if (r.q_joint[i][j]) fprintf(f, "  %2d %2d  %llu\n", i, j, (unsigned long long)r.q_joint[i][j]);
}
// the whole stream as one JSON object
inline void print_report_json(FILE* f, const ReportSet& S)
{
	const cl_report& r = *S.r;
	auto arr = [&](const char* name, const uint64_t* p, int n) { fprintf(f, "\"%s\": [", name); for (int i = 0; i < n; ++i) fprintf(f, "%s%llu", i ? ", " : "", (unsigned long long)p[i]); fprintf(f, "]"); };
	fprintf(f, "{\"version\": 1, \"has_qual\": %d, \"reads\": %llu, \"bases\": %llu, ", r.has_qual ? 1 : 0, (unsigned long long)r.reads, (unsigned long long)r.bases);
	arr("base_count", r.base_count, 5);
	fprintf(f, ", \"len_min\": %llu, \"len_max\": %llu, \"n50\": %llu, \"n90\": %llu, ", (unsigned long long)r.len_min, (unsigned long long)r.len_max, (unsigned long long)S.n50, (unsigned long long)S.n90);
	arr("len_hist", r.len_hist, 33); fprintf(f, ", "); arr("len_bases", r.len_bases, 33);
	if (r.has_qual)
	{
		fprintf(f, ", \"q_reads\": %llu, \"q_symbols\": %llu, ", (unsigned long long)r.q_reads, (unsigned long long)r.q_symbols);
		arr("mean_q_hist", r.mean_q_hist, 96);
		const ReportLoss L = report_loss(r);
		fprintf(f, ", \"unchanged\": %.9f, \"mae\": %.9f, \"rmse\": %.9f, \"max_abs\": %d, \"q_joint\": [", L.unchanged, L.mae, L.rmse, L.max_abs);
		bool first = true;
		for (int i = 0; i < 96; ++i) for (int j = 0; j < 96; ++j) if (r.q_joint[i][j]) { fprintf(f, "%s[%d, %d, %llu]", first ? "" : ", ", i, j, (unsigned long long)r.q_joint[i][j]); first = false; }
		fprintf(f, "]");
	}
	fprintf(f, "}\n");
}
