// The cases of the coded-part check (csrc/rc_check.hpp), shared by the CPU program (rc_check_host_test.cpp: the host loop over
// rc_check_step) and the GPU program (rc_check_test.hip: k_range_check).  The JUDGE of every case is the oracle's decoder (oracle/rc.h:
// orc_rcd_start / _cum / _update, the restatement of sub_rc.h:216-392 that the CPU suite pins to the reference's streams): a part is
// handed to it followed by 16 zero bytes, so that bytes it asks for beyond the part count and `pos` can be compared with the stored size.
// Test infrastructure only.
#pragma once
extern "C" {
#include "../../oracle/rc.h"
}
#include <cstdio>
#include <functional>
#include <random>
#include <vector>

namespace rcc {
typedef uint64_t trip_t;
constexpr uint32_t DECODES = 0xffffffffu;
inline uint32_t t_tot(trip_t t) { return (uint32_t)(t & 0x1fffff); }
inline uint32_t t_freq(trip_t t) { return (uint32_t)((t >> 21) & 0x1fffff); }
inline uint32_t t_cum(trip_t t) { return (uint32_t)(t >> 42); }
inline trip_t t_pack(uint32_t cum, uint32_t freq, uint32_t tot) { return ((uint64_t)cum << 42) | ((uint64_t)freq << 21) | tot; }

// 150 parts in three groups of the coder's layout: 64 parts that all have three whole rounds and more (a few hundred to `typical`
// symbols, one of `longest`), 64 empty parts, and a ragged group of 22 with the round and triple-round edges.
// Totals as in rc_kernel_test.hip: the whole 21-bit range, the models' usual ones, and the extremes in parts of their own.
inline std::vector<std::vector<trip_t>> make_parts(uint32_t longest, uint32_t typical, std::mt19937_64& rng)
{
	std::vector<uint32_t> len;
	for (uint32_t i = 0; i < 64; ++i) len.push_back(i == 5 ? longest : 50 + (uint32_t)(rng() % typical));
	for (uint32_t i = 0; i < 64; ++i) len.push_back(0);
	const uint32_t edges[12] = { 0, 1, 2, 7, 8, 9, 23, 24, 25, 47, 48, 49 };
	for (uint32_t i = 0; i < 22; ++i) len.push_back(i < 12 ? edges[i] : 100 + (uint32_t)(rng() % typical));
	std::vector<std::vector<trip_t>> parts(len.size());
	for (size_t p = 0; p < len.size(); ++p)
		for (uint32_t i = 0; i < len[p]; ++i)
		{
			uint32_t tot = (rng() & 1) ? (uint32_t)(rng() % ((1u << 21) - 1)) + 1 : (uint32_t)(rng() % 60000) + 1000;
			if (p % 10 == 4) { const uint32_t ex[6] = { 1, 2, 3, 1u << (1 + rng() % 20), (1u << 21) - 1, (1u << 21) - 2 }; tot = ex[rng() % 6]; }
			const uint32_t freq = (rng() % 4 == 0) ? 1 : (uint32_t)(rng() % tot) + 1, cum = (uint32_t)(rng() % (tot - freq + 1));
			parts[p].push_back(t_pack(cum, freq, tot));
		}
	return parts;
}

inline std::vector<uint8_t> oracle_code(const std::vector<trip_t>& sy)
{
	orc_bytes ob{ nullptr, 0, 0 }; orc_rce e; e.out = &ob;
	orc_rce_start(&e);
	for (const trip_t t : sy) orc_rce_encode(&e, t_freq(t), t_cum(t), t_tot(t));
	orc_rce_end(&e);
	std::vector<uint8_t> out(ob.p, ob.p + ob.n);
	free(ob.p);
	return out;
}

// what the check must answer for a part of `size` bytes at p: the first symbol whose decoded value lies outside [cum, cum + freq),
// else the number of symbols if the decoder did not consume exactly `size` bytes, else DECODES
inline uint32_t judge(const std::vector<trip_t>& sy, const uint8_t* p, uint64_t size)
{
	std::vector<uint8_t> in(p, p + size);
	in.resize(size + 16, 0);
	orc_rcd d{}; d.in = in.data(); d.n = in.size(); d.pos = 0;
	orc_rcd_start(&d);
	for (size_t i = 0; i < sy.size(); ++i)
	{
		const uint64_t v = orc_rcd_cum(&d, t_tot(sy[i]));
		if (v < t_cum(sy[i]) || v >= (uint64_t)t_cum(sy[i]) + t_freq(sy[i])) return (uint32_t)i;
		orc_rcd_update(&d, t_freq(sy[i]), t_cum(sy[i]));
	}
	return d.pos != size ? (uint32_t)sy.size() : DECODES;
}

// the parts back to back, at whatever alignment their sizes give (+ slack bytes that belong to no part)
struct Packed { std::vector<uint8_t> bytes; std::vector<uint64_t> off, size; };
inline Packed pack(const std::vector<std::vector<uint8_t>>& coded)
{
	Packed P;
	P.bytes.assign(3, 0x5a);
	for (const auto& c : coded) { P.off.push_back(P.bytes.size()); P.size.push_back(c.size()); P.bytes.insert(P.bytes.end(), c.begin(), c.end()); }
	P.bytes.resize(P.bytes.size() + 16, 0x5a);
	return P;
}

// checker: (parts' triples, bytes, n_bytes, part_off, part_size) -> first_bad per part
typedef std::function<std::vector<uint32_t>(const std::vector<std::vector<trip_t>>&, const std::vector<uint8_t>&, uint64_t, const std::vector<uint64_t>&, const std::vector<uint64_t>&)> Checker;

// runs the cases (a)-(g); returns the number of differences (printed)
inline int run_cases(const std::vector<std::vector<trip_t>>& parts, const Packed& clean, const Checker& check, std::mt19937_64& rng)
{
	const size_t np = parts.size();
	int bad = 0;
	// must_be_bad: a condition on the test's INPUTS — the oracle itself has to report every injected corruption
	auto run = [&](const char* name, const std::vector<std::vector<trip_t>>& ps, const Packed& P, uint64_t n_bytes, const std::vector<int>& injected, const std::vector<int>& invalid)
	{
		std::vector<uint32_t> want(np);
		for (size_t p = 0; p < np; ++p)
		{
			const bool placed = P.size[p] != ~0ULL && P.size[p] >= 8 && P.off[p] <= n_bytes && P.size[p] <= n_bytes - P.off[p];
			if (!invalid.empty() && invalid[p] && placed) { printf("%s: part %zu was to be out of place\n", name, p); ++bad; }
			want[p] = placed ? judge(ps[p], P.bytes.data() + P.off[p], P.size[p]) : 0;
			if (placed && !injected.empty() && injected[p] && want[p] == DECODES) { printf("%s: the oracle does not see the corruption injected into part %zu (%zu symbols, %llu bytes)\n", name, p, ps[p].size(), (unsigned long long)P.size[p]); ++bad; }
			if (injected.empty() && invalid.empty() && want[p] != DECODES) { printf("%s: the oracle does not decode clean part %zu: %u\n", name, p, want[p]); ++bad; }
		}
		const std::vector<uint32_t> got = check(ps, P.bytes, n_bytes, P.off, P.size);
		int shown = 0;
		for (size_t p = 0; p < np; ++p)
			if (got.size() != np || got[p] != want[p]) { ++bad; if (shown++ < 8) printf("%s: part %zu (%zu symbols, %llu bytes): first_bad %u, the oracle's decoder says %u\n", name, p, ps[p].size(), (unsigned long long)P.size[p], got.size() == np ? got[p] : 0u, want[p]); }
	};
	const std::vector<int> none;
	run("(a) clean", parts, clean, clean.bytes.size(), none, none);
	{	// (b) one flipped bit per part of >= 64 bytes, at a random offset <= size - 24
		Packed P = clean; std::vector<int> inj(np, 0);
		for (size_t p = 0; p < np; ++p) if (P.size[p] >= 64) { P.bytes[P.off[p] + rng() % (P.size[p] - 23)] ^= (uint8_t)(1u << (rng() % 8)); inj[p] = 1; }
		run("(b) flipped bit", parts, P, P.bytes.size(), inj, none);
	}
	for (int d = -1; d <= 1; d += 2)
	{	// (c) part_size - 1 and + 1
		Packed P = clean; std::vector<int> inj(np, 1);
		for (size_t p = 0; p < np; ++p) P.size[p] += d;
		run(d < 0 ? "(c) size - 1" : "(c) size + 1", parts, P, P.bytes.size(), inj, none);
	}
	{	// (d) cum + 1 on a symbol of freq == 1; (e) a triple with freq = 0
		std::vector<std::vector<trip_t>> pd = parts, pe = parts; std::vector<int> injd(np, 0), inje(np, 0);
		for (size_t p = 0; p < np; ++p)
		{
			if (parts[p].empty()) continue;
			std::vector<uint32_t> ones;
			for (uint32_t i = 0; i < parts[p].size(); ++i) if (t_freq(parts[p][i]) == 1) ones.push_back(i);
			if (!ones.empty()) { const uint32_t i = ones[rng() % ones.size()]; const trip_t t = parts[p][i]; pd[p][i] = t_pack(t_cum(t) + 1, 1, t_tot(t)); injd[p] = 1; }
			const uint32_t i = (uint32_t)(rng() % parts[p].size()); const trip_t t = parts[p][i];
			pe[p][i] = t_pack(t_cum(t), 0, t_tot(t)); inje[p] = 1;
		}
		run("(d) cum + 1", pd, clean, clean.bytes.size(), injd, none);
		run("(e) freq = 0", pe, clean, clean.bytes.size(), inje, none);
	}
	{	// (f) part_size = ~0 on every third part; (g) a buffer that ends inside the last part
		Packed P = clean; std::vector<int> inv(np, 0);
		for (size_t p = 0; p < np; p += 3) { P.size[p] = ~0ULL; inv[p] = 1; }
		run("(f) size = ~0", parts, P, P.bytes.size(), none, inv);
		std::vector<int> inv2(np, 0); inv2[np - 1] = 1;
		run("(g) buffer ends inside the last part", parts, clean, clean.off[np - 1] + clean.size[np - 1] - 1, none, inv2);
	}
	return bad;
}
} // namespace rcc
