// sketch.hpp — the k-mer MinHash sketch: of the distinct sampled k-mers that occur at least min_count times, the `size`
// smallest values of cl_sketch_hash(kmer), each with the k-mer's count.  On the device: k_sketch_bins / k_sketch_take (sketch.hip) over
// the run starts of the sorted keys in count_range (kmer.hip).  Here: the hash, the host-side accumulator cl_sketch and its merge rule.
//
// MERGE RULE, used by every path: union by hash, the counts of equal hashes add, the lowest `size` stay; `qualifying` adds.  Exact over
// disjoint key ranges and ranks (no hash can repeat: hash_mm is a bijection).  Exact for independent k-mer sets (--domains K) too: a
// hash in the union's bottom-`size` is in the bottom-`size` of every set that holds it, so its summed count is complete; min_count then
// applies per set and `qualifying` is a sum over the sets.
//
// Under a host compiler alone this header needs no HIP.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <algorithm>
#include <vector>
#include "../../include/colord_hip.h"

#if defined(__HIPCC__)
#define SK_HD __host__ __device__
#else
#define SK_HD
#endif

constexpr uint32_t SK_MAX_SIZE = CL_SKETCH_MAX_SIZE;   // 2^20 entries, 16 MB
constexpr uint32_t SK_BIN_BITS = 12, SK_BINS = 1u << SK_BIN_BITS, SK_BIN_SHIFT = 64 - SK_BIN_BITS;    // the device's cutoff search: 4096 bins by the top bits of the hash
constexpr uint64_t SK_SALT = 0x9E3779B97F4A7C15ULL;

// cl_sketch_hash on the host and on the device (the library exports it under that name): MurmurHash3 fmix64 (common.hpp: hash_mm) of
// the salted k-mer; the salt decouples it from the sampling test hash_mm(kmer) % f == 0
SK_HD static inline uint64_t sk_hash(uint64_t x)
{
	x ^= SK_SALT;
	x ^= x >> 33; x *= 0xff51afd7ed558ccdULL;
	x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ULL;
	x ^= x >> 33;
	return x;
}

struct cl_sketch {
	uint32_t size = 0, min_count = 0;
	uint64_t qualifying = 0;                           // distinct k-mers with count >= min_count, added over calls
	std::vector<cl_sketch_entry> e;                    // n = e.size() <= size entries, strictly ascending by hash, no count 0
};

inline bool sk_params_ok(uint32_t size, uint32_t min_count) { return size >= 1 && size <= SK_MAX_SIZE && min_count >= 1; }
// strictly ascending hashes, no count 0
inline bool sk_entries_ok(const cl_sketch_entry* e, uint64_t n)
{
	for (uint64_t i = 0; i < n; ++i) if (!e[i].count || (i && e[i].hash <= e[i - 1].hash)) return false;
	return true;
}
// the merge rule; e[0 .. n) must be sk_entries_ok
inline void sk_merge(cl_sketch* d, const cl_sketch_entry* e, uint64_t n, uint64_t qualifying)
{
	std::vector<cl_sketch_entry> out; out.reserve(std::min<uint64_t>(d->size, d->e.size() + n));
	size_t a = 0; uint64_t b = 0;
	while (out.size() < d->size && (a < d->e.size() || b < n))
	{
		if (b >= n || (a < d->e.size() && d->e[a].hash < e[b].hash)) out.push_back(d->e[a++]);
		else if (a >= d->e.size() || e[b].hash < d->e[a].hash) out.push_back(e[b++]);
		else { out.push_back({ e[b].hash, d->e[a].count + e[b].count }); ++a; ++b; }
	}
	d->e.swap(out);
	d->qualifying += qualifying;
}
