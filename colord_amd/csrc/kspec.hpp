// kspec.hpp — the k-mer count spectrum: how many distinct sampled k-mers occur once, twice, and so on, counted from
// the run starts of the sorted keys in count_range (kmer.hip) before the cut at ci and the saturation at cs.  On the device:
// k_run_spectrum (kspec.hip).  Here: the layout of cl_kspec as an array of 64-bit words (what the kernel's totals, the `hipkmers`
// stream and the bindings index) and the helpers.  Every field adds over disjoint key ranges; max_count combines by max.
//
// Under a host compiler alone this header needs no HIP.
#pragma once
#include <string.h>
#include <stddef.h>
#include <stdint.h>
#include "../../include/colord_hip.h"

constexpr uint32_t KS_WORDS = sizeof(cl_kspec) / 8;
#define KS_AT(field) ((uint32_t)(offsetof(cl_kspec, field) / 8))
constexpr uint32_t KS_KMERS = KS_AT(kmers), KS_DISTINCT = KS_AT(distinct), KS_MAX = KS_AT(max_count), KS_EXACT = KS_AT(exact), KS_BIG = KS_AT(big), KS_MASS = KS_AT(big_mass);
constexpr uint32_t KS_BINS = 33;                       // big / big_mass: the bit lengths 0..32 of a count below 2^32 (13..32 are used)
static_assert(sizeof(cl_kspec) == 4165 * 8 && KS_MASS + KS_BINS == KS_WORDS && KS_EXACT == 3, "cl_kspec is 4165 words without padding");

inline void ks_clear(cl_kspec* s) { memset(s, 0, sizeof(*s)); }
inline void ks_add(cl_kspec* d, const cl_kspec* s)
{
	uint64_t* a = (uint64_t*)d; const uint64_t* b = (const uint64_t*)s;
	for (uint32_t i = 0; i < KS_WORDS; ++i) if (i == KS_MAX) { if (b[i] > a[i]) a[i] = b[i]; } else a[i] += b[i];
}
// kmers and distinct from the bins: the sums every other field implies
inline void ks_totals(cl_kspec* s)
{
	s->kmers = s->distinct = 0;
	for (uint32_t c = 0; c < CL_KSPEC_EXACT; ++c) { s->distinct += s->exact[c]; s->kmers += (uint64_t)c * s->exact[c]; }
	for (uint32_t b = 0; b < KS_BINS; ++b) { s->distinct += s->big[b]; s->kmers += s->big_mass[b]; }
}
