// qual_ctx.hpp — what the quality ENCODER (qual.hip, k_qual_symbols) and the device DECODER (qual_decode.hip, k_qual_decode) must
// agree on, written once: the coder's configuration, the numbering of the contexts and the context of a position.  The encoder
// computes a position's context from the input, the decoder from what it has decoded so far; both go through the functions below, so
// the partition of the symbols into models cannot drift apart (quality_coder_impl.cpp:88-135, 203-210, 323-339).
#pragma once
#include "common.hpp"

enum { QM_ORIGINAL = 0, QM_QUINARY_AVG, QM_QUAD_AVG, QM_BINARY_AVG, QM_QUINARY_THR, QM_QUAD_THR, QM_BINARY_THR, QM_AVERAGE, QM_NONE };

struct QualCfg {
	int32_t mode, level;
	uint32_t bits_per_sym, n_ctx_sym, ctx_bits;   // previous-symbol history
	uint32_t base_bits;                            // neighbouring-base part of the context
	uint32_t n_sym, sym_bits;                      // alphabet of the per-base family
	uint32_t n_bins, navg;                         // *-avg: bins and coded bytes per read (2 per bin; avg: 2)
	uint32_t max_total, adder;
	uint32_t n_ctx;                                // dense context count of the per-base family
	uint32_t is_avg, is_thr;
	uint32_t hist_radix, n_hist;                   // values a history field takes, and histories: hist_radix ^ n_ctx_sym (qual_hist_radix)
	uint32_t dense_bits;                           // bits of a context id: ids are 0 .. n_ctx - 1 <= 2^dense_bits
	uint8_t map_fwd[96], quant[96];
};
constexpr uint32_t QUAL_BYTE_CTX = 5 * 128 + 256;  // byte family: (bin, floor(prev avg)) and 0x100 + high byte (quality_coder_impl.cpp:821-834)
constexpr uint32_t QUAL_BYTE_MAX_TOTAL = 1u << 18, QUAL_BYTE_ADDER = 8;     // quality_coder.h:41

// ---- context ids ------------------------------------------------------------------------------------
// The id of a context is private to the library: the sort only has to bring equal contexts together in stream order, and the models start
// uniform (k_init_state), so any one-to-one numbering gives the same triples.  Ids are therefore DENSE: a history field holds a symbol
// 0 .. n_sym - 1 or "no such position" (= n_sym), the n_ctx_sym fields are packed in base n_sym + 1, and the base context (and the
// edit-script flags of levels 2 and 3) multiply on top.  4-avg / 4-thr: 125 histories x 256 = 32 000 ids, 15 bits (bit fields: 17);
// 5-*: 216 x 256, 16 bits (17); 2-*: 729 x 256, 18 bits (20).  QM_ORIGINAL keeps its bit fields: the quantised values fill them.
__host__ __device__ inline uint32_t qual_hist_radix(const QualCfg& c) { return c.mode == QM_ORIGINAL ? 1u << c.bits_per_sym : c.n_sym + 1; }
// history so far + the field of the position t + 1 back, whose place value is `place` (1, radix, radix^2 ...)
__host__ __device__ inline uint32_t qual_hist_add(uint32_t hist, uint32_t place, uint32_t field) { return hist + place * field; }
__host__ __device__ inline uint32_t qual_ctx_id(const QualCfg& c, uint32_t hist, uint32_t bctx, uint32_t fl)
{
	return hist + c.n_hist * (bctx | (fl << c.base_bits));
}
// the history field a coded symbol leaves behind (QM_ORIGINAL: its quantised class)
__host__ __device__ inline uint32_t qual_hist_field(const QualCfg& c, uint32_t sym) { return c.mode == QM_ORIGINAL ? (c.quant[sym] & (c.hist_radix - 1)) : sym; }
// The history of position i: the fields of positions i-1 .. i-n (missing = the field's last value), packed in base hist_radix.
// field_back(t) = the field of position i - t, asked for only where i >= t.
template<class FieldBack>
__host__ __device__ inline uint32_t qual_hist_of(const QualCfg& c, uint32_t i, FieldBack field_back)
{
	const uint32_t radix = c.hist_radix, missing = radix - 1;
	uint32_t hist = 0, place = 1;
	for (uint32_t t = 1; t <= c.n_ctx_sym; ++t, place *= radix) hist = qual_hist_add(hist, place, i >= t ? field_back(t) : missing);
	return hist;
}
// the neighbouring bases of position i of a read of len bases: b0 = base i, bm1 / bm2 = the bases before (0 where there is none),
// bp1 = the base behind (0 at the read's end)
__host__ __device__ inline uint32_t qual_base_ctx(const QualCfg& c, uint32_t i, uint32_t b0, uint32_t bm1, uint32_t bm2, uint32_t bp1)
{
	if (c.is_avg) return (bm2 << 6) | (bm1 << 4) | (b0 << 2) | bp1;                       // :203-210
	if (c.is_thr) return b0 | (bm1 << 2) | (bm2 << 4) | (bp1 << 6);                       // :323-339
	if (c.level == 3) return b0 | (bm1 << 2) | (bm2 << 4) | (bp1 << 6);                   // :88-108
	return b0 | (bm1 << 2) | ((uint32_t)(i > 1 && bm2 == bm1) << 4) | (bp1 << 5);
}
// the class bits of a base at levels 2 and 3, from its cl_es_flags byte
__host__ __device__ inline uint32_t qual_flag_bits(uint8_t c) { return (c == 'M' ? 1u : 0u) | (c == 'A' ? 2u : 0u); }
// the whole base context of position i from the arena: word wb on holds the read
__device__ inline uint32_t arena_base(const uint64_t* __restrict__ packed, uint64_t wb, uint32_t p)
{
	return (uint32_t)(packed[wb + (p >> 5)] >> (62 - 2 * (p & 31))) & 3u;
}
__device__ inline uint32_t qual_base_ctx_at(const QualCfg& c, const uint64_t* __restrict__ packed, uint64_t wb, uint32_t i, uint32_t len)
{
	const uint32_t b0 = arena_base(packed, wb, i);
	const uint32_t bm1 = i > 0 ? arena_base(packed, wb, i - 1) : 0;
	const uint32_t bm2 = i > 1 ? arena_base(packed, wb, i - 2) : 0;
	const uint32_t bp1 = i + 1 < len ? arena_base(packed, wb, i + 1) : 0;
	return qual_base_ctx(c, i, b0, bm1, bm2, bp1);
}
// the byte-family contexts of a read's averages (quality_coder_impl.cpp:821-834): high byte of bin t after an average whose floor is
// ctx_p (avg mode: bin 0, ctx_p 0), low byte after the high byte a1
__host__ __device__ inline uint32_t qual_avg_ctx_hi(uint32_t bin, uint32_t ctx_p) { return bin * 128u + ctx_p; }
__host__ __device__ inline uint32_t qual_avg_ctx_lo(uint32_t a1) { return 640u + a1; }

// qual.hip: the configuration of a coder of these parameters (CQualityCoder::Init, quality_coder.cpp:26-247), and its initial model
// tables on the context's stream (counters 1, total = the alphabet)
cl_status qual_make_cfg(cl_ctx* ctx, const cl_qual_params* prm, QualCfg& c);
cl_status qual_init_state(cl_ctx* ctx, uint32_t* d_state, uint64_t n_ctx, uint32_t n_sym);
