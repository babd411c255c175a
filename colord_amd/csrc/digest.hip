// digest.hip — the content digests of a chunk on the device (digest.hpp): cl_digest_bases over the 2-bit arena,
// cl_digest_quals and cl_digest_qual_values / cl_qual_values over the quality bytes, all from the INPUT alone; their host counterparts;
// the pipeline's hooks (digest_chunk, digest_values_chunk).
//
// Shape of both kernels (that of k_qual_symbols and k_es_expand): one wave per read, four reads per 256-thread block; the lanes stride
// over the read's arena words / over 8-byte groups of its quality bytes, so a wave reads 512 contiguous bytes a step; the terms of W are
// summed over the wave, lane 0 forms h and the read's term; the four terms of a block are added through LDS and leave as ONE 64-bit
// vector atomic add into one of DG_SLOTS accumulators (by block index: the adds do not queue on one address), which the host adds up.
// Integer addition commutes, so whichever order the blocks arrive in the result is the same.  A long read keeps its wave busy while
// the rest of the launch has drained, exactly as in k_qual_symbols: the launch's tail is the longest read.
// Bounds by construction: a read's arena words are [word_off[r], word_off[r + 1]) and hold all its 32-base blocks; a quality byte is
// loaded only at an index inside [qoff[r], qoff[r + 1]).
#include "common.hpp"
#include "objects.hpp"
#include "digest.hpp"
#include "qual_walk.hpp"

namespace {
constexpr uint32_t DG_SLOTS = 64;                                               // accumulators of a launch: sum[DG_SLOTS], then symbols[DG_SLOTS]

// the block's four (term, symbols) pairs — lane 0 of each wave holds its read's, zero for a wave without a read — into the launch's accumulators
__device__ inline void block_add(uint64_t term, uint64_t syms, unsigned long long* __restrict__ slots)
{
	__shared__ uint64_t s_term[4], s_syms[4];
	const uint32_t w = threadIdx.x >> 6;
	if ((threadIdx.x & 63) == 0) { s_term[w] = term; s_syms[w] = syms; }
	__syncthreads();
	if (threadIdx.x == 0)
	{
		const uint32_t slot = blockIdx.x % DG_SLOTS;
		atomicAdd(slots + slot, (unsigned long long)(s_term[0] + s_term[1] + s_term[2] + s_term[3]));
		atomicAdd(slots + DG_SLOTS + slot, (unsigned long long)(s_syms[0] + s_syms[1] + s_syms[2] + s_syms[3]));
	}
}

__global__ __launch_bounds__(256) void k_digest_bases(const uint64_t* __restrict__ packed, const uint32_t* __restrict__ inv, const uint64_t* __restrict__ word_off,
                                                     const uint32_t* __restrict__ lens, uint32_t n_reads, uint64_t first_read, unsigned long long* __restrict__ slots)
{
	const uint32_t r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
	uint64_t term = 0, syms = 0;
	if (r < n_reads)                                                            // (wave-uniform)
	{
		const uint64_t wb = word_off[r], words = word_off[r + 1] - wb, len = lens[r];
		uint64_t nb = (len + 31) / 32;                                          // blocks that hold bases: the further word of a length that is a multiple of 32 holds the pad base only
		if (nb > words) nb = words;                                             // (never: an arena read has len / 32 + 1 words)
		uint64_t acc = 0;
		for (uint64_t b = lane; b < nb; b += 64)
		{
			uint64_t P = packed[wb + b]; uint32_t I = inv[wb + b];
			dg_block(P, I, len - 32 * b);
			acc += dg_word(P, 2 * b) + dg_word(I, 2 * b + 1);
		}
		const uint64_t W = wave_sum64(acc);
		term = dg_term(dg_read(W, len, DG_DNA), first_read + r); syms = len;
	}
	block_add(term, syms, slots);
}

// the layout of a mode as the kernel takes it: the 96-entry symbol map as twelve words (copied to LDS by twelve scalar loads)
struct DigestQualArg { uint32_t mode, n_bins, navg, per_base; uint64_t map8[12]; };

__global__ __launch_bounds__(256) void k_digest_quals(DigestQualArg cfg, const uint8_t* __restrict__ quals, const uint64_t* __restrict__ qoff,
                                                     uint32_t n_reads, uint64_t first_read, unsigned long long* __restrict__ slots)
{
	__shared__ uint64_t s_map8[12];
#pragma unroll
	for (uint32_t t = 0; t < 12; ++t) if (threadIdx.x == t) s_map8[t] = cfg.map8[t];
	__syncthreads();
	const uint8_t* s_map = (const uint8_t*)s_map8;
	const uint32_t r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
	uint64_t term = 0, syms = 0;
	if (r < n_reads)                                                            // (wave-uniform)
	{
		const uint64_t qb = qoff[r], len = qoff[r + 1] - qb;
		const uint8_t* __restrict__ q = quals + qb;                              // this read's bytes: q[0 .. len)
		const uint32_t navg = cfg.navg;
		// the average bytes (quality_coder_impl.cpp:438-450 and k_qual_symbols): per-bin integer sums and counts first; a_lo = bytes 0..7, a_hi = bytes 8, 9
		uint64_t a_lo = 0, a_hi = 0;
		if (navg)
		{
			uint32_t a[5];
			bin_averages(s_map, cfg.mode == 7, cfg.mode == 7 ? 1u : cfg.n_bins, q, len, lane, a);
#pragma unroll
			for (uint32_t t = 0; t < 5; ++t)
			{
				const uint64_t two = (uint64_t)(a[t] >> 8) | ((uint64_t)(a[t] & 0xff) << 8);
				if (t < 4) a_lo |= two << (16 * t); else a_hi = two;
			}
		}
		// the read's symbols: the average bytes, then (per_base) one symbol a base; word i = symbols 8 i .. 8 i + 7
		const uint64_t n = navg + (cfg.per_base ? len : 0), words = (n + 7) / 8;
		uint64_t acc = 0;
		for (uint64_t i = lane; i < words; i += 64)
		{
			const uint64_t j0 = 8 * i;
			uint64_t w = 0;
			if (j0 >= navg && j0 - navg + 8 <= len)
			{
				const uint64_t v = load_q8(q, j0 - navg);
#pragma unroll
				for (uint32_t k = 0; k < 8; ++k) w |= (uint64_t)s_map[q_value((uint32_t)(v >> (8 * k)) & 0xffu)] << (8 * k);
			}
			else
			{	// the head (average bytes, the first bases behind them) and the tail (fewer than 8 symbols left): byte by byte, inside the read
				for (uint32_t k = 0; k < 8; ++k)
				{
					const uint64_t j = j0 + k;
					if (j >= n) break;
					const uint64_t s = j < navg ? ((j < 8 ? a_lo >> (8 * j) : a_hi >> (8 * (j - 8))) & 0xff) : (uint64_t)s_map[q_value(q[j - navg])];
					w |= s << (8 * k);
				}
			}
			acc += dg_word(w, i);
		}
		const uint64_t W = wave_sum64(acc);
		term = dg_term(dg_read(W, n, DG_QUAL), first_read + r); syms = n;
	}
	block_add(term, syms, slots);
}

// ---- qual-values (digest.hpp, kind 4): the values the decoders will make of a read's quality symbols, from the INPUT qualities -----
__device__ inline void store_q8(uint8_t* __restrict__ p, uint64_t v) { __builtin_memcpy(p, &v, 8); }             // one unaligned 8-byte store inside the read
constexpr uint64_t DG_ASCII8 = 0x2121212121212121ULL;                           // + 33 on each of eight values <= 222: no carry between the bytes

// One wave per read, four reads a block; the walk over the read's bytes is qual_value_walk (qual_walk.hpp).  A group's value word becomes
// the read's digest word i and, under STORE, eight bytes of `values` (value + 33, at the offsets of qoff).  Nothing outside
// [qoff[r], qoff[r + 1]) is loaded or stored for read r.
template<bool STORE>
__global__ __launch_bounds__(256) void k_qual_values(QualValueArg cfg, const uint8_t* __restrict__ quals, const uint64_t* __restrict__ qoff, uint32_t n_reads, uint64_t first_read,
                                                    uint8_t* __restrict__ values, unsigned long long* __restrict__ slots)
{
	__shared__ uint64_t s_tab8[12];
#pragma unroll
	for (uint32_t t = 0; t < 12; ++t) if (threadIdx.x == t) s_tab8[t] = cfg.tab8[t];
	__syncthreads();
	const uint8_t* s_tab = (const uint8_t*)s_tab8;
	const uint32_t r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
	uint64_t term = 0, syms = 0;
	if (r < n_reads)                                                            // (wave-uniform)
	{
		const uint64_t qb = qoff[r], len = qoff[r + 1] - qb;
		const uint8_t* __restrict__ q = quals + qb;                              // this read's bytes: q[0 .. len)
		uint8_t* __restrict__ out = STORE ? values + qb : nullptr;               // its values: out[0 .. len)
		uint64_t acc = 0;
		// the group's word (its values, low byte first) into the digest and, under STORE, into out[8 i .. 8 i + nb)
		qual_value_walk(cfg, s_tab, q, len, lane, [&](uint64_t, uint64_t w, uint64_t i, uint32_t nb) {
			acc += dg_word(w, i);
			if (STORE)
			{
				const uint64_t a = w + DG_ASCII8;
				if (nb == 8) store_q8(out + 8 * i, a); else for (uint32_t k = 0; k < nb; ++k) out[8 * i + k] = (uint8_t)(a >> (8 * k));
			}
		});
		const uint64_t W = wave_sum64(acc);
		term = dg_term(dg_read(W, len, DG_QVAL), first_read + r); syms = len;
	}
	block_add(term, syms, slots);
}

// the accumulators of a launch, zeroed on the launch stream; collected after the kernel
struct DigestRun { DevBuf<unsigned long long> slots; };
cl_status digest_begin(cl_ctx* ctx, DigestRun& run)
{
	DEV_ALLOC(ctx, run.slots, 2 * DG_SLOTS);
	HIP_TRY(ctx, hipMemsetAsync(run.slots.p, 0, 2 * DG_SLOTS * 8, cl_launch_stream(ctx)));
	return CL_OK;
}
cl_status digest_collect(cl_ctx* ctx, DigestRun& run, uint64_t n_reads, cl_digest* acc)
{
	HIP_TRY(ctx, hipGetLastError());
	unsigned long long h[2 * DG_SLOTS];
	HIP_TRY(ctx, hipMemcpyAsync(h, run.slots.p, sizeof(h), hipMemcpyDeviceToHost, cl_launch_stream(ctx)));
	HIP_TRY(ctx, hipStreamSynchronize(cl_launch_stream(ctx)));
	cl_timing_collect(ctx);
	acc->reads += n_reads;
	for (uint32_t i = 0; i < DG_SLOTS; ++i) { acc->sum += h[i]; acc->symbols += h[DG_SLOTS + i]; }
	return CL_OK;
}
} // namespace

extern "C" cl_status cl_digest_bases(cl_ctx* ctx, const cl_reads* R, uint64_t first_read, cl_digest* acc)
{
	if (!ctx || !R || !acc) return cl_fail(ctx, CL_E_INVALID, "cl_digest_bases: null argument");
	if (!dg_range_ok(first_read, R->n_reads)) return cl_fail(ctx, CL_E_INVALID, "cl_digest_bases: first_read + n_reads exceeds 2^63");
	if (!R->n_reads) return CL_OK;
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	DigestRun run; CL_TRY(digest_begin(ctx, run));
	// bytes: 8 + 4 per word, i.e. 0.375 per base, and the offsets and lengths
	LAUNCHB(ctx, 12.0 * R->total_words + 12.0 * R->n_reads, k_digest_bases, grid_for(R->n_reads, 4), 256, (const uint64_t*)R->packed.p, (const uint32_t*)R->inv.p,
	        (const uint64_t*)R->word_off.p, (const uint32_t*)R->lens.p, R->n_reads, first_read, run.slots.p);
	return digest_collect(ctx, run, R->n_reads, acc);
}

extern "C" cl_status cl_digest_quals(cl_ctx* ctx, const cl_qual_params* qparams, const cl_reads* R, const uint8_t* d_quals, const uint64_t* d_qual_off,
                                     uint64_t first_read, cl_digest* acc)
{
	if (!ctx || !qparams || !R || !acc) return cl_fail(ctx, CL_E_INVALID, "cl_digest_quals: null argument");
	DigestQualLayout L;
	if (!dg_qual_layout(qparams, L)) return cl_fail(ctx, CL_E_INVALID, "cl_digest_quals: mode 0..8 with the thresholds of its bins");
	if (L.mode == 8) return CL_OK;                                              // none: nothing is coded, nothing is digested
	if (!dg_range_ok(first_read, R->n_reads)) return cl_fail(ctx, CL_E_INVALID, "cl_digest_quals: first_read + n_reads exceeds 2^63");
	if (!R->n_reads) return CL_OK;
	if (!d_quals || !d_qual_off) return cl_fail(ctx, CL_E_INVALID, "cl_digest_quals: null argument");
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	DigestQualArg A; A.mode = L.mode; A.n_bins = L.n_bins; A.navg = L.navg; A.per_base = L.per_base;
	memcpy(A.map8, L.map, 96);
	DigestRun run; CL_TRY(digest_begin(ctx, run));
	// bytes: every quality byte once, twice where the averages need a pass of their own, and the offsets
	LAUNCHB(ctx, (L.navg && L.per_base ? 2.0 : 1.0) * R->total_bases + 8.0 * R->n_reads, k_digest_quals, grid_for(R->n_reads, 4), 256, A, d_quals, d_qual_off, R->n_reads, first_read, run.slots.p);
	return digest_collect(ctx, run, R->n_reads, acc);
}

extern "C" cl_status cl_digest_bases_host(const uint8_t* h_codes, const uint64_t* h_off, uint64_t n, uint64_t first_read, cl_digest* acc)
{
	return dg_bases_host(h_codes, h_off, n, first_read, acc) ? CL_OK : CL_E_INVALID;
}
extern "C" cl_status cl_digest_bytes_host(uint32_t kind, const uint8_t* h_bytes, const uint64_t* h_off, uint64_t n, uint64_t first_read, cl_digest* acc)
{
	return dg_bytes_host(kind, h_bytes, h_off, n, first_read, acc) ? CL_OK : CL_E_INVALID;
}

extern "C" void cl_ctx_set_digest(cl_ctx* c, int on) { if (c) c->digest = on != 0; }
extern "C" cl_status cl_ctx_digest(const cl_ctx* c, cl_digest* dna, cl_digest* qual)
{
	if (!c) return CL_E_INVALID;
	if (dna) *dna = c->digest_dna;
	if (qual) *qual = c->digest_qual;
	return CL_OK;
}
// ---- qual-values --------------------------------------------------------------------------------------------------------------------
namespace {
// both entry points: acc (digest) and / or d_values (the ASCII values)
cl_status qual_values_run(cl_ctx* ctx, const char* who, const cl_qual_params* qparams, const cl_reads* R, const uint8_t* d_quals, const uint64_t* d_qual_off,
                          uint64_t first_read, uint8_t* d_values, cl_digest* acc)
{
	DigestValueLayout V;
	if (qparams->mode == 8) return CL_OK;                                       // none: nothing is coded, nothing is digested
	if (!dg_value_layout(qparams, V)) return cl_fail(ctx, CL_E_INVALID, std::string(who) + ": mode 0..8 with the thresholds of its bins and, for *-fix, a -D value (<= 222) for every bin");
	if (!dg_range_ok(first_read, R->n_reads)) return cl_fail(ctx, CL_E_INVALID, std::string(who) + ": first_read + n_reads exceeds 2^63");
	if (!R->n_reads) return CL_OK;
	if (!d_quals || !d_qual_off) return cl_fail(ctx, CL_E_INVALID, std::string(who) + ": null argument");
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	QualValueArg A; A.diffuse = V.diffuse; A.bins = V.bins;
	memcpy(A.tab8, V.tab, 96);
	DigestRun run; CL_TRY(digest_begin(ctx, run));
	// bytes: every quality byte once, twice where the averages need a pass of their own, the offsets, and the values where they are stored
	const double bytes = (V.diffuse ? 2.0 : 1.0) * R->total_bases + 8.0 * R->n_reads + (d_values ? 1.0 * R->total_bases : 0.0);
	if (d_values) LAUNCHB(ctx, bytes, k_qual_values<true>, grid_for(R->n_reads, 4), 256, A, d_quals, d_qual_off, R->n_reads, first_read, d_values, run.slots.p);
	else LAUNCHB(ctx, bytes, k_qual_values<false>, grid_for(R->n_reads, 4), 256, A, d_quals, d_qual_off, R->n_reads, first_read, (uint8_t*)nullptr, run.slots.p);
	cl_digest d{ 0, 0, 0 };
	CL_TRY(digest_collect(ctx, run, R->n_reads, &d));
	if (acc) { acc->reads += d.reads; acc->symbols += d.symbols; acc->sum += d.sum; }
	return CL_OK;
}
} // namespace

extern "C" cl_status cl_digest_qual_values(cl_ctx* ctx, const cl_qual_params* qparams, const cl_reads* R, const uint8_t* d_quals, const uint64_t* d_qual_off,
                                           uint64_t first_read, cl_digest* acc)
{
	if (!ctx || !qparams || !R || !acc) return cl_fail(ctx, CL_E_INVALID, "cl_digest_qual_values: null argument");
	return qual_values_run(ctx, "cl_digest_qual_values", qparams, R, d_quals, d_qual_off, first_read, nullptr, acc);
}
extern "C" cl_status cl_qual_values(cl_ctx* ctx, const cl_qual_params* qparams, const cl_reads* R, const uint8_t* d_quals, const uint64_t* d_qual_off,
                                    uint8_t* d_values, uint64_t cap)
{
	if (!ctx || !qparams || !R) return cl_fail(ctx, CL_E_INVALID, "cl_qual_values: null argument");
	if (qparams->mode == 8) return cl_fail(ctx, CL_E_INVALID, "cl_qual_values: mode none codes no quality values");
	if (!R->n_reads) return CL_OK;
	if (!d_qual_off) return cl_fail(ctx, CL_E_INVALID, "cl_qual_values: null argument");
	// the values go to the offsets of d_qual_off: its last one is what d_values must hold (read back before anything is launched)
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	uint64_t end = 0;
	HIP_TRY(ctx, hipMemcpyAsync(&end, d_qual_off + R->n_reads, 8, hipMemcpyDeviceToHost, cl_launch_stream(ctx)));
	HIP_TRY(ctx, hipStreamSynchronize(cl_launch_stream(ctx)));
	if (cap < end) return cl_fail(ctx, CL_E_CAPACITY, "cl_qual_values: d_values holds " + std::to_string(cap) + " bytes, the offsets end at " + std::to_string(end));
	if (end && !d_values) return cl_fail(ctx, CL_E_INVALID, "cl_qual_values: null argument");
	return qual_values_run(ctx, "cl_qual_values", qparams, R, d_quals, d_qual_off, 0, d_values, nullptr);
}
extern "C" cl_status cl_qual_values_host(const cl_qual_params* qparams, const uint8_t* h_quals, const uint64_t* h_off, uint64_t n, uint8_t* h_values)
{
	return dg_qual_values_host(qparams, h_quals, h_off, n, h_values, 0, nullptr) ? CL_OK : CL_E_INVALID;
}
extern "C" cl_status cl_digest_qual_values_host(const uint8_t* h_ascii_quals, const uint64_t* h_off, uint64_t n, uint64_t first_read, cl_digest* acc)
{
	return dg_qual_ascii_host(h_ascii_quals, h_off, n, first_read, acc) ? CL_OK : CL_E_INVALID;
}
extern "C" void cl_ctx_set_digest_values(cl_ctx* c, int on) { if (c) c->digest_values = on != 0; }
extern "C" cl_status cl_ctx_digest_values(const cl_ctx* c, cl_digest* out)
{
	if (!c || !out) return CL_E_INVALID;
	*out = c->digest_qval;
	return CL_OK;
}
// Internal (driver.hip, stream.hip): the digests of one chunk of the input, whose first read is read `first_read`, into the context's totals
cl_status digest_chunk(cl_ctx* ctx, const cl_reads* reads, const cl_qual_params* qparams, const uint8_t* d_quals, const uint64_t* d_base_off, uint64_t first_read)
{
	cl_digest d{ 0, 0, 0 }, q{ 0, 0, 0 };
	CL_TRY(cl_digest_bases(ctx, reads, first_read, &d));
	if (qparams) CL_TRY(cl_digest_quals(ctx, qparams, reads, d_quals, d_base_off, first_read, &q));
	ctx->digest_dna.reads += d.reads; ctx->digest_dna.symbols += d.symbols; ctx->digest_dna.sum += d.sum;
	ctx->digest_qual.reads += q.reads; ctx->digest_qual.symbols += q.symbols; ctx->digest_qual.sum += q.sum;
	return CL_OK;
}
// The same for the qual-values digest alone (cl_ctx_set_digest_values); nothing without a quality stream
cl_status digest_values_chunk(cl_ctx* ctx, const cl_reads* reads, const cl_qual_params* qparams, const uint8_t* d_quals, const uint64_t* d_base_off, uint64_t first_read)
{
	if (!qparams) return CL_OK;
	cl_digest v{ 0, 0, 0 };
	CL_TRY(cl_digest_qual_values(ctx, qparams, reads, d_quals, d_base_off, first_read, &v));
	ctx->digest_qval.reads += v.reads; ctx->digest_qval.symbols += v.symbols; ctx->digest_qval.sum += v.sum;
	return CL_OK;
}
