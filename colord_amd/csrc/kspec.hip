// kspec.hip — the k-mer count spectrum on the device (kspec.hpp): cl_kmer_spectrum_heads over the run starts that
// count_range (kmer.hip) derives from its sorted keys; the opt-in switch of the context; count_range's hook (kmer_spectrum_range).
//
// k_run_spectrum: persistent blocks of 256 lanes stride over the heads, a head per lane, so a wave loads 64 consecutive 4-byte
// positions (and their right neighbours, which are the same cache lines but for one).  The count of run j is the distance to the
// next head, or to n for the last.  Every block counts into 32-bit cells in LDS: 4096 for the exact values, 33 for the bit lengths
// of the counts from 4096 on, and 33 64-bit sums of those counts — about 17 KB.  A call covers n < 2^32 keys, so it has fewer than
// 2^32 runs and no 32-bit cell can wrap.
// Skew: on real reads 93 % to 99.6 % of the runs have length 1, so a plain LDS atomic per lane would serialise 64 adds on one
// address.  The values 1..KS_WAVE are therefore counted per wave: a ballot per value, whose popcount lane (value - 1) keeps in a
// register until the block's end — one LDS add per wave and value for the whole call.  Every other value is one LDS atomic that
// returns nothing.
// At its end a block adds its NON-ZERO cells to the 64-bit totals in memory by global atomics (a few dozen for real reads, not
// 4162), the maximum by one atomicMax, the flag by one atomicOr.  kmers and distinct are not counted: the host sums them from
// the bins (ks_totals).
// Bounds by construction: head_pos is read at j and at j + 1 only where j < n_heads and j + 1 < n_heads; a count is formed in
// 64 bits and one that is 0, negative or above n (positions not strictly ascending, or not below n) raises the flag and indexes
// nothing; every other count is in 1 .. n < 2^32, so its exact cell is below 4096 where it is used and its bit length at most 32.
#include "common.hpp"
#include "objects.hpp"
#include "kspec.hpp"
#include <memory>

namespace {
constexpr uint32_t KS_WAVE = 8;                         // the values 1..KS_WAVE are counted per wave
// memory: the KS_WORDS totals, then the flag of a malformed position
constexpr uint32_t KS_FLAG = KS_WORDS, KS_G_WORDS = KS_FLAG + 1;

__global__ __launch_bounds__(256) void k_run_spectrum(const uint32_t* __restrict__ head_pos, uint64_t n_heads, uint64_t n, unsigned long long* __restrict__ g)
{
	__shared__ uint32_t s_exact[CL_KSPEC_EXACT];
	__shared__ uint32_t s_big[KS_BINS];
	__shared__ unsigned long long s_mass[KS_BINS];
	__shared__ unsigned long long s_max;
	__shared__ uint32_t s_bad;
	for (uint32_t c = threadIdx.x; c < CL_KSPEC_EXACT; c += 256) s_exact[c] = 0;
	if (threadIdx.x < KS_BINS) { s_big[threadIdx.x] = 0; s_mass[threadIdx.x] = 0; }
	if (threadIdx.x == 0) { s_max = 0; s_bad = 0; }
	__syncthreads();
	const uint32_t lane = threadIdx.x & 63;
	uint32_t small = 0;                                 // lane v - 1 < KS_WAVE: the runs of length v this wave has seen
	uint64_t top = 0; bool bad = false;
	// (the loop's bounds are the same in every thread of a block, so every ballot is over a whole wave)
	for (uint64_t base = (uint64_t)blockIdx.x * 256; base < n_heads; base += (uint64_t)gridDim.x * 256)
	{
		const uint64_t j = base + threadIdx.x;
		uint64_t c = 0;                                 // 0: no run on this lane
		if (j < n_heads)
		{
			const uint64_t start = head_pos[j], end = j + 1 < n_heads ? (uint64_t)head_pos[j + 1] : n;
			if (end <= start || end - start > n) bad = true; else c = end - start;
		}
#pragma unroll
		for (uint32_t v = 1; v <= KS_WAVE; ++v)
		{
			const unsigned long long m = __ballot(c == v);
			if (lane == v - 1) small += (uint32_t)__popcll(m);
		}
		if (c > KS_WAVE)
		{
			if (c < CL_KSPEC_EXACT) atomicAdd(&s_exact[(uint32_t)c], 1u);
			else
			{
				const uint32_t b = 64u - (uint32_t)__clzll((long long)c);   // 13..32
				atomicAdd(&s_big[b], 1u);
				atomicAdd(&s_mass[b], (unsigned long long)c);
			}
		}
		if (c > top) top = c;
	}
	if (lane < KS_WAVE && small) atomicAdd(&s_exact[lane + 1], small);
	for (uint32_t d = 32; d; d >>= 1) { const uint64_t o = __shfl_xor((unsigned long long)top, d); if (o > top) top = o; }
	if (lane == 0 && top) atomicMax(&s_max, (unsigned long long)top);
	if (__ballot(bad) && lane == 0) atomicOr(&s_bad, 1u);
	__syncthreads();
	for (uint32_t c = threadIdx.x; c < CL_KSPEC_EXACT; c += 256) { const uint32_t v = s_exact[c]; if (v) atomicAdd(g + KS_EXACT + c, (unsigned long long)v); }
	if (threadIdx.x < KS_BINS)
	{
		const uint32_t v = s_big[threadIdx.x];
		if (v) { atomicAdd(g + KS_BIG + threadIdx.x, (unsigned long long)v); atomicAdd(g + KS_MASS + threadIdx.x, s_mass[threadIdx.x]); }
	}
	if (threadIdx.x == 0)
	{
		if (s_max) atomicMax(g + KS_MAX, s_max);
		if (s_bad) atomicOr(g + KS_FLAG, 1ULL);
	}
}

// the spectrum of one range into *acc; no device selection and no timing scope of its own (count_range runs inside its caller's)
cl_status spectrum_heads(cl_ctx* ctx, const uint32_t* d_head_pos, uint64_t n_heads, uint64_t n, uint32_t max_blocks, cl_kspec* acc)
{
	if (!max_blocks) max_blocks = 4 * (uint32_t)std::max(1, ctx->n_cu);
	const uint32_t grid = (uint32_t)std::min<uint64_t>(grid_for(n_heads, 256), max_blocks);
	DevBuf<unsigned long long> g; DEV_ALLOC(ctx, g, KS_G_WORDS);
	HIP_TRY(ctx, hipMemsetAsync(g.p, 0, KS_G_WORDS * 8, cl_launch_stream(ctx)));
	LAUNCHB(ctx, n_heads * 4.0, k_run_spectrum, grid, 256, d_head_pos, n_heads, n, g.p);
	HIP_TRY(ctx, hipGetLastError());
	std::vector<unsigned long long> h(KS_G_WORDS);
	HIP_TRY(ctx, hipMemcpyAsync(h.data(), g.p, KS_G_WORDS * 8, hipMemcpyDeviceToHost, cl_launch_stream(ctx)));
	HIP_TRY(ctx, hipStreamSynchronize(cl_launch_stream(ctx)));
	if (h[KS_FLAG]) return cl_fail(ctx, CL_E_INVALID, "cl_kmer_spectrum_heads: the run starts are not strictly ascending positions below n");
	// the range's own spectrum, complete before anything of it is added
	std::unique_ptr<cl_kspec> B(new cl_kspec);
	memcpy(B.get(), h.data(), sizeof(cl_kspec));
	ks_totals(B.get());
	if (B->distinct != n_heads) return cl_fail(ctx, CL_E_INVALID, "cl_kmer_spectrum_heads: internal: the bins do not hold every run");
	ks_add(acc, B.get());
	return CL_OK;
}
} // namespace

extern "C" void cl_kspec_clear(cl_kspec* s) { if (s) ks_clear(s); }
extern "C" void cl_kspec_add(cl_kspec* dst, const cl_kspec* src) { if (dst && src) ks_add(dst, src); }

extern "C" cl_status cl_kmer_spectrum_heads(cl_ctx* ctx, const uint32_t* d_head_pos, uint64_t n_heads, uint64_t n, uint32_t max_blocks, cl_kspec* acc)
{
	if (!ctx || !acc || (n_heads && !d_head_pos)) return cl_fail(ctx, CL_E_INVALID, "cl_kmer_spectrum_heads: null argument");
	if (n >= (1ULL << 32) || n_heads > n) return cl_fail(ctx, CL_E_INVALID, "cl_kmer_spectrum_heads: need n_heads <= n < 2^32");
	if (!n_heads) return CL_OK;
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	cl_timing_begin(ctx);
	const cl_status s = spectrum_heads(ctx, d_head_pos, n_heads, n, max_blocks, acc);
	cl_timing_collect(ctx);
	return s;
}

extern "C" void cl_ctx_set_kmer_spectrum(cl_ctx* c, int on)
{
	if (!c) return;
	if (on && !c->kmer_spectrum) { if (!c->kspec_acc) c->kspec_acc = new cl_kspec; ks_clear(c->kspec_acc); }
	c->kmer_spectrum = on != 0;
}
extern "C" cl_status cl_ctx_kmer_spectrum(const cl_ctx* c, cl_kspec* out)
{
	if (!c || !out) return CL_E_INVALID;
	if (c->kspec_acc) *out = *c->kspec_acc; else ks_clear(out);
	return CL_OK;
}
// Internal (kmer.hip: count_range): the spectrum of one counted key range into the context's total
cl_status kmer_spectrum_range(cl_ctx* ctx, const uint32_t* d_head_pos, uint64_t n_heads, uint64_t n)
{
	if (!n_heads) return CL_OK;
	if (!ctx->kspec_acc) { ctx->kspec_acc = new cl_kspec; ks_clear(ctx->kspec_acc); }
	return spectrum_heads(ctx, d_head_pos, n_heads, n, 0, ctx->kspec_acc);
}
