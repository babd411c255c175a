// sketch.hip — the k-mer MinHash sketch on the device (sketch.hpp): cl_kmer_sketch_runs over the sorted keys and the run
// starts that count_range (kmer.hip) derives from them; the host-side accumulator's entry points; the opt-in switch of the context;
// count_range's hook (kmer_sketch_range).
//
// Two walks over head_pos and one small sort:
// k_sketch_bins: persistent blocks of 256 lanes stride over the heads, a head per lane, so a wave loads 64 consecutive 4-byte positions
// (and their right neighbours, the same cache lines but for one), as k_run_spectrum does.  A run with count >= min_count loads its key
// at d_keys[head_pos[j]] — a gather of 8 bytes per QUALIFYING run, a few percent of the runs of real reads at min_count 2 —, hashes it
// and adds 1 to the LDS cell (hash >> 52): 4096 32-bit cells, 16 KB.  The hash is uniform over the bins, so a plain LDS atomic that
// returns nothing does: the ballot path of k_run_spectrum answers a skew (93 % and more of its adds on ONE cell) that does not exist
// here.  At its end a block adds its non-zero cells to the 64-bit totals in memory.  A call covers n < 2^32 keys, so no cell can wrap.
// Cutoff (host): one 32-KB copy back; B = the smallest bin whose cumulative count reaches size (4095 if none does).  The host then knows
// exactly how many candidates lie in the bins <= B: at most size plus one bin's population.
// k_sketch_take: the same walk in units of 4096 heads (16 per lane).  Lanes whose run qualifies with a bin <= B keep (hash, count) in
// registers; one block scan and ONE returning atomic give the unit its place in the candidate arrays (the lesson of k_key_gather: one
// word takes about 88 returning atomics per microsecond).  The host checks that the candidates written are the candidates expected.
// dev_sort_pairs over the 64 hash bits orders the candidates (a few tens of thousands at most for real reads); the first
// min(size, candidates) come back and are merged on the host.
// Bounds by construction: head_pos is read at j and at j + 1 only where j < n_heads and j + 1 < n_heads; a count is formed in 64 bits,
// and a run whose start is not below n or whose count is 0, negative or above n raises the flag, loads no key and indexes nothing; a bin
// is 12 bits of a 64-bit word; a candidate is written below the capacity the host counted only.
#include "common.hpp"
#include "objects.hpp"
#include "sketch.hpp"
#include <memory>

namespace {
constexpr uint32_t SK_TAKE_ITEMS = 16;                  // k_sketch_take: heads per lane and unit
// memory of k_sketch_bins: the SK_BINS totals, then the flag of a malformed position
constexpr uint32_t SK_FLAG = SK_BINS, SK_G_WORDS = SK_FLAG + 1;

// the count of run j, or 0 with *bad set where the positions are malformed; *start is valid where the count is not 0
__device__ inline uint64_t run_count(const uint32_t* __restrict__ head_pos, uint64_t j, uint64_t n_heads, uint64_t n, uint64_t* start, bool* bad)
{
	const uint64_t s = head_pos[j], e = j + 1 < n_heads ? (uint64_t)head_pos[j + 1] : n;
	if (s >= n || e <= s || e - s > n) { *bad = true; return 0; }
	*start = s;
	return e - s;
}

__global__ __launch_bounds__(256) void k_sketch_bins(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ head_pos, uint64_t n_heads, uint64_t n, uint32_t min_count,
                                                     unsigned long long* __restrict__ g)
{
	__shared__ uint32_t s_bin[SK_BINS];
	for (uint32_t c = threadIdx.x; c < SK_BINS; c += 256) s_bin[c] = 0;
	__syncthreads();
	bool bad = false;
	for (uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x; j < n_heads; j += (uint64_t)gridDim.x * 256)
	{
		uint64_t start = 0;
		const uint64_t c = run_count(head_pos, j, n_heads, n, &start, &bad);
		if (c >= min_count && c) atomicAdd(&s_bin[(uint32_t)(sk_hash(keys[start]) >> SK_BIN_SHIFT)], 1u);
	}
	__syncthreads();
	for (uint32_t c = threadIdx.x; c < SK_BINS; c += 256) { const uint32_t v = s_bin[c]; if (v) atomicAdd(g + c, (unsigned long long)v); }
	if (bad) atomicOr(g + SK_FLAG, 1ULL);
}

// the qualifying runs whose hash lies in a bin <= top_bin, appended to (out_hash, out_count) in any order: they are sorted next
__global__ __launch_bounds__(256) void k_sketch_take(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ head_pos, uint64_t n_heads, uint64_t n, uint32_t min_count,
                                                     uint32_t top_bin, uint64_t* __restrict__ out_hash, uint32_t* __restrict__ out_count, uint64_t cap, unsigned long long* __restrict__ counter)
{
	__shared__ uint32_t sh[4];
	__shared__ unsigned long long sbase;
	constexpr uint64_t UNIT = 256 * SK_TAKE_ITEMS;
	const uint64_t n_units = (n_heads + UNIT - 1) / UNIT;
	// (the loop's bounds are the same in every thread of a block: every barrier is met by all of them)
	for (uint64_t u = blockIdx.x; u < n_units; u += gridDim.x)
	{
		uint64_t hash[SK_TAKE_ITEMS]; uint32_t cnt[SK_TAKE_ITEMS]; uint32_t mask = 0, mine = 0;
#pragma unroll
		for (uint32_t i = 0; i < SK_TAKE_ITEMS; ++i)
		{
			const uint64_t j = u * UNIT + (uint64_t)i * 256 + threadIdx.x;
			hash[i] = 0; cnt[i] = 0;
			if (j < n_heads)
			{
				uint64_t start = 0; bool bad = false;
				const uint64_t c = run_count(head_pos, j, n_heads, n, &start, &bad);
				if (c >= min_count && c)
				{
					const uint64_t h = sk_hash(keys[start]);
					if ((uint32_t)(h >> SK_BIN_SHIFT) <= top_bin) { hash[i] = h; cnt[i] = (uint32_t)c; mask |= 1u << i; ++mine; }
				}
			}
		}
		uint32_t total;
		const uint32_t ex = block_excl_scan_256(mine, sh, &total);
		if (threadIdx.x == 0) sbase = total ? atomicAdd(counter, (unsigned long long)total) : 0ULL;
		__syncthreads();
		uint64_t at = sbase + ex;
#pragma unroll
		for (uint32_t i = 0; i < SK_TAKE_ITEMS; ++i) if ((mask >> i) & 1u) { if (at < cap) { out_hash[at] = hash[i]; out_count[at] = cnt[i]; } ++at; }
	}
}

// the sketch of one range merged into *acc; no device selection and no timing scope of its own (count_range runs inside its caller's)
cl_status sketch_runs(cl_ctx* ctx, const uint64_t* d_keys, const uint32_t* d_head_pos, uint64_t n_heads, uint64_t n, uint32_t max_blocks, cl_sketch* acc)
{
	if (!max_blocks) max_blocks = 4 * (uint32_t)std::max(1, ctx->n_cu);
	hipStream_t st = cl_launch_stream(ctx);
	DevBuf<unsigned long long> g; DEV_ALLOC(ctx, g, SK_G_WORDS + 1);             // (the last word: k_sketch_take's counter)
	HIP_TRY(ctx, hipMemsetAsync(g.p, 0, (SK_G_WORDS + 1) * 8, st));
	const uint32_t grid = (uint32_t)std::min<uint64_t>(grid_for(n_heads, 256), max_blocks);
	LAUNCHB(ctx, n_heads * 4.0, k_sketch_bins, grid, 256, d_keys, d_head_pos, n_heads, n, acc->min_count, g.p);
	HIP_TRY(ctx, hipGetLastError());
	std::vector<unsigned long long> h(SK_G_WORDS);
	HIP_TRY(ctx, hipMemcpyAsync(h.data(), g.p, SK_G_WORDS * 8, hipMemcpyDeviceToHost, st));
	HIP_TRY(ctx, hipStreamSynchronize(st));
	if (h[SK_FLAG]) return cl_fail(ctx, CL_E_INVALID, "cl_kmer_sketch_runs: the run starts are not strictly ascending positions below n");
	// the cutoff: the smallest bin whose cumulative count reaches size
	uint64_t qualifying = 0, expect = 0; uint32_t top_bin = SK_BINS - 1;
	for (uint32_t b = 0; b < SK_BINS; ++b) qualifying += h[b];
	for (uint32_t b = 0; b < SK_BINS; ++b) { expect += h[b]; if (expect >= acc->size) { top_bin = b; break; } }
	if (qualifying > n_heads) return cl_fail(ctx, CL_E_INVALID, "cl_kmer_sketch_runs: internal: the bins hold more than every run");
	if (!qualifying) return CL_OK;
	DevBuf<uint64_t> ch; DEV_ALLOC(ctx, ch, expect);
	DevBuf<uint32_t> cc; DEV_ALLOC(ctx, cc, expect);
	const uint32_t tgrid = (uint32_t)std::min<uint64_t>(grid_for(n_heads, 256 * SK_TAKE_ITEMS), max_blocks);
	LAUNCHB(ctx, n_heads * 4.0 + expect * 20.0, k_sketch_take, tgrid, 256, d_keys, d_head_pos, n_heads, n, acc->min_count, top_bin, ch.p, cc.p, expect, g.p + SK_G_WORDS);
	HIP_TRY(ctx, hipGetLastError());
	unsigned long long got = 0;
	HIP_TRY(ctx, hipMemcpyAsync(&got, g.p + SK_G_WORDS, 8, hipMemcpyDeviceToHost, st));
	HIP_TRY(ctx, hipStreamSynchronize(st));
	if (got != expect) return cl_fail(ctx, CL_E_INVALID, "cl_kmer_sketch_runs: internal: the bins and the candidates disagree");
	CL_TRY(dev_sort_pairs(ctx, ch.p, cc.p, expect, 0, 64));
	const uint64_t m = std::min<uint64_t>(acc->size, expect);
	std::vector<uint64_t> hh(m); std::vector<uint32_t> hc(m);
	HIP_TRY(ctx, hipMemcpyAsync(hh.data(), ch.p, m * 8, hipMemcpyDeviceToHost, st));
	HIP_TRY(ctx, hipMemcpyAsync(hc.data(), cc.p, m * 4, hipMemcpyDeviceToHost, st));
	HIP_TRY(ctx, hipStreamSynchronize(st));
	// the range's own sketch, complete and checked before anything of it is merged
	std::vector<cl_sketch_entry> e(m);
	for (uint64_t i = 0; i < m; ++i) e[i] = { hh[i], hc[i] };
	if (!sk_entries_ok(e.data(), m)) return cl_fail(ctx, CL_E_INVALID, "cl_kmer_sketch_runs: the keys of the runs are not distinct");
	sk_merge(acc, e.data(), m, qualifying);
	return CL_OK;
}
} // namespace

extern "C" uint64_t cl_sketch_hash(uint64_t kmer) { return sk_hash(kmer); }
extern "C" cl_status cl_sketch_create(uint32_t size, uint32_t min_count, cl_sketch** out)
{
	if (!out) return CL_E_INVALID;
	*out = new cl_sketch; (*out)->size = size; (*out)->min_count = min_count;
	return CL_OK;
}
extern "C" void cl_sketch_free(cl_sketch* s) { delete s; }
extern "C" cl_status cl_sketch_info(const cl_sketch* s, uint32_t* size, uint32_t* min_count, uint64_t* qualifying, uint64_t* n)
{
	if (!s) return CL_E_INVALID;
	if (size) *size = s->size;
	if (min_count) *min_count = s->min_count;
	if (qualifying) *qualifying = s->qualifying;
	if (n) *n = s->e.size();
	return CL_OK;
}
extern "C" cl_status cl_sketch_entries(const cl_sketch* s, cl_sketch_entry* h_out, uint64_t cap)
{
	if (!s || (!h_out && !s->e.empty())) return CL_E_INVALID;
	if (cap < s->e.size()) return CL_E_CAPACITY;
	if (!s->e.empty()) memcpy(h_out, s->e.data(), s->e.size() * sizeof(cl_sketch_entry));
	return CL_OK;
}
extern "C" cl_status cl_sketch_merge(cl_sketch* dst, const cl_sketch_entry* e, uint64_t n, uint64_t qualifying)
{
	if (!dst || (n && !e) || !sk_params_ok(dst->size, dst->min_count) || !sk_entries_ok(e, n)) return CL_E_INVALID;
	sk_merge(dst, e, n, qualifying);
	return CL_OK;
}

extern "C" cl_status cl_kmer_sketch_runs(cl_ctx* ctx, const uint64_t* d_keys, const uint32_t* d_head_pos, uint64_t n_heads, uint64_t n, uint32_t max_blocks, cl_sketch* acc)
{
	if (!ctx || !acc || (n_heads && (!d_keys || !d_head_pos))) return cl_fail(ctx, CL_E_INVALID, "cl_kmer_sketch_runs: null argument");
	if (!sk_params_ok(acc->size, acc->min_count)) return cl_fail(ctx, CL_E_INVALID, "cl_kmer_sketch_runs: need 1 <= size <= 2^20 and min_count >= 1");
	if (n >= (1ULL << 32) || n_heads > n) return cl_fail(ctx, CL_E_INVALID, "cl_kmer_sketch_runs: need n_heads <= n < 2^32");
	if (!n_heads) return CL_OK;
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	cl_timing_begin(ctx);
	const cl_status s = sketch_runs(ctx, d_keys, d_head_pos, n_heads, n, max_blocks, acc);
	cl_timing_collect(ctx);
	return s;
}

extern "C" cl_status cl_ctx_set_kmer_sketch(cl_ctx* c, int on, uint32_t size, uint32_t min_count)
{
	if (!c) return CL_E_INVALID;
	if (on)
	{
		if (!sk_params_ok(size, min_count)) return cl_fail(c, CL_E_INVALID, "cl_ctx_set_kmer_sketch: need 1 <= size <= 2^20 and min_count >= 1");
		if (!c->sketch_acc) c->sketch_acc = new cl_sketch;
		*c->sketch_acc = cl_sketch(); c->sketch_acc->size = size; c->sketch_acc->min_count = min_count;
	}
	c->kmer_sketch = on != 0;
	return CL_OK;
}
extern "C" cl_status cl_ctx_kmer_sketch(const cl_ctx* c, cl_sketch* out)
{
	if (!c || !out) return CL_E_INVALID;
	if (c->sketch_acc) *out = *c->sketch_acc; else *out = cl_sketch();
	return CL_OK;
}
// Internal (kmer.hip: count_range): the sketch of one counted key range into the context's
cl_status kmer_sketch_range(cl_ctx* ctx, const uint64_t* d_keys, const uint32_t* d_head_pos, uint64_t n_heads, uint64_t n)
{
	if (!n_heads || !ctx->sketch_acc) return CL_OK;
	return sketch_runs(ctx, d_keys, d_head_pos, n_heads, n, 0, ctx->sketch_acc);
}
